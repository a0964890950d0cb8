"""CPU-side checks of `colnde_ensemble_wm_embedded`: the binding against the header, the wrapper's shape and argument rules (raised before any
library call) and the work-list arithmetic of the ensemble launch (csrc/engine_wm_infer.h: wm_ens_groups, wm_ens_grid, wm_ens_range), restated."""
import os
import re

import numpy as np
import pytest

from colnde import _lib
from colnde.nde import check_wm_ens_embed_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 19563


def test_prototype_and_header_agree():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    for name in ("colnde_ensemble_wm_embedded", "colnde_ensemble_wm_embedded_dev"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 22 == len(bound[name]), (name, len(args), len(bound[name]))
        # float and int arguments sit where the binding says
        import ctypes
        for a, t in zip(args, bound[name]):
            assert (t is ctypes.c_float) == bool(re.match(r"float\s+\w+$", a)), (name, a)
            assert (t is ctypes.c_int) == bool(re.match(r"int\s+\w+$", a)), (name, a)
    assert hasattr(_lib.lib(), "colnde_ensemble_wm_embedded_dev")


def _arrays(K=3, n=5, Nz=32):
    z = lambda *s: np.zeros(s, np.float32)
    return dict(weights=z(K, P), state=(z(K, n, Nz), z(K, n, Nz), z(K, n, Nz)), top_flux=z(3, n), dt=60.0, params=z(K, 7), halo_bottom=z(K, 3, n),
                halo_top=z(K, 3, n))


def _check(K=3, **over):
    a = _arrays()
    a.update(over)
    return check_wm_ens_embed_arrays(K, P, 32, a["weights"], a["state"], a["top_flux"], a["dt"], a["params"], a["halo_bottom"], a["halo_top"],
                                     over.get("step", True))


def test_wrapper_checks():
    z = lambda *s: np.zeros(s, np.float32)
    assert _check() == 5
    assert _check(dt=None, step=False) == 5 and _check(params=None, halo_bottom=None, halo_top=None) == 5
    with pytest.raises(ValueError, match=r"weights: expected shape \(3, 19563\) for 3 models"):
        _check(weights=z(2, P))
    with pytest.raises(ValueError, match=r"top_flux: expected shape \(3, 5\)"):
        _check(top_flux=z(5, 3))
    with pytest.raises(ValueError, match=r"top_flux: expected shape \(3, 5\)"):
        _check(top_flux=z(3, 3, 5))
    with pytest.raises(ValueError, match="step=True takes the implicit step and needs dt > 0"):
        _check(dt=None)
    with pytest.raises(ValueError, match="needs dt > 0"):
        _check(dt=0.0)
    with pytest.raises(ValueError, match=r"halo_bottom: expected shape \(3, 3, 5\) for 3 models"):
        _check(halo_bottom=z(2, 3, 5))
    with pytest.raises(ValueError, match=r"halo_top: expected shape \(3, 3, 5\) for 3 models"):
        _check(halo_top=z(3, 5))
    with pytest.raises(ValueError, match=r"u: expected shape \(3, 5, 32\)"):
        _check(state=(z(3, 4, 32), z(3, 5, 32), z(3, 5, 32)))
    with pytest.raises(ValueError, match=r"T: expected shape \(3, n, 32\)"):
        _check(state=(z(5, 32), z(5, 32), z(5, 32)))
    with pytest.raises(ValueError, match=r"params: expected shape \(3, 7\)"):
        _check(params=z(3, 5))


# ---- the work list, restated from csrc/engine_wm_infer.h -----------------------------------------------------------------------------------------
def groups(n_col):
    return ((n_col + 31) // 32 + 3) // 4


def grid_size(K, n_col, n_cu, cap):
    g = min(K * groups(n_col), n_cu)
    if cap > 0:
        g = min(g, cap)
    return max(g, 1)


def ranges(grid, K, n_col):
    """per workgroup b: the (model, first group, group count) runs of its items [b W / grid, (b + 1) W / grid)"""
    G = groups(n_col)
    W = K * G
    out = []
    for b in range(grid):
        first, last = b * W // grid, (b + 1) * W // grid
        runs = []
        it = first
        while it < last:
            m, g = divmod(it, G)
            cnt = min(G - g, last - it)
            runs.append((m, g, cnt))
            it += cnt
        out.append((first, last, runs))
    return out


def test_header_states_the_same_arithmetic():
    src = open(os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc", "engine_wm_infer.h")).read()
    assert "return ((n_col + 31) / 32 + 3) / 4;" in src
    assert "*first = (long long)b * W / grid;" in src and "*last = (long long)(b + 1) * W / grid;" in src
    assert "long long g = W < (long long)n_cu ? W : (long long)n_cu;" in src and "if (grid_cap > 0 && g > grid_cap) g = grid_cap;" in src


def test_work_list_covers_every_group_once():
    for n_col in range(1, 401):
        G = groups(n_col)
        assert (G - 1) * 128 < n_col <= G * 128
        for K in range(1, 10):
            for grid in range(1, 9):
                seen = [[0] * G for _ in range(K)]
                nxt = 0
                for first, last, runs in ranges(grid, K, n_col):
                    assert first == nxt and last >= first                          # contiguous in model-major order, workgroup after workgroup
                    nxt = last
                    it = first
                    for m, g, cnt in runs:
                        assert 0 <= m < K and 0 <= g and g + cnt <= G and cnt >= 1 and it == m * G + g
                        for q in range(g, g + cnt):
                            seen[m][q] += 1
                        it += cnt
                    assert it == last
                    if grid <= K * G:
                        assert last > first                                        # no idle workgroup while there is work for each
                    assert len({m for m, _, _ in runs}) == len(runs)               # one run — one copy of the weight image — per model it touches
                assert nxt == K * G and all(c == 1 for row in seen for c in row), (grid, K, n_col)


def test_grid_choice():
    assert grid_size(8, 18, 256, 0) == 8 and grid_size(64, 8, 256, 0) == 64 and grid_size(512, 8, 256, 0) == 256
    assert grid_size(8, 4096, 256, 0) == 256 and grid_size(2, 300, 256, 0) == 6
    assert grid_size(5, 129, 256, 2) == 2 and grid_size(5, 1, 256, 1) == 1 and grid_size(1, 1, 256, 8) == 1
    for K in range(1, 10):
        for n_col in (1, 128, 129, 400):
            for cap in range(0, 9):
                g = grid_size(K, n_col, 256, cap)
                assert 1 <= g <= K * groups(n_col) and (cap == 0 or g <= cap)
