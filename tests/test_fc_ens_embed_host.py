"""CPU checks of the ensemble free-convection embedding (`colnde_ensemble_fc_embedded`): what needs no device of the header, the bindings and the
Python checker; the float64 reference of the conv members pinned against a literal loop over the Flux chain; the GPU test's inputs shown
robust to the switch; and the float32 restatement's own distance from float64, from which the conv tolerances come (tests/fc_ens_embed_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib
from colnde.free_convection import conv_n_params, conv_to_dense
from oracle import nde_oracle as O
from tests import fc_ens_embed_cases as C
from tests import fc_embed_restatement as R
from tests.conv_cases import dense_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("colnde_ensemble_fc_embedded", "colnde_ensemble_fc_embedded_dev")


# ---------------------------------------------------------------------------------------------- ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colnde.h")).read(), flags=re.S)


def test_header_bindings_and_library_move_together():
    text = _header()
    protos = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
              for m in re.finditer(r"\b(colnde_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.lib()
    for name in NEW:
        assert protos[name] == 13 == len(bound[name]), name
        assert hasattr(L, name), "%s declared in colnde.h but not exported" % name
    assert re.search(r"#define\s+COLNDE_VERSION\s+106\b", text) and L.colnde_version() == 106
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    assert "(:colnde_ensemble_fc_embedded, libcolnde)" in jl
    for doc in ("INTEGRATION.md", "README.md"):
        assert "colnde_ensemble_fc_embedded" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_refused_by_name(name):
    L = _lib.lib()
    z = np.zeros(64, np.float32)
    P = z.ctypes.data_as(ctypes.c_void_p)
    rc = getattr(L, name)(None, P, P, P, None, None, ctypes.c_float(1000.0), ctypes.c_float(600.0), ctypes.c_float(1.0), P, P, None, 1)
    msg = L.colnde_last_error().decode()
    assert rc != 0 and name in msg and "null handle" in msg, msg


# ---------------------------------------------------------------------------------------------- the array checker
def test_array_rules_of_fc_embedded():
    chk = colnde.check_fc_ens_embed_arrays
    K, Nz, n = 3, 32, 5
    P, Pc = C.config(Nz).n_params, conv_n_params(Nz, 3)
    assert colnde.nde.fc_ensemble_n_params(C.config(Nz), 3) == Pc != P
    f = lambda *s: np.zeros(s, np.float32)
    W, Wc, T, top, hb = f(K, P), f(K, Pc), f(K, n, Nz), f(n), f(K, n)
    assert chk(K, P, Nz, W, T, top, 600.0) == n
    assert chk(K, P, Nz, None, T, top, 600.0, (hb, None)) == n                  # weights=None: the packed images
    assert chk(K, Pc, Nz, Wc, T, top, None, (None, hb), step=False) == n        # faces only: no dt
    assert chk(1, Pc, Nz, Wc[:1], T[:1], top, 600.0, faces=False) == n          # a single conv handle: K = 1
    assert chk(K, P, Nz, W, T, top, 600.0, None, True, True, f(K, n, Nz), T) == n
    with pytest.raises(ValueError, match="n_models must be >= 1"):
        chk(0, P, Nz, W[:0], T[:0], top, 600.0)
    with pytest.raises(ValueError, match=r"T: expected shape \(2, n, 32\) for 2 models"):
        chk(2, P, Nz, W[:2], T, top, 600.0)
    with pytest.raises(ValueError, match="weights: expected shape"):
        chk(2, P, Nz, W, T[:2], top, 600.0)
    with pytest.raises(ValueError, match="weights: expected shape .*leads with its filter"):
        chk(K, Pc, Nz, W, T, top, 600.0)                                          # vectors of the plain length on a conv ensemble
    with pytest.raises(ValueError, match="one output group .*only dz_out"):
        chk(K, P, Nz, W, T, top, 600.0, dz_out=f(K, n, Nz))                       # a half-given step group
    with pytest.raises(ValueError, match="one output group .*only T_out"):
        chk(K, P, Nz, W, T, top, 600.0, T_out=T)
    with pytest.raises(ValueError, match="T_out: expected shape"):
        chk(K, P, Nz, W, T, top, 600.0, dz_out=f(K, n, Nz), T_out=f(K, n, Nz + 1))
    with pytest.raises(ValueError, match="step=False writes none"):
        chk(K, P, Nz, W, T, top, None, step=False, dz_out=f(K, n, Nz), T_out=T)
    with pytest.raises(ValueError, match="halo_top: expected shape"):
        chk(K, P, Nz, W, T, top, 600.0, (None, f(n)))                             # the single-model shape
    with pytest.raises(ValueError, match="halo_bottom: expected shape"):
        chk(K, P, Nz, W, T, top, 600.0, (f(K, n + 1), None))
    with pytest.raises(ValueError, match="halos must be"):
        chk(K, P, Nz, W, T, top, 600.0, (hb,))
    with pytest.raises(ValueError, match="top_flux: expected shape"):
        chk(K, P, Nz, W, T, f(K, n), 600.0)                                       # the top flux is shared, not per member
    with pytest.raises(ValueError, match="T: expected float32"):
        chk(K, P, Nz, W, T.astype(np.float64), top, 600.0)
    with pytest.raises(ValueError, match="needs dt > 0"):
        chk(K, P, Nz, W, T, top, None)
    with pytest.raises(ValueError, match="needs dt > 0"):
        chk(K, P, Nz, W, T, top, 0.0)
    with pytest.raises(ValueError, match="nothing to compute"):
        chk(K, P, Nz, W, T, top, None, step=False, faces=False)


# ---------------------------------------------------------------------------------------------- the conv reference, pinned
def _flux_chain(theta, Nz, c, x):
    """The literal Flux chain of train_free_convection_nde.jl:110-122 in float64, one column at a time: reshape, Conv((c, 1), 1 => 1, relu) with
    NNlib's flipped kernel, reshape, Dense(M, 4Nz, relu), Dense(4Nz, 4Nz, relu), Dense(4Nz, Nz - 1)."""
    theta = np.asarray(theta, np.float64)
    H, M = 4 * Nz, Nz - c + 1
    w, b, off = theta[:c], theta[c], c + 1
    mats = []
    for ni, no in ((M, H), (H, H), (H, Nz - 1)):
        Wl = theta[off:off + ni * no].reshape((no, ni), order="F")
        off += ni * no
        mats.append((Wl, theta[off:off + no]))
        off += no
    assert off == theta.size
    out = np.empty((x.shape[0], Nz - 1))
    for col in range(x.shape[0]):
        y = np.empty(M)
        for i in range(M):
            s = b
            for kk in range(c):                                                  # conv flips: out[i] = sum_k w[k] x[i + c - 1 - k]
                s += w[kk] * x[col, i + c - 1 - kk]
            y[i] = max(s, 0.0)
        a = y
        for li, (Wl, bl) in enumerate(mats):
            a = Wl @ a + bl
            if li < 2:
                a = np.maximum(a, 0.0)
        out[col] = a
    return out


@pytest.mark.parametrize("c", C.CONVS)
@pytest.mark.parametrize("Nz", [32, 64])
def test_conv_to_dense_on_the_oracle_is_the_flux_chain(Nz, c):
    cfg = C.config(Nz)
    T = C.states(Nz)[0][1].astype(np.float64)
    for k in range(C.K_MODELS):
        theta = C.weights(Nz, c)[k].astype(np.float64)
        m = O.Model(dense_cfg(cfg, c), np.float64)
        x = ((19.65 + T / 20.0) - m.mu_T) / m.s_T
        y, _ = O.mlp_forward(m.unpack(conv_to_dense(theta, Nz, c))[0], m.acts, x)
        lit = _flux_chain(theta, Nz, c, x)
        assert np.abs(lit).max() > 0 and (np.abs(y - lit).max() <= 1e-12 * np.abs(lit).max())
        # ... and the filter takes both relu branches (an all-zero or all-linear filter output would show little)
        pre = np.array([[theta[c] + sum(theta[kk] * x[col, i + c - 1 - kk] for kk in range(c)) for i in range(Nz - c + 1)] for col in range(x.shape[0])])
        assert (pre > 0).mean() > 0.1 and (pre <= 0).mean() > 0.1


# ---------------------------------------------------------------------------------------------- inputs robust to the switch
@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("n", C.SIZES + (C.N_ALL,))
@pytest.mark.parametrize("Nz", [32, 64])
def test_inputs_take_the_same_switches_in_float32_and_float64(Nz, n, halo):
    T, top, hb, ht = C.case(Nz, n)
    assert T.shape == (C.K_MODELS, n, Nz) and top.shape == (n,) and hb.shape == ht.shape == (C.K_MODELS, n)
    C.same_switches(T, (hb, ht) if halo else None)
    assert not np.array_equal(T[0], T[1])                                        # every member its own state


def test_members_differ_and_cover_the_switch_patterns():
    for c in (0,) + C.CONVS:
        W = C.weights(32, c)
        assert not np.array_equal(W[0], W[1]) and not np.array_equal(W[1], W[2])
    T, top, hb, ht = C.states(32)
    f = R.face_switch(T[0], (hb[0], ht[0]))
    assert (~f[0]).all() and f[1].all() and (f[2, 1:] != f[2, :-1]).all()


# ---------------------------------------------------------------------------------------------- tolerances from the reference's own error
def test_float32_restatement_distance_sets_the_gpu_tolerances():
    d = C.distances()
    print("fc_ens_embed float32-restatement distances:", {"/".join(str(x) for x in k): "%.3e" % v for k, v in sorted(d.items(), key=str)})
    for kind in ("plain", "conv"):
        for K_ca in (C.K_STEP, C.K_DIAG):
            assert 0 < 10.0 * d[(kind, "faces", K_ca)] <= C.FACES_BOUND[(kind, K_ca)] * 1.0001, (kind, K_ca, d[(kind, "faces", K_ca)])
            assert C.FACES_BOUND[(kind, K_ca)] <= 12.0 * d[(kind, "faces", K_ca)]      # ... and no wider than the rule gives
    assert 0 < 10.0 * d[("conv", "dz")] <= C.DZ_REL_CONV * 1.0001 <= 12.0 * d[("conv", "dz")] * 1.0001
    # the plain members' fixed bounds are not tighter than float32 itself allows
    assert d[("plain", "dz")] < C.DZ_REL_PLAIN
