"""CPU-side checks of the ensemble flux pre-training of a wind-mixing sweep (`colnde_ensemble_pretrain_wm_flux_dev`): declared, exported, bound in ctypes and
wrapped in Julia with the header's arity; `check_wm_pretrain_arrays` and the driver refuse wrong shapes, dtypes, nets and an out-of-range order before any
handle is touched; the constant sets of tests/wm_pretrain_cases.py differ in every constant and are stable at the helper config's sub-step count; and what
float32 alone costs for this arithmetic under each model's constants — the yardstick of tests/test_gpu_wm_pretrain.py, whose every tolerance must lie
between 10x and 12x the float32 restatement's largest error over the cases it is used on."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from colnde import _lib
from colnde.config import to_c_config
from colnde.nde import check_wm_pretrain_arrays, wm_pretrain_nets_mask
from colnde.wind_mixing import train_NN_ensemble
from colnde.flux_compat import ADAM
from tests import pretrain_cases as PC
from tests import wm_pretrain_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "colnde_ensemble_pretrain_wm_flux_dev"
ARITY = 18


def test_symbol_declared_exported_bound_and_wrapped_with_the_headers_arity():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % NAME, header, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == ARITY, m
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == ARITY and hasattr(_lib.lib(), NAME)
    assert "#define COLNDE_VERSION 106" in text                                                # additive: the version stays
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    m = re.search(r"ccall\(\(:%s,\s*libcolnde\),\s*Cint,\s*\(([^)]*)\)" % NAME, jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == ARITY, m
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_null_handle_is_refused_with_the_calls_name():
    L = _lib.lib()
    z, f, bt = ctypes.c_void_p(), ctypes.c_float(), (ctypes.c_double * 2)(0.9, 0.999)
    assert getattr(L, NAME)(None, 7, z, z, z, z, z, z, z, 1, 1e-2, z, 0.9, 0.999, 1e-8, bt, 1, ctypes.byref(f)) != 0
    msg = L.colnde_last_error().decode()
    assert NAME in msg and "null handle" in msg
    assert list(bt) == [0.9, 0.999]


def test_check_wm_pretrain_arrays_refuses_shapes_dtypes_and_orders():
    cfg = WC.samples("mpp_zero_weights").cfg
    K, n, P, f = 3, 5, cfg.n_params, np.float32
    good = dict(theta=np.zeros((K, P), f), profiles=np.zeros((n, 96), f), bcs=np.zeros((n, 6), f), fluxes=np.zeros((3, n, 33), f),
                order=np.tile(np.arange(n, dtype=np.int32), (K, 3, 1)), etas=np.zeros((K, 3), f), m=np.zeros((K, P), f), v=np.zeros((K, P), f))
    assert check_wm_pretrain_arrays(cfg, K, **good) == n
    assert check_wm_pretrain_arrays(cfg, K, good["theta"], good["profiles"], good["bcs"], good["fluxes"]) == n      # the optional ones left out
    assert check_wm_pretrain_arrays(cfg, K, **dict(good, order=np.tile(np.array([4, 4, 0, 0, 1], np.int32), (K, 3, 1)))) == n     # an index may repeat
    bad = [
        (dict(theta=np.zeros((K, P + 1), f)), "theta"), (dict(theta=np.zeros((K + 1, P), f)), "theta"), (dict(theta=np.zeros(K * P, f)), "theta"),
        (dict(m=np.zeros((K, P - 1), f)), "m"), (dict(v=np.zeros((1, P), f)), "v"),
        (dict(profiles=np.zeros((n, 32), f)), "profiles"), (dict(profiles=np.zeros((0, 96), f)), "profiles"), (dict(profiles=np.zeros(96, f)), "profiles"),
        (dict(bcs=np.zeros((n, 2), f)), "bcs"), (dict(bcs=np.zeros((n + 1, 6), f)), "bcs"),
        (dict(fluxes=np.zeros((n, 33), f)), "fluxes"), (dict(fluxes=np.zeros((3, n, 32), f)), "fluxes"), (dict(fluxes=np.zeros((3, n - 1, 33), f)), "fluxes"),
        (dict(fluxes=np.zeros((n, 3, 33), f)), "fluxes"),
        (dict(etas=np.zeros(K, f)), "etas"), (dict(etas=np.zeros((3, K + 1), f)), "etas"),
        (dict(order=np.tile(np.arange(n, dtype=np.int32), (K, 1))), "order"), (dict(order=np.zeros((K, 3, n + 1), np.int32)), "order"),
        (dict(order=np.zeros((3 * K, n), np.int32)), "order"),
        (dict(theta=np.zeros((K, P), np.float64)), "theta: expected float32"), (dict(profiles=np.zeros((n, 96), np.float64)), "profiles: expected float32"),
        (dict(fluxes=np.zeros((3, n, 33), np.float16)), "fluxes: expected float32"), (dict(etas=np.zeros((K, 3), np.float64)), "etas: expected float32"),
        (dict(m=np.zeros((K, P), np.float64)), "m: expected float32"), (dict(bcs=np.zeros((n, 6), np.int32)), "bcs: expected float32"),
        (dict(order=np.zeros((K, 3, n), np.int64)), "order: expected int32"), (dict(order=np.zeros((K, 3, n), f)), "order: expected int32"),
        (dict(order=np.full((K, 3, n), n, np.int32)), r"order: entries must lie in 0\.\.4"),
        (dict(order=np.tile(np.array([0, 1, 2, 3, -1], np.int32), (K, 3, 1))), "order: entries"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            check_wm_pretrain_arrays(cfg, K, **dict(good, **kw))
    with pytest.raises(ValueError, match="n_models"):
        check_wm_pretrain_arrays(cfg, 0, good["theta"], good["profiles"], good["bcs"], good["fluxes"])
    fc = PC.sample("fc-gs0").cfg
    with pytest.raises(ValueError, match="wind-mixing"):
        check_wm_pretrain_arrays(fc, K, good["theta"], good["profiles"], good["bcs"], good["fluxes"])


def test_nets_mask():
    assert wm_pretrain_nets_mask(("uw", "vw", "wT")) == 7 and wm_pretrain_nets_mask("wT") == 4 and wm_pretrain_nets_mask(["vw", "uw", "uw"]) == 3
    assert wm_pretrain_nets_mask(5) == 5 and wm_pretrain_nets_mask(np.int32(1)) == 1
    for bad in (0, 8, -1, (), ("uw", "wt"), ("T",), True, 2.0, None):
        with pytest.raises(ValueError, match="nets"):
            wm_pretrain_nets_mask(bad)


def test_driver_checks_its_arrays_before_the_handle_is_touched():
    class NoHandle:                        # any library call through it is an error of the test
        cfg, n_models, device = WC.samples("mpp_zero_weights").cfg, 2, 0

        def pretrain_fluxes(self, *a, **kw):
            raise AssertionError("the handle was touched")

    ens, f = NoHandle(), np.float32
    P, n = ens.cfg.n_params, 4
    W, X, B, Y = np.zeros((2, P), f), np.zeros((n, 96), f), np.zeros((n, 6), f), np.zeros((3, n, 33), f)
    opts = [ADAM(1e-3), ADAM(1e-4)]
    for args, kw, what in (((np.zeros((2, P - 1), f), X, B, Y, opts, [1, 1]), {}, "theta"), ((W, X[:, :95], B, Y, opts, [1, 1]), {}, "profiles"),
                           ((W, X, B, Y[:2], opts, [1, 1]), {}, "fluxes"), ((W, X, B, Y, opts, [1]), {}, "train_epochs"), ((W, X, B, Y, opts, [1, -1]), {}, "train_epochs"),
                           ((W, X, B, Y, opts, [1, 1]), dict(etas=np.zeros(2)), "etas"), ((W, X, B, Y, opts, [1, 1]), dict(etas=np.zeros((2, 2, 2))), "etas"),
                           ((W, X, B, Y, opts, [1, 1]), dict(seeds=(1, 2, 3)), "seeds"), ((W, X, B, Y, opts, [1, 1]), dict(nets=("uw", "wt")), "nets"),
                           ((W, X, B, Y, opts, [1, 1]), dict(nets=0), "nets")):
        with pytest.raises(ValueError, match=what):
            train_NN_ensemble(ens, *args, **kw)


def test_constant_sets_differ_in_every_constant_and_are_stable_at_the_helpers_substeps():
    ph = np.vstack([WC.PHYSICS, WC.PHYSICS_ALT[None]])
    for q in range(5):
        assert len(set(ph[:, q].tolist())) == len(ph), q                                       # pairwise different, the replacement set included
    assert np.float32(0.1) in WC.PHYSICS[:, 2] and (WC.PHYSICS[:, 4] != 1).any()
    L = _lib.lib()
    for cond in WC.MPP_CONDS + WC.PLAIN_CONDS:
        for n in (1, WC.N):
            s = WC.samples(cond, n)
            rows = ph if cond in WC.MPP_CONDS else [None]
            for row in rows:
                cfg = s.cfg if row is None else WC.model_cfg(s.cfg, row)
                c, keep = to_c_config(cfg, 1)
                need = L.colnde_min_substeps(ctypes.byref(c))
                assert 1 <= need <= s.cfg.substeps, (cond, row, need, s.cfg.substeps)
    for a in (WC.ORDERS.reshape(9, -1), WC.driver_orders()[0].reshape(6, -1)):
        assert len({tuple(r) for r in a.tolist()}) == len(a)                                   # every chain walks its own order
    assert all(len(set(r)) < len(r) for r in WC.ORDERS.reshape(9, -1).tolist())                # ... with repeats
    assert len(set(WC.ETAS[0].tolist())) == 3 and not np.array_equal(WC.ETAS[0], WC.ETAS[1])


def test_the_chains_are_non_trivial_and_the_constants_matter():
    for cond in WC.MPP_CONDS:
        s, ref = WC.grad_reference(cond)
        assert s.W.shape == (3, s.cfg.n_params) and not np.array_equal(s.W[0], s.W[1])
        for (k, j), (loss, g) in ref.items():
            assert loss > 1e-3 and all(np.linalg.norm(g[sl]) > 1e-6 for _, sl in PC.blocks(s.cfg)), (cond, k, j)
            c0 = WC.chain(s, k, j, physics=None)                                               # the same weights under the config's constants
            if k > 0:
                assert abs(PC.oracle_loss_grad(c0, c0.theta[c0.net], 0)[0] - loss) > 1e-4 * loss, (cond, k, j)         # a hundred times TOL_LOSS


# ---- what float32 alone costs: the yardstick of tests/test_gpu_wm_pretrain.py, measured without the kernel --------------------------------------------
@functools.lru_cache(maxsize=None)
def _f32_worst():
    """Largest float32-restatement error per tolerance constant of the GPU module, over the cases that constant is used on."""
    w = dict(TOL_LOSS=0.0, TOL_W=0.0, TOL_B=0.0, TOL_M=0.0, TOL_V=0.0, TOL_THETA=0.0, TOL_MOVED=0.0, TOL_DRV_THETA=0.0, TOL_DRV_HIST=0.0)

    def up(name, e):
        w[name] = max(w[name], float(e))

    for cond in WC.MPP_CONDS:                                                                  # single-sample loss and gradient
        s, ref = WC.grad_reference(cond)
        for k, j, c in WC.chains(s):
            loss, g = PC.f32_loss_grad(c, c.theta[c.net], 0)
            e_loss, e_W, e_b, _ = WC.grad_errors(c, loss, g, ref[k, j])
            up("TOL_LOSS", e_loss), up("TOL_W", e_W), up("TOL_B", e_b)
    s, ref = WC.sequence_reference()                                                           # one ADAM pass over the per-chain orders
    _, got = WC.sequence(True)
    for k, j, c in WC.chains(s):
        th, m, v, bt, losses = got[k, j]
        assert bt == ref[k, j][3]
        e = WC.pass_errors(c, th, m, v, np.mean(losses), ref[k, j])
        assert e["moved_least"] > 1e-3                                                         # every block moved
        up("TOL_LOSS", e["loss"]), up("TOL_THETA", e["theta"]), up("TOL_MOVED", e["moved"]), up("TOL_M", e["m"]), up("TOL_V", e["v"])
    s, th, hist = WC.driver_reference()                                                        # the driver's loop
    _, th32, hist32 = WC.driver(True)
    for k in range(WC.DRV_K):
        for j in range(3):
            sl = slice(j * s.cfg.net_size, (j + 1) * s.cfg.net_size)
            up("TOL_DRV_THETA", max(PC.block_errors(s.cfg, th32[k, sl], th[k, sl]).values()))
    up("TOL_DRV_HIST", (np.abs(hist32 - hist) / hist).max())
    assert (hist[-1] < hist[0]).all()
    return w


def test_gpu_tolerances_are_ten_to_twelve_times_the_float32_restatement():
    """Each constant of the GPU module lies between 10x and 12x the largest error of the float32 restatement over the cases it judges (run with -s for the
    figures): a bound from the precision of the format, not from the kernel, and not stale on the loose side."""
    from tests import test_gpu_wm_pretrain as G
    worst = _f32_worst()
    for name, e in worst.items():
        tol = getattr(G, name)
        print("%-14s float32 restatement %.3e   tolerance %.2e = %.2fx" % (name, e, tol, tol / e))
        assert 10 * e <= tol <= 12 * e, (name, e, tol)
