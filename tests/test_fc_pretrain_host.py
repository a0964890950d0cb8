"""CPU-side checks of the ensemble T -> wT pre-training (`colnde_ensemble_pretrain_flux_dev`): declared, exported, bound in ctypes and wrapped in Julia with
the header's arity; `check_fc_pretrain_arrays` refuses wrong shapes, dtypes and an out-of-range order before any handle is touched; the float64 reference
of conv + penalty (tests/fc_pretrain_cases.py) against central finite differences; and what float32 alone costs for this arithmetic — the yardstick of
tests/test_gpu_fc_pretrain.py, whose every tolerance must lie between 10x and 12x the float32 restatement's largest error over the cases it is used on."""
import functools
import os
import re

import numpy as np
import pytest

from colnde import _lib, synthetic
from colnde.free_convection import conv_n_params, pretrain_orders, train_neural_network_ensemble
from colnde.nde import check_fc_pretrain_arrays
from tests import fc_pretrain_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "colnde_ensemble_pretrain_flux_dev"
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


def test_null_handle_is_refused_with_the_calls_name():
    import ctypes
    L = _lib.lib()
    z, f, bt = ctypes.c_void_p(), ctypes.c_float(), (ctypes.c_double * 2)(0.9, 0.999)
    assert L.colnde_ensemble_pretrain_flux_dev(None, z, z, z, z, z, z, z, 1, z, 0, z, 0.9, 0.999, 1e-8, bt, 1, ctypes.byref(f)) != 0
    msg = L.colnde_last_error().decode()
    assert NAME in msg and "null handle" in msg


def test_check_fc_pretrain_arrays_refuses_shapes_dtypes_and_orders():
    cfg = FC.handle_cfg(32)
    K, n, P, f = 3, 5, cfg.n_params, np.float32
    good = dict(theta=np.zeros((K, P), f), T=np.zeros((n, 32), f), bcs=np.zeros((n, 2), f), fluxes=np.zeros((n, 33), f),
                order=np.tile(np.arange(n, dtype=np.int32), (K, 1)), coeff=np.zeros(K, f), etas=np.zeros(K, f), m=np.zeros((K, P), f), v=np.zeros((K, P), f))
    assert check_fc_pretrain_arrays(cfg, K, **good) == n
    assert check_fc_pretrain_arrays(cfg, K, good["theta"], good["T"], good["bcs"], good["fluxes"]) == n        # the optional ones left out
    rep = dict(good, order=np.array([[4, 4, 0, 0, 1]] * K, np.int32))
    assert check_fc_pretrain_arrays(cfg, K, **rep) == n                                                          # an index may repeat
    Pc = conv_n_params(32, 3)
    assert check_fc_pretrain_arrays(cfg, K, np.zeros((K, Pc), f), good["T"], good["bcs"], good["fluxes"], conv=3) == n
    bad = [
        (dict(theta=np.zeros((K, P + 1), f)), "theta"), (dict(theta=np.zeros((K + 1, P), f)), "theta"), (dict(theta=np.zeros(K * P, f)), "theta"),
        (dict(theta=np.zeros((K, Pc), f)), "theta"),                                                            # the conv count on a plain ensemble
        (dict(m=np.zeros((K, P - 1), f)), "m"), (dict(v=np.zeros((1, P), f)), "v"),
        (dict(T=np.zeros((n, 31), f)), "T"), (dict(T=np.zeros((0, 32), f)), "T"), (dict(T=np.zeros(32, f)), "T"),
        (dict(bcs=np.zeros((n, 6), f)), "bcs"), (dict(bcs=np.zeros((n + 1, 2), f)), "bcs"),
        (dict(fluxes=np.zeros((n, 32), f)), "fluxes"), (dict(fluxes=np.zeros((n - 1, 33), f)), "fluxes"),
        (dict(coeff=np.zeros(K + 1, f)), "coeff"), (dict(etas=np.zeros((K, 1), f)), "etas"),
        (dict(order=np.arange(n, dtype=np.int32)), "order"), (dict(order=np.zeros((K, n + 1), np.int32)), "order"),
        (dict(theta=np.zeros((K, P), np.float64)), "theta: expected float32"), (dict(T=np.zeros((n, 32), np.float64)), "T: expected float32"),
        (dict(fluxes=np.zeros((n, 33), np.float16)), "fluxes: expected float32"), (dict(etas=np.zeros(K, np.float64)), "etas: expected float32"),
        (dict(coeff=np.zeros(K, np.int32)), "coeff: expected float32"), (dict(m=np.zeros((K, P), np.float64)), "m: expected float32"),
        (dict(order=np.zeros((K, n), np.int64)), "order: expected int32"), (dict(order=np.zeros((K, n), f)), "order: expected int32"),
        (dict(order=np.full((K, n), n, np.int32)), r"order: entries must lie in 0\.\.4"), (dict(order=np.array([[0, 1, 2, 3, -1]] * K, np.int32)), "order: entries"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            check_fc_pretrain_arrays(cfg, K, **dict(good, **kw))
    with pytest.raises(ValueError, match="theta"):
        check_fc_pretrain_arrays(cfg, K, good["theta"], good["T"], good["bcs"], good["fluxes"], conv=3)          # the plain count on a conv ensemble
    with pytest.raises(ValueError, match="conv = 9"):
        check_fc_pretrain_arrays(cfg, K, good["theta"], good["T"], good["bcs"], good["fluxes"], conv=9)
    with pytest.raises(ValueError, match="n_models"):
        check_fc_pretrain_arrays(cfg, 0, good["theta"], good["T"], good["bcs"], good["fluxes"])
    with pytest.raises(ValueError, match="free-convection"):
        check_fc_pretrain_arrays(synthetic.wind_mixing_problem(1, n_frames=2).cfg, K, good["theta"], good["T"], good["bcs"], good["fluxes"])


def test_driver_checks_its_arrays_before_the_handle_is_touched():
    class NoHandle:                        # any library call through it is an error of the test
        cfg, n_models, conv, device = FC.handle_cfg(32), 2, 0, 0

        def pretrain_flux(self, *a, **kw):
            raise AssertionError("the handle was touched")

    ens, f = NoHandle(), np.float32
    P, n = ens.cfg.n_params, 4
    W, T, B, Y = np.zeros((2, P), f), np.zeros((n, 32), f), np.zeros((n, 2), f), np.zeros((n, 33), f)
    for args, kw, what in (((np.zeros((2, P - 1), f), T, B, Y), {}, "theta"), ((W, T[:, :31], B, Y), {}, "T"), ((W, T, B, Y[:3]), {}, "fluxes"),
                           ((W, T, B, Y), dict(causal_coeff=np.zeros(3)), "coeff"), ((W, T, B, Y), dict(etas=np.zeros(2)), "etas"),
                           ((W, T, B, Y), dict(seeds=(1, 2, 3)), "seeds"), ((W, T, B, Y), dict(optimizers=(("rmsprop", 1e-3),)), "optimizers")):
        with pytest.raises(ValueError, match=what):
            train_neural_network_ensemble(ens, *args, **kw)
    o = pretrain_orders((5, 6), 7, 3)
    assert o.shape == (3, 2, 7) and o.dtype == np.int32 and all(sorted(r) == list(range(7)) for r in o.reshape(-1, 7))
    assert not np.array_equal(o[0, 0], o[1, 0]) and not np.array_equal(o[0, 0], o[0, 1])                        # fresh per pass, different per model
    np.testing.assert_array_equal(o, pretrain_orders((5, 6), 7, 3))


@pytest.mark.parametrize("Nz,c,coeff", [(32, 3, 0.3), (64, 8, 1.0), (32, 0, 1.0), (32, 2, 0.0)])
def test_float64_gradient_of_conv_and_penalty_matches_finite_differences(Nz, c, coeff):
    s = FC.samples(Nz, c, 1, 3)
    th = s.W[0].astype(np.float64)
    _, g = FC.loss_grad64(s, th, 0, coeff)
    rng = np.random.default_rng(0)
    mask = FC.causal_mask(s.cfg, c)
    dirs = [rng.standard_normal(th.shape) for _ in range(2)]
    dirs.append(np.where(mask, rng.standard_normal(th.shape), 0.0))                       # along the penalised entries only
    if c:
        d = np.zeros_like(th)
        d[:c + 1] = rng.standard_normal(c + 1)                                            # along the filter only
        dirs.append(d)
    for d in dirs:
        d = d / np.linalg.norm(d)
        h = 1e-6
        fd = (FC.loss_grad64(s, th + h * d, 0, coeff)[0] - FC.loss_grad64(s, th - h * d, 0, coeff)[0]) / (2 * h)
        assert np.isclose(fd, g @ d, rtol=1e-6, atol=1e-12), (fd, g @ d)


def test_the_cases_are_non_trivial_and_away_from_the_kinks():
    for case, (Nz, c, coeff) in FC.GRAD_CASES.items():
        s, ref = FC.grad_reference(case)
        assert s.W.shape == (3, FC.n_params(s.cfg, c)) and not np.array_equal(s.W[0], s.W[1])
        for k in range(3):
            assert FC._min_kink(s.cfg, c, s.W[k], s.X, s.B) > FC.PC.KINK_MARGIN
            assert ref[k][0] > 1e-3 and all(np.linalg.norm(ref[k][1][sl]) > 1e-3 for _, sl in FC.blocks(s.cfg, c)), case
    s = FC.samples(32, 0, 1, 3)
    m = FC.causal_mask(s.cfg, 0)
    H = 128
    assert m[1 * H + 0] and not m[0] and not m[1 * H + 1] and m[31 * H + 30] and not m[31 * H + 31] and not m[32 * H:].any()       # W1[r, q] at q H + r, r < q


# ---- what float32 alone costs: the yardstick of tests/test_gpu_fc_pretrain.py, measured without the kernel ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _f32_worst():
    """Largest float32-restatement error per tolerance constant of the GPU module, over the cases that constant is used on."""
    w = dict(TOL_LOSS=0.0, TOL_W=0.0, TOL_B=0.0, TOL_DESCENT_W=0.0, TOL_DESCENT_B=0.0, TOL_M=0.0, TOL_V=0.0, TOL_THETA=0.0, TOL_MOVED=0.0,
             TOL_DRV_THETA=0.0, TOL_DRV_HIST=0.0)

    def up(name, e):
        w[name] = max(w[name], float(e))

    for case, (Nz, c, coeff) in FC.GRAD_CASES.items():                                       # single-sample loss and gradient
        s, ref = FC.grad_reference(case)
        for k in range(3):
            loss, g = FC.loss_grad32(s, s.W[k], 0, coeff[k])
            e_loss, e_W, e_b, _ = FC.grad_errors(s, coeff[k], loss, g, ref[k])
            up("TOL_LOSS", e_loss), up("TOL_W", e_W), up("TOL_B", e_b)
    for case, (Nz, c, coeff) in FC.DESCENT_CASES.items():                                    # one Descent step, the gradient read back out of it
        s, ref = FC.descent_reference(case)
        for k in range(3):
            loss, g = FC.loss_grad32(s, s.W[k], 0, coeff[k])
            th = FC.descent32(s.W[k], g, FC.ETA_DESCENT)
            e_loss, e_W, e_b, _ = FC.grad_errors(s, coeff[k], loss, FC.descent_gradient(s.W[k], th, FC.ETA_DESCENT), ref[k])
            up("TOL_LOSS", e_loss), up("TOL_DESCENT_W", e_W), up("TOL_DESCENT_B", e_b)
    s, ref = FC.sequence_reference()                                                         # an ADAM pass, then a Descent pass
    _, got = FC.sequence(True)
    for k in range(3):
        (th1, m, v, bt, l1), (th2, l2) = got[k]
        (r1, rm, rv, rbt, rl1), (r2, rl2) = ref[k]
        assert bt == rbt
        for e in (FC.pass_errors(s, s.W[k], th1, r1, np.mean(l1), rl1, m, rm, v, rv), FC.pass_errors(s, r1, th2, r2, np.mean(l2), rl2)):
            assert e["moved_least"] > 1e-3                                                   # every block moved
            up("TOL_LOSS", e["loss"]), up("TOL_THETA", e["theta"]), up("TOL_MOVED", e["moved"])
            if "m" in e:
                up("TOL_M", e["m"]), up("TOL_V", e["v"])
    s, th, hist = FC.driver_reference()                                                      # the driver's loop
    _, th32, hist32 = FC.driver(True)
    for k in range(FC.DRV_K):
        up("TOL_DRV_THETA", max(FC.block_errors(s.cfg, FC.DRV_C, th32[k], th[k]).values()))
    up("TOL_DRV_HIST", (np.abs(hist32 - hist) / hist).max())
    assert (hist[-1] < hist[0]).all()
    return w


def test_gpu_tolerances_are_ten_to_twelve_times_the_float32_restatement():
    """Each constant of the GPU module lies between 10x and 12x the largest error of the float32 restatement over the cases it judges (run with -s for the
    figures): a bound from the precision of the format, not from the kernel, and not stale on the loose side."""
    from tests import test_gpu_fc_pretrain as G
    worst = _f32_worst()
    for name, e in worst.items():
        tol = getattr(G, name)
        print("%-14s float32 restatement %.3e   tolerance %.2e = %.2fx" % (name, e, tol, tol / e))
        assert 10 * e <= tol <= 12 * e, (name, e, tol)
