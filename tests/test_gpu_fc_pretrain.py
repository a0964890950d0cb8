"""`fc_pretrain_ens_kernel` (csrc/engine_fc_pretrain.hip, `colnde_ensemble_pretrain_flux_dev`): the T -> wT pre-training of all K networks of a
free-convection ensemble in one launch.  Rows against the single handle's bits (A), independence of the models (B), a grid larger than the machine (C),
the gradient of the conv chain and of the penalty read out of the ADAM moments (D), Descent (E), the sequence semantics of an ADAM pass followed by a
Descent pass (F), the driver's loop (G) and the refusals (H).  One column, n_save = 3 throughout.

Tolerances: 10x what float32 alone costs for this arithmetic, measured WITHOUT the kernel by the float32 restatement of tests/fc_pretrain_cases.py, largest
over the cases each constant judges (tests/test_fc_pretrain_host.py holds every constant between 10x and 12x its measurement).  Beside each: the
restatement's largest error / the kernel's largest error on an MI355X."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde.flux_compat import ADAM
from colnde.free_convection import train_neural_network_ensemble
from tests import fc_pretrain_cases as FC
from tests import pretrain_cases as PC

pytestmark = pytest.mark.gpu

#                          float32 restatement (CPU)   kernel (MI355X)
TOL_LOSS = 1.0e-6        # 9.69e-8   2.08e-7   single-sample losses, the mean of a pass's pre-update losses
TOL_W = 3.5e-6           # 3.44e-7   9.42e-7   gradient, weight blocks (the filter's taps, W1's masked and unmasked entries under a penalty)
TOL_B = 3.3e-5           # 3.20e-6   3.72e-6   gradient, bias blocks (the filter's bias)
TOL_DESCENT_W = 2.1e-4   # 2.04e-5   2.04e-5   (theta_0 - theta) / eta after one Descent step: the rounding of theta itself, over eta |g|
TOL_DESCENT_B = 7.6e-5   # 7.56e-6   7.56e-6
TOL_M = 1.8e-5           # 1.76e-6   3.17e-6   one pass of ADAM(1e-3) over eight visits, largest over the blocks
TOL_V = 2.8e-6           # 2.76e-7   4.92e-7
TOL_THETA = 4.4e-6       # 4.31e-7   3.46e-7   relative to |theta|, after the ADAM pass and after the Descent pass
TOL_MOVED = 9.5e-5       # 9.42e-6   9.36e-6   relative to the distance the pass moved the block
TOL_DRV_THETA = 1.7e-6   # 1.69e-7   1.58e-7   the driver: 2 + 2 epochs over 8 samples
TOL_DRV_HIST = 1.1e-6    # 1.07e-7   1.20e-7   ... its training-set losses
# exact bounds: bit equality, and one ulp for v (D)

F32_TINY = float(np.finfo(np.float32).tiny)
SC = [0, 0, 1, 0, 0, 0]


def _t(a, dt=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(torch.device("cuda", 0))


def _np(t):
    return t.detach().cpu().numpy()


def _ens(Nz, K, c=0):
    return colnde.FreeConvectionEnsemble(FC.handle_cfg(Nz), 1, K, conv=c)


def _run(ens, s, W, kind, etas, orders=None, coeff=None, m=None, v=None, beta=(0.9, 0.999), beta_t=None, update=True, dev=None):
    """One call; (theta, m, v, beta_t, losses) as numpy afterwards (m, v: None under Descent without moments)."""
    X, B, Y = dev if dev is not None else (_t(s.X), _t(s.B), _t(s.Y))
    theta = _t(W)
    adam = kind == "adam"
    m = _t(np.zeros_like(W) if m is None else m) if adam else None
    v = _t(np.zeros_like(W) if v is None else v) if adam else None
    bt = list(beta_t) if beta_t is not None else [beta[0], beta[1]]
    loss = ens.pretrain_flux(theta, m, v, X, B, Y, None if orders is None else _t(orders, np.int32), None if coeff is None else _t(coeff), kind,
                             None if etas is None else _t(etas), beta, 1e-8, bt, update=update)
    assert loss.shape == (W.shape[0],) and loss.dtype == np.float32
    return _np(theta), None if m is None else _np(m), None if v is None else _np(v), bt, loss


def _single(eng, s, w, order, eta=1e-3, update=True):
    """`colnde_pretrain_flux_dev` on the single handle `eng` for one model's weights, gradient_scaling = 0: (theta, m, v, beta_t, loss)."""
    X, B, Y = _t(s.X), _t(s.B), _t(s.Y)
    theta, m, v = _t(w), _t(np.zeros_like(w)), _t(np.zeros_like(w))
    opt = ADAM(eta)
    loss = eng.pretrain_flux(2, theta, m, v, X, B, Y, None if order is None else _t(order, np.int32), 0.0, opt, update=update)
    return _np(theta), _np(m), _np(v), list(opt.beta_t), np.float32(loss)


def _assert_row_is_the_single_handles(got, k, ref):
    theta, m, v, bt, loss = got
    for a, r in ((theta, ref[0]), (m, ref[1]), (v, ref[2])):
        np.testing.assert_array_equal(a[k], r)
    assert loss[k] == ref[4] and bt == ref[3]


# ---- A: bits ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz", [32, 64])
def test_rows_hold_the_bits_of_the_single_handle(Nz):
    """Plain ensemble, K = 3, ADAM(1e-3) with c_k = 0, PC.SEQ_ORDER over 8 samples: theta, m, v, the loss and beta_t of every row are those of
    `colnde_pretrain_flux_dev` on a single handle with gradient_scaling = 0; the same with update=False."""
    s = FC.samples(Nz, 0, FC.SEQ_N, 3)
    cfg = FC.handle_cfg(Nz)
    order = np.asarray(PC.SEQ_ORDER, np.int32)
    etas = np.full(3, 1e-3, np.float32)
    with _ens(Nz, 3) as ens:
        got = _run(ens, s, s.W, "adam", etas, np.tile(order, (3, 1)), coeff=np.zeros(3, np.float32))
        got_none = _run(ens, s, s.W, "adam", etas, None, coeff=None)                                        # order NULL, coeff NULL
        ev = _run(ens, s, s.W, "adam", etas, np.tile(order, (3, 1)), coeff=np.zeros(3, np.float32), beta_t=[0.81, 0.998001], update=False)
    with colnde.ColumnNDE(cfg, 1) as eng:
        for k in range(3):
            _assert_row_is_the_single_handles(got, k, _single(eng, s, s.W[k], order))
            _assert_row_is_the_single_handles(got_none, k, _single(eng, s, s.W[k], None))
            ref = _single(eng, s, s.W[k], order, update=False)
            assert ev[4][k] == ref[4]
            assert not np.array_equal(got[0][k], s.W[k])                                                    # the pass moved the weights
    np.testing.assert_array_equal(ev[0], s.W)                                                               # update=False: nothing written
    assert not ev[1].any() and not ev[2].any() and ev[3] == [0.81, 0.998001]


# ---- B: independence --------------------------------------------------------------------------------------------------------------------------------------
def test_changing_one_model_leaves_the_others_bits():
    s = FC.samples(32, 0, FC.SEQ_N, 3)
    orders, coeff, etas = FC.SEQ_ORDERS.copy(), np.array([0.3, 1.0, 0.0], np.float32), np.array([1e-3, 2e-3, 5e-4], np.float32)
    with _ens(32, 3) as ens:
        dev = (_t(s.X), _t(s.B), _t(s.Y))
        base = _run(ens, s, s.W, "adam", etas, orders, coeff, dev=dev)
        for what in ("weights", "rate", "order", "coefficient"):
            W, e, o, c = s.W.copy(), etas.copy(), orders.copy(), coeff.copy()
            if what == "weights":
                W[1] = W[1] * np.float32(1.01)
            elif what == "rate":
                e[1] = 3e-3
            elif what == "order":
                o[1] = o[1][::-1]
            else:
                c[1] = 0.5
            got = _run(ens, s, W, "adam", e, o, c, dev=dev)
            for k in (0, 2):
                for a, b in zip(got[:3], base[:3]):
                    np.testing.assert_array_equal(a[k], b[k], err_msg=what)
                assert got[4][k] == base[4][k], what
            assert not np.array_equal(got[0][1], base[0][1]), what
            assert got[3] == base[3]


# ---- C: a grid larger than the machine --------------------------------------------------------------------------------------------------------------------
def test_more_models_than_compute_units():
    """K = 260 workgroups on 256 CUs, 3 samples: the first, a middle and the last row are the single handle's bits."""
    K = 260
    s = FC.samples(32, 0, 3, 3)
    cfg = FC.handle_cfg(32)
    rng = np.random.default_rng(7)
    W = (s.W[0][None, :] * (1.0 + 0.05 * rng.standard_normal((K, 1)))).astype(np.float32)
    with _ens(32, K) as ens:
        got = _run(ens, s, W, "adam", np.full(K, 1e-3, np.float32))
    with colnde.ColumnNDE(cfg, 1) as eng:
        for k in (0, 128, 259):
            _assert_row_is_the_single_handles(got, k, _single(eng, s, W[k], None))
    assert not np.array_equal(got[0][0], got[0][259])


# ---- D: the gradient through the moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FC.GRAD_CASES))
def test_single_sample_loss_and_gradient(case):
    """One sample, zero moments, beta1 = beta2 = 0.5, beta_t = (0.5, 0.5), eta = 0: m = g / 2 exactly, so g = 2 m; v = fl(g g) / 2 ties v to the same g
    within one ulp; theta keeps its bits.  Per block against float64 — the filter's w and b are blocks of their own, and under a penalty the masked
    and the unmasked entries of W1 are."""
    Nz, c, coeff = FC.GRAD_CASES[case]
    s, ref = FC.grad_reference(case)
    with _ens(Nz, 3, c) as ens:
        theta, m, v, bt, loss = _run(ens, s, s.W, "adam", np.zeros(3, np.float32), None, np.asarray(coeff, np.float32), beta=(0.5, 0.5), beta_t=[0.5, 0.5])
    np.testing.assert_array_equal(theta, s.W)
    assert bt == [0.25, 0.25]
    for k in range(3):
        g = (np.float32(2) * m[k]).astype(np.float32)
        e_loss, e_W, e_b, errs = FC.grad_errors(s, coeff[k], float(loss[k]), g, ref[k])
        v_ref = g * g / np.float32(2)
        ulps = float((np.abs(v[k].astype(np.float64) - v_ref) / np.maximum(np.spacing(v_ref), F32_TINY)).max())
        print("%s model %d (c_k = %g): loss %.6e rel err %.2e; gradient blocks %s; v off by %.2f ulp at most" %
              (case, k, coeff[k], loss[k], e_loss, " ".join("%s %.2e" % kv for kv in errs.items()), ulps))
        assert np.isfinite(g).all() and ulps <= 1.0
        assert e_loss < TOL_LOSS
        assert e_W < TOL_W, errs
        assert e_b < TOL_B, errs


# ---- E: Descent -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FC.DESCENT_CASES))
def test_descent_step(case):
    """One sample, Descent(1e-2), no moments: (theta_0 - theta) / eta is the gradient, per block against float64; the running powers stay."""
    Nz, c, coeff = FC.DESCENT_CASES[case]
    s, ref = FC.descent_reference(case)
    with _ens(Nz, 3, c) as ens:
        theta, m, v, bt, loss = _run(ens, s, s.W, "descent", np.full(3, FC.ETA_DESCENT, np.float32), None, np.asarray(coeff, np.float32), beta_t=[0.81, 0.998001])
    assert m is None and v is None and bt == [0.81, 0.998001]
    for k in range(3):
        e_loss, e_W, e_b, errs = FC.grad_errors(s, coeff[k], float(loss[k]), FC.descent_gradient(s.W[k], theta[k], FC.ETA_DESCENT), ref[k])
        print("%s model %d (c_k = %g): loss rel err %.2e; (theta_0 - theta) / eta blocks %s" % (case, k, coeff[k], e_loss, " ".join("%s %.2e" % kv for kv in errs.items())))
        assert e_loss < TOL_LOSS
        assert e_W < TOL_DESCENT_W, errs
        assert e_b < TOL_DESCENT_B, errs


def test_descent_leaves_given_moments_alone():
    s = FC.samples(32, 0, 1, 3)
    with _ens(32, 3) as ens:
        theta, X, B, Y = _t(s.W), _t(s.X), _t(s.B), _t(s.Y)
        m, v = _t(np.full_like(s.W, 7.0)), _t(np.full_like(s.W, 7.0))
        ens.pretrain_flux(theta, m, v, X, B, Y, None, None, 1, _t(np.full(3, 1e-2, np.float32)))
    assert (_np(m) == 7.0).all() and (_np(v) == 7.0).all() and not np.array_equal(_np(theta), s.W)


# ---- F: sequence semantics --------------------------------------------------------------------------------------------------------------------------------
def test_adam_pass_then_descent_pass_follow_the_sequential_loop():
    """Conv c = 3 with the penalty (c_k = 1, 0, 0.3), per-model orders that differ (with repeats): one ADAM pass, then one Descent pass from where it
    ended, against the float64 sequential loop — theta per block and per distance moved, m, v, and the mean of the pre-update losses, penalty included."""
    s, ref = FC.sequence_reference()
    coeff = np.asarray(FC.SEQ_COEFF, np.float32)
    with _ens(FC.SEQ_NZ, 3, FC.SEQ_C) as ens:
        dev = (_t(s.X), _t(s.B), _t(s.Y))
        th1, m, v, bt, l1 = _run(ens, s, s.W, "adam", np.full(3, FC.ETA_ADAM, np.float32), FC.SEQ_ORDERS, coeff, dev=dev)
        th2, _, _, bt2, l2 = _run(ens, s, th1, "descent", np.full(3, FC.ETA_DESCENT, np.float32), FC.SEQ_ORDERS, coeff, beta_t=bt, dev=dev)
    assert bt2 == bt
    for k in range(3):
        (r1, rm, rv, rbt, rl1), (r2, rl2) = ref[k]
        np.testing.assert_allclose(bt, rbt, rtol=1e-15)
        ea = FC.pass_errors(s, s.W[k], th1[k], r1, l1[k], rl1, m[k], rm, v[k], rv)
        ed = FC.pass_errors(s, r1, th2[k], r2, l2[k], rl2)
        print("model %d ADAM pass: %s\n        Descent pass: %s" % (k, " ".join("%s %.2e" % kv for kv in ea.items()), " ".join("%s %.2e" % kv for kv in ed.items())))
        for e in (ea, ed):
            assert e["moved_least"] > 1e-3                       # every block moved
            assert e["loss"] < TOL_LOSS                          # the mean of each sample's loss just before its own update
            assert e["theta"] < TOL_THETA and e["moved"] < TOL_MOVED, e
        assert ea["m"] < TOL_M and ea["v"] < TOL_V, ea


# ---- G: the driver ----------------------------------------------------------------------------------------------------------------------------------------
def test_driver_follows_the_float64_loop():
    """`train_neural_network_ensemble`, K = 2, 2 ADAM + 2 Descent epochs over 8 samples, model 1 with the penalty, against the float64 loop on the same
    permutations; the training-set loss ends below where it started."""
    s, th_ref, hist_ref = FC.driver_reference()
    with _ens(FC.DRV_NZ, FC.DRV_K, FC.DRV_C) as ens:
        theta, hist = train_neural_network_ensemble(ens, s.W, s.X, s.B, s.Y, epochs=FC.DRV_EPOCHS, optimizers=FC.DRV_OPTIMIZERS, causal_coeff=FC.DRV_COEFF,
                                                    seeds=FC.DRV_SEEDS)
    assert theta.shape == s.W.shape and hist.shape == (4, FC.DRV_K)
    e_hist = np.abs(hist - hist_ref) / hist_ref
    e_th = [max(FC.block_errors(s.cfg, FC.DRV_C, theta[k], th_ref[k]).values()) for k in range(FC.DRV_K)]
    print("driver: theta %s, history rel err at most %.2e; losses %s" % (" ".join("%.2e" % e for e in e_th), e_hist.max(), hist.tolist()))
    assert (hist[-1] < hist[0]).all()
    assert max(e_th) < TOL_DRV_THETA and e_hist.max() < TOL_DRV_HIST


# ---- H: refusals ------------------------------------------------------------------------------------------------------------------------------------------
NAME = "colnde_ensemble_pretrain_flux_dev"


def test_refusals_name_the_call_and_leave_the_handle_usable():
    from colnde.nde import ClosureColumns, ColumnNDEEnsemble
    from colnde import synthetic
    from oracle import nde_oracle as O
    L = colnde._lib.lib()
    s = FC.samples(32, 0, 1, 3)
    p = synthetic.free_convection_problem(1, Nz=32, n_save=3, substeps=2, t_end=0.01)
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    theta, m, v, X, B, Y, eta = _t(s.W), _t(np.zeros_like(s.W)), _t(np.zeros_like(s.W)), _t(s.X), _t(s.B), _t(s.Y), _t(np.full(3, 1e-3, np.float32))
    loss = (ctypes.c_float * 3)()

    def call(h, th=theta, mm=m, vv=v, x=X, n=1, opt=0, bt=(0.9, 0.999), update=1, lo=loss):
        P = lambda a: a.data_ptr() if a is not None else None
        bt = (ctypes.c_double * 2)(*bt) if bt is not None else None
        rc = L.colnde_ensemble_pretrain_flux_dev(h, P(th), P(mm), P(vv), P(x), P(B), P(Y), None, n, None, opt, P(eta), 0.9, 0.999, 1e-8, bt, update, lo)
        return rc, L.colnde_last_error().decode()

    def refused(h, what, **kw):
        rc, msg = call(h, **kw)
        assert rc != 0 and NAME in msg and what in msg, (what, msg)

    with _ens(32, 3) as ens:
        ens.set_problem(p.x0, p.bcs, truth)
        refused(None, "null handle")
        refused(ens._h, "null pointer", th=None)
        refused(ens._h, "null pointer", x=None)
        refused(ens._h, "null pointer", bt=None)
        refused(ens._h, "null pointer", lo=None)
        for o in (2, -1):
            refused(ens._h, "optimiser = %d" % o, opt=o)
        refused(ens._h, "moments", mm=None)
        refused(ens._h, "moments", vv=None)
        for bt in ((1.0, 0.5), (0.5, 1.0), (float("nan"), 0.5)):
            refused(ens._h, "beta", bt=bt)
        for n in (0, -3):
            refused(ens._h, "n_samples", n=n)
        assert call(ens._h, th=_t(s.W), mm=None, vv=None, opt=1, bt=(1.0, 1.0))[0] == 0   # Descent needs neither moments nor running powers below 1
        with pytest.raises(ValueError, match="moments"):                                     # ... and the wrapper's own checks
            ens.pretrain_flux(_t(s.W), None, None, X, B, Y, None, None, "adam", eta)
        with pytest.raises(ValueError, match="opt_kind"):
            ens.pretrain_flux(_t(s.W), m, v, X, B, Y, None, None, "rmsprop", eta)
        with pytest.raises(ValueError, match="order"):
            ens.pretrain_flux(_t(s.W), m, v, X, B, Y, _t(np.full((3, 1), 1, np.int32), np.int32), None, "adam", eta)
        # colnde_pretrain_flux_dev still refuses the ensemble
        z, f, bt = ctypes.c_void_p(), ctypes.c_float(), (ctypes.c_double * 2)(0.9, 0.999)
        assert L.colnde_pretrain_flux_dev(ens._h, 2, z, z, z, z, z, z, z, 1, 0.0, 1e-3, 0.9, 0.999, 1e-8, bt, 0, ctypes.byref(f)) != 0
        msg = L.colnde_last_error().decode()
        assert "colnde_pretrain_flux_dev" in msg and "ensemble of 3 models" in msg
        np.testing.assert_array_equal(_np(theta), s.W)                                       # nothing was written by a refused call
        assert not _np(m).any() and not _np(v).any()
        assert np.isfinite(ens.loss(s.W, SC)).all()                                          # the handle is still good
    with colnde.ColumnNDE(FC.handle_cfg(32), 1) as single:
        refused(single._h, "single-model handle")
    with colnde.ColumnNDE(FC.handle_cfg(32), 1, conv=3) as conv:
        refused(conv._h, "single-model handle")
    wm = PC.sample(PC.SEQ_CASE).cfg
    with ColumnNDEEnsemble(wm, 1, 2) as wme:
        refused(wme._h, "wind-mixing")
    with ClosureColumns(wm, 1, 1) as clo:
        refused(clo._h, "closure handle")
