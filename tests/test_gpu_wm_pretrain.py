"""`wm_pretrain_ens_kernel` (csrc/engine_wm_pretrain.hip, `colnde_ensemble_pretrain_wm_flux_dev`): `train_NN` for the K x 3 flux networks of a wind-mixing
ensemble in one launch, model k's nets fitted under model k's closure constants.  Blocks against the single handle's bits (A), independence of the chains
(B), a grid larger than the machine (C), the gradient read out of the ADAM moments (D), the sequence semantics of a pass (E), the driver's loop (F) and the
refusals (G).  One column, the helper's config of at most 8 frames, at most 8 samples, Nz = 32, 96-50-20-31 nets throughout.

Tolerances: 10x what float32 alone costs for this arithmetic under each model's constants, measured WITHOUT the kernel by the float32 restatement of
tests/pretrain_cases.py, largest over the cases each constant judges (tests/test_wm_pretrain_host.py holds every constant between 10x and 12x its
measurement).  Beside each: the restatement's largest error / the kernel's largest error on an MI355X."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde.flux_compat import ADAM
from colnde.wind_mixing import train_NN, train_NN_ensemble
from tests import pretrain_cases as PC
from tests import wm_pretrain_cases as WC

pytestmark = pytest.mark.gpu

#                          float32 restatement (CPU)   kernel (MI355X)
TOL_LOSS = 1.1e-6        # 1.10e-7   3.00e-7   single-sample losses, the mean of a pass's pre-update losses
TOL_W = 4.1e-6           # 4.06e-7   5.75e-7   gradient, weight blocks
TOL_B = 3.9e-6           # 3.83e-7   4.79e-7   gradient, bias blocks
TOL_M = 6.2e-6           # 6.13e-7   3.75e-7   one pass of ADAM over eight visits, largest over the blocks and the nine chains
TOL_V = 9.1e-6           # 9.00e-7   4.59e-7
TOL_THETA = 1.1e-6       # 1.09e-7   1.08e-7   relative to |theta|
TOL_MOVED = 6.0e-5       # 5.93e-6   5.96e-6   relative to the distance the pass moved the block
TOL_DRV_THETA = 2.5e-6   # 2.44e-7   2.45e-7   the driver: 2 + 2 epochs over 8 samples
TOL_DRV_HIST = 3.0e-6    # 2.92e-7   5.88e-7   ... its training-set losses
# exact bounds: bit equality, and one ulp for v (D)

F32_TINY = float(np.finfo(np.float32).tiny)
SENTINEL = 7.0      # in the moments of the nets not trained: whatever touches them shows
NAME = "colnde_ensemble_pretrain_wm_flux_dev"


def _t(a, dt=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(torch.device("cuda", 0))


def _np(t):
    return t.detach().cpu().numpy()


def _ens(s, K=None, physics="own"):
    return colnde.ColumnNDEEnsemble(s.cfg, 1, s.K if K is None else K, physics=WC.physics_of(s.cond) if isinstance(physics, str) else physics)


def _dev(s):
    return _t(s.X), _t(s.B), _t(s.Y)


def _run(ens, s, W, etas, orders=None, nets=7, m=None, v=None, beta=(0.9, 0.999), beta_t=None, update=True, gs=WC.GS, dev=None):
    """One call; (theta, m, v, beta_t, losses [K, 3]) as numpy afterwards."""
    X, B, Y = dev if dev is not None else _dev(s)
    theta = _t(W)
    m, v = _t(np.zeros_like(W) if m is None else m), _t(np.zeros_like(W) if v is None else v)
    bt = list(beta_t) if beta_t is not None else [beta[0], beta[1]]
    loss = ens.pretrain_fluxes(theta, m, v, X, B, Y, None if orders is None else _t(orders, np.int32), gs, None if etas is None else _t(etas), nets, beta, 1e-8, bt,
                               update=update)
    assert loss.shape == (W.shape[0], 3) and loss.dtype == np.float32
    return _np(theta), _np(m), _np(v), bt, loss


def _single(eng, s, j, w, order, eta, update=True, gs=WC.GS, dev=None):
    """`colnde_pretrain_flux_dev` on the single handle `eng` (its config carries the model's constants) for one model's weights, flux_type = j, from zero
    moments: (theta, m, v, beta_t, loss) — full vectors, of which only net j's block may have changed."""
    X, B, Y = dev if dev is not None else _dev(s)
    theta, m, v = _t(w), _t(np.zeros_like(w)), _t(np.zeros_like(w))
    opt = ADAM(float(eta))
    loss = eng.pretrain_flux(j, theta, m, v, X, B, Y[j], None if order is None else _t(order, np.int32), gs, opt, update=update)
    return _np(theta), _np(m), _np(v), list(opt.beta_t), np.float32(loss)


def _net(cfg, j):
    return slice(j * cfg.net_size, (j + 1) * cfg.net_size)


def _assert_block_is_the_single_handles(s, got, k, j, ref):
    theta, m, v, bt, loss = got
    sl = _net(s.cfg, j)
    for a, r in ((theta, ref[0]), (m, ref[1]), (v, ref[2])):
        np.testing.assert_array_equal(a[k][sl], r[sl], err_msg="model %d net %d" % (k, j))
    assert loss[k, j] == ref[4] and bt == ref[3], (k, j, loss[k, j], ref[4], bt, ref[3])


def _model_handle(s, k, physics="own"):
    ph = WC.physics_of(s.cond) if isinstance(physics, str) else physics
    return colnde.ColumnNDE(s.cfg if ph is None else WC.model_cfg(s.cfg, ph[k]), 1)


# ---- A: bits ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", WC.MPP_CONDS + WC.PLAIN_CONDS)
def test_blocks_hold_the_bits_of_the_single_handle(cond):
    """K = 3, all three nets in one launch over the per-chain orders, gradient_scaling = 1e-2, per-chain rates: block (k, j) of theta, m, v, the loss and
    beta_t are those of `colnde_pretrain_flux_dev` on a single handle whose config carries model k's constants, flux_type = j; the same with order = None
    and with update=False.  (conv_adj_branch, raw: the closure is off, physics = None.)"""
    s = WC.samples(cond, WC.N)
    with _ens(s) as ens:
        dev = _dev(s)
        got = _run(ens, s, s.W, WC.ETAS, WC.ORDERS, dev=dev)
        got_none = _run(ens, s, s.W, WC.ETAS, None, dev=dev)
        ev = _run(ens, s, s.W, None, WC.ORDERS, beta_t=[0.81, 0.998001], update=False, dev=dev)
    for k in range(3):
        with _model_handle(s, k) as eng:
            for j in range(3):
                _assert_block_is_the_single_handles(s, got, k, j, _single(eng, s, j, s.W[k], WC.ORDERS[k, j], WC.ETAS[k, j], dev=dev))
                _assert_block_is_the_single_handles(s, got_none, k, j, _single(eng, s, j, s.W[k], None, WC.ETAS[k, j], dev=dev))
                ref = _single(eng, s, j, s.W[k], WC.ORDERS[k, j], WC.ETAS[k, j], update=False, dev=dev)
                assert ev[4][k, j] == ref[4], (k, j)
                assert not np.array_equal(got[0][k][_net(s.cfg, j)], s.W[k][_net(s.cfg, j)])                # the pass moved the weights
    np.testing.assert_array_equal(ev[0], s.W)                                                               # update=False: nothing written
    assert not ev[1].any() and not ev[2].any() and ev[3] == [0.81, 0.998001]
    if cond in WC.MPP_CONDS:
        assert len({float(x) for x in ev[4][:, 2]}) == 3                                                    # (three models, three different fits)


# ---- B: independence --------------------------------------------------------------------------------------------------------------------------------------
def test_changing_one_model_leaves_the_others_bits():
    s = WC.samples("mpp_zero_weights", WC.N)
    with _ens(s) as ens:
        dev = _dev(s)
        base = _run(ens, s, s.W, WC.ETAS, WC.ORDERS, dev=dev)
        for what in ("weights", "rate", "order", "constants"):
            W, e, o = s.W.copy(), WC.ETAS.copy(), WC.ORDERS.copy()
            if what == "weights":
                W[1] = W[1] * np.float32(1.01)
            elif what == "rate":
                e[1] = 3e-3
            elif what == "order":
                o[1] = o[1][:, ::-1]
            else:
                ph = WC.PHYSICS.copy()
                ph[1] = WC.PHYSICS_ALT
                ens.set_physics(ph)
            got = _run(ens, s, W, e, o, dev=dev)
            for k in (0, 2):
                for a, b in zip(got[:3], base[:3]):
                    np.testing.assert_array_equal(a[k], b[k], err_msg=what)
                assert (got[4][k] == base[4][k]).all(), what
            for j in range(3):
                assert not np.array_equal(got[0][1][_net(s.cfg, j)], base[0][1][_net(s.cfg, j)]), (what, j)
            assert got[3] == base[3]
        # after set_physics row 1 holds the bits of a single handle with the NEW constants: no stale device copy
        with _model_handle(s, 1, physics=ph) as eng:
            for j in range(3):
                _assert_block_is_the_single_handles(s, got, 1, j, _single(eng, s, j, s.W[1], WC.ORDERS[1, j], WC.ETAS[1, j], dev=dev))


def test_a_net_mask_leaves_the_other_nets_blocks_alone():
    """nets = 0b100 with the uw and vw blocks of the moments pre-filled with 7.0: those blocks of theta, m, v keep their bits, their losses are 0, and
    the wT block is the three-net launch's."""
    s = WC.samples("mpp_zero_weights", WC.N)
    sl = _net(s.cfg, 2)
    mom = np.full_like(s.W, SENTINEL)
    mom[:, sl] = 0.0
    with _ens(s) as ens:
        dev = _dev(s)
        base = _run(ens, s, s.W, WC.ETAS, WC.ORDERS, dev=dev)
        got = _run(ens, s, s.W, WC.ETAS, WC.ORDERS, nets=0b100, m=mom, v=mom, dev=dev)
        named = _run(ens, s, s.W, WC.ETAS, WC.ORDERS, nets=("wT",), m=mom, v=mom, dev=dev)
    theta, m, v, bt, loss = got
    np.testing.assert_array_equal(theta[:, :sl.start], s.W[:, :sl.start])
    assert (m[:, :sl.start] == SENTINEL).all() and (v[:, :sl.start] == SENTINEL).all()
    assert not loss[:, :2].any() and (loss[:, 2] == base[4][:, 2]).all() and bt == base[3]
    for a, b in zip(got[:3], base[:3]):
        np.testing.assert_array_equal(a[:, sl], b[:, sl])
    for a, b in zip(got[:3], named[:3]):
        np.testing.assert_array_equal(a, b)


# ---- C: a grid larger than the machine --------------------------------------------------------------------------------------------------------------------
def test_more_chains_than_compute_units():
    """K = 90: 270 workgroups on 256 CUs, 3 samples: the first, a middle and the last model hold the single handle's bits in all three nets."""
    K = 90
    s = WC.samples("mpp_zero_weights", 3)
    rng = np.random.default_rng(7)
    W = (s.W[0][None, :] * (1.0 + 0.05 * rng.standard_normal((K, 1)))).astype(np.float32)
    ph = WC.PHYSICS[np.arange(K) % 3]
    etas = np.full((K, 3), 1e-3, np.float32)
    with _ens(s, K, ph) as ens:
        dev = _dev(s)
        got = _run(ens, s, W, etas, dev=dev)
    for k in (0, 45, 89):
        with _model_handle(s, k, physics=ph) as eng:
            for j in range(3):
                _assert_block_is_the_single_handles(s, got, k, j, _single(eng, s, j, W[k], None, 1e-3, dev=dev))
    assert not np.array_equal(got[0][0], got[0][89])


# ---- D: the gradient through the moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", WC.MPP_CONDS)
def test_single_sample_loss_and_gradient(cond):
    """One sample, zero moments, beta1 = beta2 = 0.5, beta_t = (0.5, 0.5), eta = 0: m = g / 2 exactly, so g = 2 m; v = fl(g g) / 2 ties v to the same g
    within one ulp; theta keeps its bits.  Loss and per-block gradient against float64 for each (model, net) under its own constants."""
    s, ref = WC.grad_reference(cond)
    with _ens(s) as ens:
        theta, m, v, bt, loss = _run(ens, s, s.W, np.zeros((3, 3), np.float32), None, beta=(0.5, 0.5), beta_t=[0.5, 0.5])
    np.testing.assert_array_equal(theta, s.W)
    assert bt == [0.25, 0.25]
    for k, j, c in WC.chains(s):
        g = (np.float32(2) * m[k][c.net]).astype(np.float32)
        e_loss, e_W, e_b, errs = WC.grad_errors(c, float(loss[k, j]), g, ref[k, j])
        v_ref = g * g / np.float32(2)
        ulps = float((np.abs(v[k][c.net].astype(np.float64) - v_ref) / np.maximum(np.spacing(v_ref), F32_TINY)).max())
        print("%s: loss %.6e rel err %.2e; gradient blocks %s; v off by %.2f ulp at most" %
              (c.case, loss[k, j], e_loss, " ".join("%s %.2e" % kv for kv in errs.items()), ulps))
        assert np.isfinite(g).all() and ulps <= 1.0
        assert e_loss < TOL_LOSS
        assert e_W < TOL_W, errs
        assert e_b < TOL_B, errs


# ---- E: sequence semantics --------------------------------------------------------------------------------------------------------------------------------
def test_adam_pass_follows_the_sequential_loop():
    """One ADAM pass of the nine chains over their own orders (with repeats) at their own rates against the float64 sequential loop under each model's
    constants: theta per block and per distance moved, m, v, and the mean of the pre-update losses."""
    s, ref = WC.sequence_reference()
    with _ens(s) as ens:
        theta, m, v, bt, loss = _run(ens, s, s.W, WC.ETAS, WC.ORDERS)
    for k, j, c in WC.chains(s):
        np.testing.assert_allclose(bt, ref[k, j][3], rtol=1e-15)
        e = WC.pass_errors(c, theta[k][c.net], m[k][c.net], v[k][c.net], loss[k, j], ref[k, j])
        print("%s: %s" % (c.case, " ".join("%s %.2e" % kv for kv in e.items())))
        assert e["moved_least"] > 1e-3                       # every block moved
        assert e["loss"] < TOL_LOSS                          # the mean of each sample's loss just before its own update
        assert e["theta"] < TOL_THETA and e["moved"] < TOL_MOVED, e
        assert e["m"] < TOL_M and e["v"] < TOL_V, e


# ---- F: the driver ----------------------------------------------------------------------------------------------------------------------------------------
def test_driver_follows_the_float64_loop_and_train_NN():
    """`train_NN_ensemble`, K = 2, two ADAMs x 2 epochs over 8 samples, against the float64 loop on the same permutations; model 1 against
    `wind_mixing.train_NN` on a single handle with model 1's constants, net by net and pass by pass, bit for bit; the training-set loss ends below where
    it started."""
    s, th_ref, hist_ref = WC.driver_reference()
    opts = lambda: [ADAM(r) for r in WC.DRV_RATES]
    seen = []
    with _ens(s, WC.DRV_K, WC.PHYSICS[:WC.DRV_K]) as ens:
        theta, hist = train_NN_ensemble(ens, s.W, s.X, s.B, s.Y, opts(), WC.DRV_EPOCHS, gradient_scaling=WC.DRV_GS, seeds=WC.DRV_SEEDS,
                                        cb=lambda total, th: seen.append(total.copy()))
    assert theta.shape == s.W.shape and theta.dtype == np.float32 and hist.shape == (4, WC.DRV_K, 3) and len(seen) == 4
    np.testing.assert_array_equal(np.stack(seen), hist)
    e_hist = np.abs(hist - hist_ref) / hist_ref
    e_th = [max(PC.block_errors(s.cfg, theta[k, _net(s.cfg, j)], th_ref[k, _net(s.cfg, j)]).values()) for k in range(WC.DRV_K) for j in range(3)]
    print("driver: theta %s, history rel err at most %.2e; losses %s" % (" ".join("%.2e" % e for e in e_th), e_hist.max(), hist.tolist()))
    assert (hist[-1] < hist[0]).all()
    assert max(e_th) < TOL_DRV_THETA and e_hist.max() < TOL_DRV_HIST
    # model 1, net by net: one train_NN call per pass with that pass's order, the optimiser object carrying moments and running powers across its epochs
    k, orders = 1, WC.driver_orders()
    w = s.W[k].copy()
    with colnde.ColumnNDE(WC.model_cfg(s.cfg, WC.PHYSICS[k]), 1) as eng:
        for j, nm in enumerate(WC.NETS):
            p = 0
            for opt, n_ep in zip(opts(), WC.DRV_EPOCHS):
                for _ in range(n_ep):
                    w, h = train_NN(eng, nm, w, s.X, s.B, s.Y[j], [opt], [1], gradient_scaling=WC.DRV_GS, order=orders[p, k, j])
                    assert np.float32(h[0]) == hist[p, k, j], (nm, p)
                    p += 1
    np.testing.assert_array_equal(w, theta[k])


# ---- G: refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call_and_leave_the_handle_usable():
    from colnde.nde import ClosureColumns, FreeConvectionEnsemble
    from oracle import nde_oracle as O
    from tests import fc_pretrain_cases as FC
    L = colnde._lib.lib()
    s = WC.samples("mpp_zero_weights", 1)
    p = PC.problem("mpp_zero_weights-uw", 2)[0]
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    theta, m, v, X, B, Y, eta = _t(s.W), _t(np.zeros_like(s.W)), _t(np.zeros_like(s.W)), _t(s.X), _t(s.B), _t(s.Y), _t(WC.ETAS)
    loss = (ctypes.c_float * 9)()

    def call(h, th=theta, mm=m, vv=v, x=X, n=1, nets=7, bt=(0.9, 0.999), update=1, lo=loss, et=eta):
        P = lambda a: a.data_ptr() if a is not None else None
        bt = (ctypes.c_double * 2)(*bt) if bt is not None else None
        rc = getattr(L, NAME)(h, nets, P(th), P(mm), P(vv), P(x), P(B), P(Y), None, n, 1e-2, P(et), 0.9, 0.999, 1e-8, bt, update, lo)
        return rc, L.colnde_last_error().decode()

    def refused(h, what, **kw):
        rc, msg = call(h, **kw)
        assert rc != 0 and NAME in msg and what in msg, (what, msg)

    with _ens(s) as ens:
        ens.set_problem(p.x0, p.bcs, truth)
        refused(None, "null handle")
        refused(ens._h, "null pointer", th=None)
        refused(ens._h, "null pointer", x=None)
        refused(ens._h, "null pointer", bt=None)
        refused(ens._h, "null pointer", lo=None)
        for nets in (0, 8, -1):
            refused(ens._h, "nets = %d" % nets, nets=nets)
        refused(ens._h, "moments", mm=None)
        refused(ens._h, "moments", vv=None)
        refused(ens._h, "rates", et=None)
        for bt in ((1.0, 0.5), (0.5, 1.0), (float("nan"), 0.5)):
            refused(ens._h, "beta", bt=bt)
        for n in (0, -3):
            refused(ens._h, "n_samples", n=n)
        assert call(ens._h, mm=None, vv=None, et=None, update=0)[0] == 0                      # an evaluation needs neither moments nor rates
        with pytest.raises(ValueError, match="moments"):                                     # ... and the wrapper's own checks
            ens.pretrain_fluxes(_t(s.W), None, None, X, B, Y, None, 1e-2, eta)
        with pytest.raises(ValueError, match="nets"):
            ens.pretrain_fluxes(_t(s.W), m, v, X, B, Y, None, 1e-2, eta, nets=("uw", "wt"))
        with pytest.raises(ValueError, match="nets"):
            ens.pretrain_fluxes(_t(s.W), m, v, X, B, Y, None, 1e-2, eta, nets=0)
        with pytest.raises(ValueError, match="order"):
            ens.pretrain_fluxes(_t(s.W), m, v, X, B, Y, _t(np.full((3, 3, 1), 1, np.int32), np.int32), 1e-2, eta)
        with pytest.raises(ValueError, match="order"):
            ens.pretrain_fluxes(_t(s.W), m, v, X, B, Y, _t(np.zeros((3, 1), np.int32), np.int32), 1e-2, eta)
        # the two older calls still refuse this handle, with their own messages
        z, f, bt = ctypes.c_void_p(), ctypes.c_float(), (ctypes.c_double * 2)(0.9, 0.999)
        assert L.colnde_pretrain_flux_dev(ens._h, 2, z, z, z, z, z, z, z, 1, 0.0, 1e-3, 0.9, 0.999, 1e-8, bt, 0, ctypes.byref(f)) != 0
        msg = L.colnde_last_error().decode()
        assert "colnde_pretrain_flux_dev" in msg and "ensemble of 3 models" in msg
        assert L.colnde_ensemble_pretrain_flux_dev(ens._h, z, z, z, z, z, z, z, 1, z, 0, z, 0.9, 0.999, 1e-8, bt, 0, ctypes.byref(f)) != 0
        msg = L.colnde_last_error().decode()
        assert "colnde_ensemble_pretrain_flux_dev" in msg and "wind-mixing" in msg
        np.testing.assert_array_equal(_np(theta), s.W)                                       # nothing was written by a refused call
        assert not _np(m).any() and not _np(v).any()
        assert np.isfinite(ens.loss(s.W, [1, 1, 1, 0, 0, 0])).all()                          # the handle is still good
    with colnde.ColumnNDE(s.cfg, 1) as single:
        refused(single._h, "single-model handle")
    with FreeConvectionEnsemble(FC.handle_cfg(32), 1, 2) as fce:
        refused(fce._h, "colnde_ensemble_pretrain_flux_dev")
    with FreeConvectionEnsemble(FC.handle_cfg(32), 1, 2, conv=3) as fcc:
        refused(fcc._h, "free-convection")
    with colnde.ColumnNDE(FC.handle_cfg(32), 1, conv=3) as conv:
        refused(conv._h, "single-model handle")
    with ClosureColumns(s.cfg, 1, 1) as clo:
        refused(clo._h, "closure handle")
