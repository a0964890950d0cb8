"""The ensemble's error estimate member by member, and the step schedule chosen for all K (colnde_ensemble_error_estimate[_dev],
colnde_ensemble_choose_schedule; ColumnNDEEnsemble.ensemble_error_estimate / .choose_ensemble_schedule).

The reference for the estimate is tests/schedule_common.estimate_norm — the NumPy restatement of the integrator's norm — on the two solutions the
estimate compares, fetched with `forward` from twin ensembles at S and 2 S; the bound, 1e-3 relative per (member, save point), is the one
tests/test_gpu_schedule.py holds colnde_choose_schedule's estimate to.  The reference for the choice is tests/ens_schedule_cases.greedy over estimates
restated the same way from twin ensembles under `set_schedule`.  Shapes: 1, 3 and 17 columns (less than one 16-lane column group's walk, one
partial walk, two walks), K = 1, 3 and 70, 2 and 7 save points; rows of 96 (wind mixing) and 32 (free convection) floats."""
import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde._arrays import _ptr
from colnde.nde import ENGINE_TILE16
from colnde.wind_mixing import WindMixingNDE, train_NDE_ensemble
from oracle import nde_oracle as O
from tests import conv_cases
from tests import ens_schedule_cases as E
from tests import schedule_common as C
from tests import stream_cases as SC_
from tests.test_gpu_ensemble import PHYS, _model_cfg, _weights

pytestmark = pytest.mark.gpu

SC = C.SC
RK4, RKC2, SWITCH = 16.0 / 15.0, 4.0 / 3.0, 2.0              # richardson_factor: smooth RK4, smooth RKC2, a switching right-hand side
# three members of one stiffness (nu0, nu_minus and Pr shared: the same RKC2 stage count at every step, as a single handle picks for itself) that differ
# in the closure's other constants
PHYS_SAME_LAMBDA = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [1e-4, 0.1, 0.8, 0.2, 1.0], [1e-4, 0.1, 1.3, 0.3, 1.0]], np.float32)


def _wm(n_col, n_save=4, **kw):
    """a wind-mixing problem on 2 or 4 evenly spaced save points (substeps = 2), or on the uneven axis of 7 (substeps = 16: its longest interval needs 13)"""
    if n_save == 7:
        return C.with_axis(C.base_problem(n_col, **kw), C.UNEVEN, substeps=16)
    return C.base_problem(n_col, n_frames=n_save, **kw)


def _phys(K):
    return PHYS[np.arange(K) % len(PHYS)]


def _rel(got, ref):
    """the largest relative distance per (member, save point); where the reference is 0 the estimate must be 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(got[ref == 0], ref[ref == 0])
    nz = ref != 0
    return float((np.abs(got - ref)[nz] / ref[nz]).max()) if nz.any() else 0.0


def _restated(a, b, factor, floor=1e-3):
    """[K, n_save] from two solutions [K, n_col, n_save, row]"""
    return C.estimate_norm(a, b, factor, floor).max(axis=1)


# ---- 1. the kernel, through the estimate call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_save", [2, 7])
@pytest.mark.parametrize("K", [1, 3, 70])
@pytest.mark.parametrize("n_col", [1, 3, 17])
def test_estimate_is_the_norm_of_the_two_solutions(n_col, K, n_save):
    p = _wm(n_col, n_save)
    W, ph = _weights(p.cfg, K), _phys(K)
    with colnde.ColumnNDEEnsemble(p.cfg, n_col, K, physics=ph) as e, colnde.ColumnNDEEnsemble(p.cfg.with_(substeps=2 * p.cfg.substeps), n_col, K, physics=ph) as twin:
        for x in (e, twin):
            x.set_problem(p.x0, p.bcs, None)
        a, b = e.forward(W), twin.forward(W)
        est = e.ensemble_error_estimate(W)
        again = e.ensemble_error_estimate(W)
    assert est.shape == (K, n_save) and est.dtype == np.float32
    ref = _restated(a, b, RK4)
    dist = _rel(est, ref)
    print("estimate against the NumPy norm, %d columns, K = %d, %d save points: %.3e relative (largest estimate %.3e)" % (n_col, K, n_save, dist, est.max()))
    assert np.all(est[:, 0] == 0) and np.isfinite(est).all() and est[:, 1:].min() > 0
    assert dist <= 1e-3
    assert np.array_equal(est, again)
    if K > 1:
        assert not np.array_equal(est[0], est[1])                       # (the members do differ)


def test_estimate_from_device_weights_and_under_a_schedule():
    """torch device weights go to the _dev form; under a schedule the estimate compares the schedule with every interval doubled"""
    import torch
    p = _wm(17, 7)
    W, ph, S = _weights(p.cfg, 3), PHYS[:3], (4, 2, 2, 2, 8, 16)
    with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=ph) as e, colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=ph) as twin:
        for x, s in ((e, S), (twin, tuple(2 * c for c in S))):
            x.set_schedule(s)
            x.set_problem(p.x0, p.bcs, None)
        host = e.ensemble_error_estimate(W)
        dev = e.ensemble_error_estimate(torch.from_numpy(W).cuda())
        ref = _restated(e.forward(W), twin.forward(W), RK4)
        assert e.schedule() == S
    assert isinstance(dev, np.ndarray) and np.array_equal(host, dev)
    assert _rel(host, ref) <= 1e-3


# ---- 2. row k is the single handle -----------------------------------------------------------------------------------------------------------------
def _rows_against_single_handles(ens, singles, W, what):
    est = ens.ensemble_error_estimate(W)
    for k, h in enumerate(singles):
        one = h.error_estimate(W[k])
        print("%s: member %d estimate %.4e, single handle %.4e" % (what, k, est[k].max(), one))
        assert one > 0 and abs(est[k].max() - one) <= 1e-3 * one, (what, k, est[k].max(), one)
    return est


@pytest.mark.parametrize("stepper", ["rk4", "rkc2"])
def test_net_split_rows_are_the_single_handles_estimates(stepper):
    p = _wm(17, stepper=stepper)
    W, ph = _weights(p.cfg, 3), PHYS_SAME_LAMBDA if stepper == "rkc2" else PHYS[:3]
    singles = [colnde.ColumnNDE(_model_cfg(p.cfg, ph[k]), 17) for k in range(3)]
    try:
        with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=ph) as e:
            for x in singles + [e]:
                x.set_problem(p.x0, p.bcs, None)
            assert ("stepper=rkc2" in e.describe()) == (stepper == "rkc2")
            est = _rows_against_single_handles(e, singles, W, "net-split %s" % stepper)
            assert len({float(v) for v in est.max(axis=1)}) == 3
    finally:
        for h in singles:
            h.close()


def test_tile_ensemble_rows_are_the_single_handles_estimates():
    p = synthetic.wind_mixing_problem(17, n_frames=4, weight_divisor=1e2, layer_sizes=(96, 24, 31), activations=("tanh", "identity"))
    W, ph = _weights(p.cfg, 3), PHYS[:3]
    singles = [colnde.ColumnNDE(_model_cfg(p.cfg, ph[k]), 17, engine=ENGINE_TILE16) for k in range(3)]
    try:
        with colnde.TileNDEEnsemble(p.cfg, 17, 3, physics=ph) as e:
            for x in singles + [e]:
                x.set_problem(p.x0, p.bcs, None)
            assert "tile_ensemble=1" in e.describe()
            _rows_against_single_handles(e, singles, W, "tile ensemble 96-24-31 tanh")
    finally:
        for h in singles:
            h.close()


@pytest.mark.parametrize("kind", ["fc_rk4", "ca_rk4", "ca_rkc2"])
def test_free_convection_rows_are_the_single_handles_estimates(kind):
    """FreeConvectionNDE under RK4, ConvectiveAdjustmentNDE under RK4 and RKC2, Nz = 32 (rows of 32 floats; the floor is 1e-6 / cfg.reltol)"""
    n = 9
    if kind == "fc_rk4":
        cfg = (p := synthetic.free_convection_problem(n, Nz=32, n_save=5, substeps=2, t_end=0.01)).cfg
    elif kind == "ca_rk4":
        cfg = (p := synthetic.free_convection_problem(n, Nz=32, n_save=5, substeps=20, convective_adjustment=True, t_end=0.01)).cfg
    else:
        cfg = (p := synthetic.free_convection_problem(n, Nz=32, n_save=9, substeps=2, convective_adjustment=True, t_end=0.06)).cfg.with_(stepper="rkc2")
    x0 = p.x0.copy()
    if kind != "fc_rk4":
        x0[:2, 16:22] = x0[:2, 16:22][:, ::-1]                           # an inverted layer in two columns: the adjustment switches
    W = _weights(cfg, 3)
    singles = [colnde.ColumnNDE(cfg, n) for _ in range(3)]
    try:
        with colnde.FreeConvectionEnsemble(cfg, n, 3) as e, colnde.FreeConvectionEnsemble(cfg.with_(substeps=2 * cfg.substeps), n, 3) as twin:
            for x in singles + [e, twin]:
                x.set_problem(x0, p.bcs, None)
            est = _rows_against_single_handles(e, singles, W, kind)
            ref = _restated(e.forward(W), twin.forward(W), RK4 if kind == "fc_rk4" else SWITCH, 1e-6 / cfg.reltol)
            assert _rel(est, ref) <= 1e-3
    finally:
        for h in singles:
            h.close()


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["nan", "large"])
def test_a_member_that_leaves_the_stable_regime_has_inf_in_its_own_row(how):
    p = _wm(17, 7)
    K, j = 5, 3
    W, ph = _weights(p.cfg, K), _phys(K)
    bad = W.copy()
    if how == "nan":
        bad[j, 7] = np.nan
    else:
        bad[j] *= 1e6                                                    # forcings of 1e18 and more: the solve overflows within a few steps
    with colnde.ColumnNDEEnsemble(p.cfg, 17, K, physics=ph) as e:
        e.set_problem(p.x0, p.bcs, None)
        base = e.ensemble_error_estimate(W)
        got = e.ensemble_error_estimate(bad)
        assert np.array_equal(e.ensemble_error_estimate(W), base)       # and the handle is none the worse
    assert got[j, 0] == 0 and np.all(got[j, 1:] == np.inf), got[j]
    others = [k for k in range(K) if k != j]
    assert np.isfinite(got[others]).all() and np.array_equal(got[others], base[others])


# ---- 4. the handle is untouched ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [None, (4, 2, 2, 2, 8, 16)])
def test_the_handle_computes_what_it_computed_before(schedule):
    p = _wm(17, 7)
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    W = _weights(p.cfg, 3)
    with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=PHYS[:3]) as e:
        if schedule is not None:
            e.set_schedule(schedule)
        e.set_problem(p.x0, p.bcs, truth)
        counts, steps, line = e.schedule(), e.n_steps, e.describe()
        g0, f0 = e.loss_grad(W, SC), e.forward(W)
        est = e.ensemble_error_estimate(W)
        assert e.schedule() == counts and e.n_steps == steps and e.substeps == p.cfg.substeps and e.describe() == line
        assert np.array_equal(e.loss_grad(W, SC), g0) and np.array_equal(e.forward(W), f0)
        with pytest.raises(colnde.ColndeError):                          # a failing call (NULL weights reach the library as a null pointer) leaves it alone too
            _lib.check(e._L.colnde_ensemble_error_estimate(e._h, None, _ptr(est)))
        assert e.schedule() == counts and np.array_equal(e.loss_grad(W, SC), g0)
    assert np.isfinite(est).all() and est.max() > 0


def test_rkc2_solves_after_an_estimate_have_a_fresh_handles_bits():
    """the doubled solve runs another stage table (rkc_stages = 0: the count follows the step); afterwards the table in force is the one of creation"""
    p = _wm(17, stepper="rkc2")
    truth = O.solve(p.cfg.with_(stepper="rk4"), p.x0, p.bcs, p.weights_truth).astype(np.float32)
    W = _weights(p.cfg, 3)
    with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=PHYS[:3]) as fresh:
        fresh.set_problem(p.x0, p.bcs, truth)
        want = fresh.forward(W), fresh.loss_grad(W, SC)
    with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=PHYS[:3]) as e:
        e.set_problem(p.x0, p.bcs, truth)
        line = e.describe()
        est = e.ensemble_error_estimate(W)
        assert e.describe() == line
        assert np.array_equal(e.forward(W), want[0]) and np.array_equal(e.loss_grad(W, SC), want[1])
    assert np.isfinite(est).all() and est[:, 1:].min() > 0


# ---- 5. the choice -----------------------------------------------------------------------------------------------------------------------------------
def _twin_estimates(p, W, physics):
    """estimates_at for ens_schedule_cases.greedy: twin ensembles under set_schedule(S) and set_schedule(2 S), their solutions through the NumPy norm"""
    def estimates_at(S):
        with colnde.ColumnNDEEnsemble(p.cfg, p.n_columns, W.shape[0], physics=physics) as a, colnde.ColumnNDEEnsemble(p.cfg, p.n_columns, W.shape[0], physics=physics) as b:
            for x, s in ((a, S), (b, tuple(2 * c for c in S))):
                x.set_schedule(s)
                x.set_problem(p.x0, p.bcs, None)
            return _restated(a.forward(W), b.forward(W), RK4)
    return estimates_at


def test_the_chosen_schedule_is_the_greedy_run_over_the_members_maximum():
    p, W = E.problem_k3()
    truth = O.solve(p.cfg.with_(substeps=16), p.x0, p.bcs, p.weights_truth).astype(np.float32)
    cfg = p.cfg.with_(substeps=16)                                       # (one count on this axis needs 16: the ensemble is created stable)
    p = synthetic.ColumnProblem(cfg, p.x0, p.bcs, p.weights, p.weights_truth)
    minima = np.max([colnde.schedule_min(c) for c in E.member_cfgs(cfg, E.PHYS_K3)], axis=0)
    start = tuple(C.pow2_ceil(int(v)) for v in minima)
    verdict, S_twin, est_twin, rounds = E.greedy(_twin_estimates(p, W, E.PHYS_K3), start, E.RELTOL)
    for r in rounds:
        print("twin round: S = %r, est = %.4e, |est - reltol| / reltol = %.3f, nearest addition to dmax / 2: %.3f" % r)
    assert E.clear_of_thresholds(rounds), rounds                         # (if not, the inputs are wrong: tests/ens_schedule_cases.py)
    assert verdict == E.MET
    with colnde.ColumnNDEEnsemble(cfg, E.N_COL, 3, physics=E.PHYS_K3) as e:
        e.set_problem(p.x0, p.bcs, truth)
        before = e.loss_grad(W, SC)                                      # the tapes are planned: an ensemble's are planned again
        counts, est = e.choose_ensemble_schedule(W, E.RELTOL)
        print("chosen %r (float64: %r), member estimates %r (twin: %r)" % (counts, E.SCHEDULE_F64, est.tolist(), est_twin.tolist()))
        assert counts == S_twin
        assert counts == E.SCHEDULE_F64                                  # every round of both runs is clear of the thresholds: float32 decides as float64
        for c, m in zip(counts, start):
            assert c >= m and c % m == 0 and (c // m) & (c // m - 1) == 0, (counts, start)
        assert est.shape == (3,) and est.max() <= E.RELTOL and _rel(est, est_twin) <= 1e-3
        assert e.schedule() == counts and e.n_steps == sum(counts)
        assert "schedule=%d/%d intervals" % (sum(counts), len(counts)) in e.describe()
        after = e.loss_grad(W, SC)
        assert not np.array_equal(after, before)
        assert _rel(e.ensemble_error_estimate(W).max(axis=1), est) <= 1e-6    # the estimate under the kept schedule: the same two solves
    with colnde.ColumnNDEEnsemble(cfg, E.N_COL, 3, physics=E.PHYS_K3) as fresh:
        fresh.set_schedule(counts)
        fresh.set_problem(p.x0, p.bcs, truth)
        assert np.array_equal(fresh.loss_grad(W, SC), after)
    # one count for all: the largest any member needs on a single twin
    U = 0
    for k in range(3):
        with colnde.ColumnNDE(_model_cfg(cfg, E.PHYS_K3[k]), E.N_COL) as h:
            h.set_problem(p.x0, p.bcs, None)
            U = max(U, h.choose_substeps(W[k], E.RELTOL)[0])
    print("sum(counts) = %d against 6 x U = %d" % (sum(counts), 6 * U))
    assert sum(counts) < 6 * U


def test_three_identical_members_choose_the_single_handles_schedule():
    p, W = E.problem_k3()
    cfg = _model_cfg(p.cfg.with_(substeps=16), E.PHYS_K3[0])
    W3, ph3 = np.stack([W[0]] * 3), np.stack([E.PHYS_K3[0]] * 3)
    with colnde.ColumnNDE(cfg, E.N_COL) as h, colnde.ColumnNDEEnsemble(cfg, E.N_COL, 3, physics=ph3) as e:
        for x in (h, e):
            x.set_problem(p.x0, p.bcs, None)
        S, est1 = h.choose_schedule(W[0], E.RELTOL)
        counts, est = e.choose_ensemble_schedule(W3, E.RELTOL)
    assert counts == S
    assert est[0] == est[1] == est[2] and abs(est[0] - est1) <= 1e-3 * est1


# ---- 6. refusals, each by its message ----------------------------------------------------------------------------------------------------------------
def _estimate_refused(h, W, match):
    est = np.zeros((max(1, getattr(h, "n_models", 1)), h.cfg.n_save), np.float32)
    w = np.ascontiguousarray(W, np.float32)
    with pytest.raises(colnde.ColndeError, match=match):
        _lib.check(h._L.colnde_ensemble_error_estimate(h._h, _ptr(w), _ptr(est)))
    with pytest.raises(colnde.ColndeError, match="colnde_ensemble_error_estimate"):
        _lib.check(h._L.colnde_ensemble_error_estimate(h._h, _ptr(w), _ptr(est)))


def _choice_refused(h, W, match):
    w = np.ascontiguousarray(W, np.float32)
    with pytest.raises(colnde.ColndeError, match=match):
        _lib.check(h._L.colnde_ensemble_choose_schedule(h._h, _ptr(w), 1e-3, None, None))


def test_refusals():
    p = _wm(3)
    W = _weights(p.cfg, 3)
    with colnde.ColumnNDE(p.cfg, 3) as h:
        h.set_problem(p.x0, p.bcs, None)
        _estimate_refused(h, W[0], "a single handle's estimate is colnde_error_estimate")
        _choice_refused(h, W[0], "colnde_ensemble_choose_schedule takes the handles of colnde_create_ensemble: a single handle's schedule is chosen by colnde_choose_schedule")
    with colnde.ClosureColumns(p.cfg, 3, 2) as h:
        _estimate_refused(h, np.zeros((2, 5), np.float32), "this is a closure handle")
        _choice_refused(h, np.zeros((2, 5), np.float32), "the closure engine")
    cv = synthetic.free_convection_conv_problem(8, 3, Nz=32, **conv_cases.FC_KW)
    with colnde.FreeConvectionEnsemble(cv.cfg, 8, 2, conv=3) as h:
        h.set_problem(cv.x0, cv.bcs, None)
        _estimate_refused(h, np.zeros((2, h.n_params), np.float32), "does not cover the convolutional first layer")
        _choice_refused(h, np.zeros((2, h.n_params), np.float32), "a conv handle")
    with colnde.ColumnNDEEnsemble(p.cfg, 3, 3, physics=PHYS[:3]) as e:
        _estimate_refused(e, W, "colnde_set_problem has not been called")
        _choice_refused(e, W, "colnde_ensemble_choose_schedule: colnde_set_problem has not been called")
        e.set_problem(p.x0, p.bcs, None)
        # a shard: both calls refuse a handle whose global column count differs from its own, in refuse_auto_on_a_shard's words — but no ensemble can be
        # made one: colnde_set_global_columns refuses every ensemble, and keeps doing so.  What can be held here is that the door stays shut.
        with pytest.raises(colnde.ColndeError, match="colnde_set_global_columns takes one weight vector, but this handle holds an ensemble of 3 models"):
            e.set_global_columns(6)
        assert e.ensemble_error_estimate(W).shape == (3, 4)
        # the calls the ensemble inherits keep refusing
        for call in (lambda: e.error_estimate(W[0]), lambda: e.choose_substeps(W[0], 1e-3), lambda: e.choose_schedule(W[0], 1e-3)):
            with pytest.raises(colnde.ColndeError, match="this handle holds an ensemble of 3 models"):
                call()
    with colnde.ColumnNDEEnsemble(p.cfg.with_(stepper="rkc2"), 3, 3, physics=PHYS[:3]) as e:
        e.set_problem(p.x0, p.bcs, None)
        _choice_refused(e, W, "RK4 only: the RKC2 stage table depends on dt")
    tp = synthetic.wind_mixing_problem(3, n_frames=4, weight_divisor=1e2, layer_sizes=(96, 24, 31), activations=("tanh", "identity"))
    with colnde.TileNDEEnsemble(tp.cfg, 3, 2, physics=PHYS[:2]) as e:
        e.set_problem(tp.x0, tp.bcs, None)
        _choice_refused(e, _weights(tp.cfg, 2), "colnde_ensemble_choose_schedule does not serve a tile ensemble")
    fc = synthetic.free_convection_problem(8, Nz=32, n_save=4)
    with colnde.FreeConvectionEnsemble(fc.cfg, 8, 2) as e:
        e.set_problem(fc.x0, fc.bcs, None)
        _choice_refused(e, _weights(fc.cfg, 2), "a free-convection ensemble")


# ---- 7. failures keep the previous schedule ---------------------------------------------------------------------------------------------------------
def test_failures_keep_the_previous_schedule():
    p, W = E.problem_k3()
    cfg = p.cfg.with_(substeps=16)
    truth = O.solve(cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    old = (4, 4, 4, 4, 16, 16)
    with colnde.ColumnNDEEnsemble(cfg, E.N_COL, 3, physics=E.PHYS_K3) as e:
        e.set_schedule(old)
        e.set_problem(p.x0, p.bcs, truth)
        g0 = e.loss_grad(W, SC)
        with pytest.raises(colnde.ColndeError, match=r"reltol = 1e-08 is below the float32 round-off floor of this solve: the estimate stopped falling at"):
            e.choose_ensemble_schedule(W, 1e-8)
        assert e.schedule() == old and np.array_equal(e.loss_grad(W, SC), g0)
        bad = W.copy()
        bad[1, 7] = np.nan
        with pytest.raises(colnde.ColndeError, match=r"the solve of member 1 is not finite under a schedule of 32 steps in all"):
            e.choose_ensemble_schedule(bad, E.RELTOL)
        assert e.schedule() == old and np.array_equal(e.loss_grad(W, SC), g0)
        with pytest.raises(colnde.ColndeError, match="reltol must be > 0"):
            e.choose_ensemble_schedule(W, -1.0)


# ---- 8. a side stream, and the training loop -----------------------------------------------------------------------------------------------------------
def test_estimate_on_a_side_stream_behind_late_weights():
    """tests/stream_cases.py's pattern: the problem and the weights arrive late, in stream order, on a non-blocking side stream; both solves, the kernel
    and the copy of the estimates are on the handle's stream, so the estimate is the null stream's, bit for bit.  (The call synchronises — it returns
    host numbers — so it is exempt from the harness's "has not waited" condition.)"""
    import torch
    from tests import reuse_cases as R
    kind = "wm_ens"
    S = SC_.side_streams()[0]
    late = SC_.Late(**SC_.problem_pairs(kind))

    def body(h, t, still):
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
        est = h.ensemble_error_estimate(t["w"])
        still("ensemble_error_estimate_dev")
        return est, h.forward(t["w"])

    got, ref = SC_.late_inputs(S, lambda: R.open_handle(kind), late, body, tag="ens_schedule/estimate", exempt=("ensemble_error_estimate_dev",))
    p = R.problem(kind, 1)
    with R.open_handle(kind) as h:
        R.set_problem(h, p)
        want = h.ensemble_error_estimate(p.w), h.forward(p.w)
    stale = SC_.Late(**SC_.problem_pairs(kind))
    with R.open_handle(kind) as h:
        h.set_problem(stale["x0"], stale["bcs"], stale["truth"])
        other = h.ensemble_error_estimate(stale["w"])
    torch.cuda.synchronize()
    R.same(ref, want, "null stream, device tensors")
    R.same(got, want, "side stream, late inputs")
    assert not np.array_equal(other, want[0])                             # (the stale inputs would have shown)


def test_training_with_a_chosen_schedule_is_training_with_the_counts():
    p, W = E.problem_k3()
    cfg = p.cfg.with_(substeps=16)
    truth = O.solve(cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    etas = np.array([3e-4, 1e-4, 5e-4], np.float32)
    wm = WindMixingNDE(cfg, p.x0, p.bcs, truth)
    try:
        chosen = train_NDE_ensemble(wm, W, E.PHYS_K3, etas, epochs=1, maxiters=3, schedule="choose", reltol=E.RELTOL)
        counts = chosen[0].schedule
        given = train_NDE_ensemble(wm, W, E.PHYS_K3, etas, epochs=1, maxiters=3, schedule=counts)
    finally:
        wm.close()
    assert counts == E.SCHEDULE_F64 and all(r.schedule == counts for r in chosen)
    assert max(r.schedule_estimate for r in chosen) <= E.RELTOL and len({r.schedule_estimate for r in chosen}) == 3
    assert all(r.schedule is None and r.schedule_estimate is None for r in given)
    for a, b in zip(chosen, given):
        assert np.array_equal(a.weights, b.weights) and a.history == b.history and len(a.history) == 3
    tile = synthetic.wind_mixing_problem(8, n_frames=4, weight_divisor=1e2, layer_sizes=(96, 24, 31), activations=("tanh", "identity"))
    twm = WindMixingNDE(tile.cfg, tile.x0, tile.bcs, O.solve(tile.cfg, tile.x0, tile.bcs, tile.weights_truth).astype(np.float32))
    try:
        with pytest.raises(ValueError, match="schedule covers the net-split shape"):
            train_NDE_ensemble(twm, _weights(tile.cfg, 2), PHYS[:2], etas[:2], maxiters=1, schedule="choose")
    finally:
        twm.close()
