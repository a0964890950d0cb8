"""A handle that has been used, re-targeted and reconfigured computes what a fresh one does — bit for bit.

Every parity test creates a handle, sets it up once, calls it and throws it away; training keeps one for hours and gives it new problems, another
arithmetic for an A/B, a sub-step count, a schedule, a profiling switch, diagnostics between gradients.  The rule here: after a sequence of calls on one
handle, forward, loss and loss_grad return the bits (np.array_equal) of a handle created directly in the final configuration that makes only that one
call (tests/reuse_cases.py: `fresh`, computed once per configuration).  Where the parity tests hold the final configuration to float64 the same result
is held to their bounds too (`hold`: SOL_ATOL, LOSS_RTOL, GRAD_REL on the whole vector and per layer block), so that a reused handle and a fresh one
cannot be wrong together.  A handle that refuses a step by design is asserted to refuse it by name and is used again afterwards.

Handles (reuse_cases.KINDS): the net-split pair, regtile, tile16 with the LDS-staged and (COLNDE_T16_DWLDS=0) the L2-streaming dW GEMM, the wide
3 x 96-400-31 and 3 x 96-400-400-31 networks at one tile (36 dW records) and two (72), fc32 plain and conv=2, ConvectiveAdjustmentNDE at 64 levels under
RKC2, a wind-mixing ensemble (K = 3, per-model constants), a free-convection ensemble (K = 2) and a closure handle.  Sequence b — the arithmetic switched
after the tapes are planned — is the one that failed before colnde_set_matrix_arithmetic re-planned the dW GEMM's slice count: on the wide handles and
under COLNDE_T16_DWLDS=0, bf16x3 -> f32 ended in "dW GEMM launch failed: invalid argument" (36 slices for a kernel that takes multiples of 8), and
f32 -> bf16x3 ran 8 slices where a fresh handle plans 36."""
import numpy as np
import pytest

import colnde
from tests import reuse_cases as R
from tests.reuse_cases import BF, F32, KINDS, OTHER

pytestmark = pytest.mark.gpu

TAPES_PLANNED = "sizes the tapes"                     # colnde_set_substeps / _set_schedule / _choose_substeps / _choose_schedule after the first loss_grad


@pytest.fixture(autouse=True)
def _environment_of_the_kind(request, monkeypatch):
    """COLNDE_* switches of the handle kind, before any handle of the test (fresh ones included) is created"""
    kind = getattr(request.node, "callspec", None) and request.node.callspec.params.get("kind")
    for k, v in (KINDS[kind].get("env", {}) if kind else {}).items():
        monkeypatch.setenv(k, v)


def _ready(kind, ma=BF, which=1, **kw):
    h = R.open_handle(kind, ma, **kw)
    R.set_problem(h, R.problem(kind, which))
    return h


# ---- a. the problem replaced ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ALL)
def test_a_problem_replaced(kind):
    p1, p2 = R.problem(kind, 1), R.problem(kind, 2)
    with _ready(kind) as h:
        r1 = R.run(h, kind, p1.w)
        R.same(r1, R.fresh(kind, 1).res, "P1")
        R.set_problem(h, p2)                                              # P1's columns in reverse order, another truth
        r2 = R.run(h, kind, p2.w)
        R.same(r2, R.fresh(kind, 2).res, "P2 after P1")
        R.hold(kind, r2, which=2, tag="a/P2_after_P1")
        assert not np.array_equal(r2[2], r1[2])
        # device tensors: colnde_set_problem_dev, from the other problem again
        R.set_problem(h, p1, device=True)
        R.same(R.run(h, kind, p1.w), r1, "P1 from device tensors")
        R.set_problem(h, p2, device=True)
        R.same(R.run(h, kind, p2.w), r2, "P2 from device tensors")
        # no truth: the losses are refused by name, the solve keeps its bits, and the handle takes a truth again
        for device in (False, True):
            R.set_problem(h, p2, device=device, truth=False)
            for call in (lambda: h.loss(p2.w, R.scalings(kind)), lambda: h.loss_grad(p2.w, R.scalings(kind))):
                with pytest.raises(colnde.ColndeError, match="no truth trajectories"):
                    call()
            assert np.array_equal(np.asarray(h.forward(p2.w)), r2[0])
        R.set_problem(h, p1)
        R.same(R.run(h, kind, p1.w), r1, "P1 again")


# ---- b. the arithmetic switched after the tapes are planned ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [BF, F32])
@pytest.mark.parametrize("kind", R.ALL)
def test_b_arithmetic_switched_after_the_tapes_are_planned(kind, first):
    p = R.problem(kind)
    closure = KINDS[kind]["family"] == "closure"                         # (no matrix products: the switch is accepted and changes nothing)
    with _ready(kind, first) as h:
        for ma in (first, OTHER[first], first, OTHER[first]):
            h.set_matrix_arithmetic(ma)
            assert h.matrix_arithmetic == ma
            want = R.fresh(kind, 1, BF if closure else ma)
            R.same((R.grad_row(h, kind, p.w),), (want.res[2],), "loss_grad under %s after %s" % (ma, first))
            R.same(R.run(h, kind, p.w), want.res, "%s after %s" % (ma, first))
            if not closure:
                plan = h.plan()
                assert plan["dw_slices"] == want.plan["dw_slices"], (ma, plan, want.plan)
                assert plan == want.plan
        R.hold(kind, R.run(h, kind, p.w), tag="b/%s_first" % first)
    if kind in R.WIDE or kind == "tile16_l2":                            # the records do not fit the LDS: the two arithmetics plan different counts
        n_rec = 36 * ((p.n + 15) // 16) if kind in R.WIDE else None
        bf, f32 = R.fresh(kind, 1, BF).plan, R.fresh(kind, 1, F32).plan
        assert bf["bf16x3_dw"] and not f32["bf16x3_dw"] and f32["dw_slices"] % 8 == 0 and bf["dw_slices"] != f32["dw_slices"]
        if kind == "tile16_l2":                                          # 2 tiles x 3 intervals x 2 sub-steps x 4 stages = 48 records, with COLNDE_T16_DWLDS=0
            assert (bf["dw_slices"], f32["dw_slices"]) == (48, 8)
        if n_rec:                                                        # csrc/dw_plan.h: min(512, n_rec) against a multiple of 8 near n_rec / 8
            assert bf["dw_slices"] == n_rec and f32["dw_slices"] == (n_rec // 8 + 7) // 8 * 8


# ---- c. diagnostics between two gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PLAIN_SINGLE)
def test_c_diagnostics_between_two_gradients(kind):
    p = R.problem(kind)
    want = R.fresh(kind, 1).res
    with _ready(kind) as h:
        g1 = R.grad_row(h, kind, p.w)
        assert np.array_equal(g1, want[2])
        est = h.error_estimate(p.w)
        assert np.isfinite(est) and est >= 0.0
        lpt = h.loss_per_tstep(p.w)
        assert lpt.shape == (p.n, 6, p.cfg.n_save) and np.isfinite(lpt).all()
        assert np.array_equal(R.loss_row(h, kind, p.w), want[1])
        # rhs and flux at 70 columns: more than the handle was created with (scratch and, for 3 x 96-400-400-31, the activation rows grow)
        reps = -(-70 // p.n)
        x70, b70 = (np.ascontiguousarray(np.concatenate([a] * reps)[:70]) for a in (p.x0, p.bcs))
        dx, fl = h.rhs(x70, p.w, b70, 0.0), h.flux(x70, p.w, b70, 0.0)
        assert np.isfinite(dx).all() and np.isfinite(fl).all()
        e200 = R.embed(h, kind, 200)
        e1 = R.embed(h, kind, 1)
        assert all(np.isfinite(a).all() for a in e200 + e1) and all(np.asarray(a).shape[-2] == 200 for a in e200)
        g2 = R.grad_row(h, kind, p.w)
        assert np.array_equal(g2, g1)
        R.same(R.run(h, kind, p.w), want, "after the diagnostics")
        with R.open_handle(kind) as f:                                   # a fresh handle called at 1 column only
            R.same(e1, R.embed(f, kind, 1), "embedding at 1 column after 200")
            with R.open_handle(kind) as f2:                              # ... and the fresh 70-column diagnostics
                assert np.array_equal(f2.rhs(x70, p.w, b70, 0.0), dx) and np.array_equal(f2.flux(x70, p.w, b70, 0.0), fl)
    R.hold(kind, (want[0], want[1], g2), tag="c")


@pytest.mark.parametrize("kind", [k for k in R.ALL if k not in R.PLAIN_SINGLE])
def test_c_diagnostics_between_two_gradients_on_handles_that_refuse_some(kind):
    """The conv handle, the two ensembles and the closure handle refuse the single-model diagnostics by name; what they do serve (loss, the conv
    handle's loss_per_tstep, the embedding call of K models at 200 columns and then at 1 with other constants and weights) runs between two
    gradients that keep their bits."""
    p, k = R.problem(kind), KINDS[kind]
    want = R.fresh(kind, 1).res
    why = R.refusal(kind)
    with _ready(kind) as h:
        g1 = R.grad_row(h, kind, p.w)
        assert np.array_equal(g1, want[2])
        for name in ("colnde_error_estimate", "colnde_error_estimate_dev", "colnde_rhs", "colnde_rhs_dev", "colnde_flux", "colnde_flux_dev"):
            R.raw_refused(h, name, why)
        if k.get("conv"):
            lpt = h.loss_per_tstep(p.w)
            assert lpt.shape == (p.n, 6, p.cfg.n_save) and np.isfinite(lpt).all()
            R.raw_refused(h, "colnde_fc_embedded_step", why)
        else:
            R.raw_refused(h, "colnde_loss_per_tstep", why)
        assert np.array_equal(R.loss_row(h, kind, p.w), want[1])
        if k["family"] == "closure":
            for name in ("colnde_ensemble_wm_embedded", "colnde_ensemble_fc_embedded"):
                R.raw_refused(h, name, "takes K weight vectors, but this is a closure handle")
            e1 = None
        else:
            e200 = R.embed(h, kind, 200)
            e1 = R.embed(h, kind, 1)
            assert all(np.isfinite(a).all() for a in e200 + e1) and all(np.asarray(a).shape[:2] == (k.get("K", 1), 200) for a in e200)
        g2 = R.grad_row(h, kind, p.w)
        assert np.array_equal(g2, g1)
        R.same(R.run(h, kind, p.w), want, "after the diagnostics and the refusals")
        if e1 is not None:
            with R.open_handle(kind) as f:                               # a fresh handle called at 1 column only
                R.same(e1, R.embed(f, kind, 1), "embedding at 1 column after 200")
    R.hold(kind, (want[0], want[1], g2), tag="c")


# ---- d. global columns -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PLAIN_SINGLE + ["closure"])
def test_d_global_columns(kind):
    p = R.problem(kind)
    with _ready(kind) as h:
        r_n = R.run(h, kind, p.w)
        R.same(r_n, R.fresh(kind, 1).res, "n")
        h.set_global_columns(2 * p.n)
        r_2n = R.run(h, kind, p.w)
        R.same(r_2n, R.fresh(kind, 1, gcols=2 * p.n).res, "2n")
        assert np.array_equal(r_2n[0], r_n[0]) and not np.array_equal(r_2n[2], r_n[2])
        with pytest.raises(colnde.ColndeError, match="global column count"):
            h.set_global_columns(p.n - 1)
        R.same(R.run(h, kind, p.w), r_2n, "2n after the refusal")
        h.set_global_columns(p.n)
        R.same(R.run(h, kind, p.w), r_n, "back to n")
    R.hold(kind, r_n, tag="d")


@pytest.mark.parametrize("kind", [k for k in R.ALL if k not in R.PLAIN_SINGLE + ["closure"]])
def test_d_global_columns_refused_by_name(kind):
    """A conv handle and the ensembles take no global column count: refused by name, and the handle goes on with its bits."""
    p = R.problem(kind)
    want = R.fresh(kind, 1).res
    with _ready(kind) as h:
        R.same(R.run(h, kind, p.w), want, "n")
        for n in (2 * p.n, p.n):
            with pytest.raises(colnde.ColndeError, match=R.refusal(kind)):
                h.set_global_columns(n)
        assert h.n_columns_total == p.n
        assert np.array_equal(R.grad_row(h, kind, p.w), want[2])
        R.same(R.run(h, kind, p.w), want, "after the refusals")
    R.hold(kind, want, tag="d")


# ---- e. profiling ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ALL)
def test_e_profiling(kind):
    p = R.problem(kind)
    want = R.fresh(kind, 1)
    closure = KINDS[kind]["family"] == "closure"
    with _ready(kind) as h:
        h.set_profiling(True)
        R.same(R.run(h, kind, p.w), want.res, "profiling on")              # forward, loss, loss_grad: three forward solves, one gradient
        g = R.grad_row(h, kind, p.w)
        assert np.array_equal(g, want.res[2])
        counts = {k: h.kernel_time(k)[1] for k in ("forward", "adjoint", "reduce", "dw1")}
        taped = not closure and (want.plan["dw_taped"] or want.plan["engine"] == colnde.nde.ENGINE_REGTILE)
        assert counts["forward"] == 4 and counts["adjoint"] == 2 and counts["dw1"] == (2 if taped else 0), counts
        assert counts["reduce"] == (3 if closure else 2), counts         # (the closure engine times the reduction of `loss` too)
        assert all(h.kernel_time(k)[0] > 0.0 for k in ("forward", "adjoint", "reduce"))
        h.set_profiling(False)
        h.reset_kernel_times()
        R.same(R.run(h, kind, p.w), want.res, "profiling off again")
        assert all(h.kernel_time(k) == (0.0, 0) for k in colnde.nde.KERNEL_IDS)
    R.hold(kind, want.res, tag="e")


# ---- f. step counts before the tapes exist -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PLAIN_SINGLE)
def test_f_step_counts_before_the_tapes_exist(kind):
    """The handle is created with one count more than the kind's, solves at twice the kind's, chooses a count, and is then given the kind's own: the
    sequence ends in the configuration every other sequence of this file (and, for the wind-mixing kinds, the parity tests' sub-step count) checks."""
    p = R.problem(kind)
    s2 = p.cfg.substeps
    created, s1 = s2 + 1, 2 * s2
    assert colnde.min_substeps(p.cfg) <= s2
    with _ready(kind, substeps=created) as h:
        assert h.substeps == created
        h.set_substeps(s1)
        sol_s1 = h.forward(p.w)
        assert h.substeps == s1 and np.array_equal(sol_s1, R.fresh(kind, 1, substeps=s1).res[0])
        chosen, est = h.choose_substeps(p.w, 0.5)
        assert h.substeps == chosen and np.isfinite(est)
        h.set_substeps(s2)
        assert h.substeps == s2
        r = R.run(h, kind, p.w)
        R.same(r, R.fresh(kind, 1).res, "substeps %d after %d (created), %d and the chosen %d" % (s2, created, s1, chosen))
        R.hold(kind, r, tag="f/substeps%d" % s2)
        # the tapes are planned: another count, a schedule and a chosen schedule are refused by name; the handle goes on
        with pytest.raises(colnde.ColndeError, match=TAPES_PLANNED):
            h.set_substeps(s1)
        with pytest.raises(colnde.ColndeError, match=TAPES_PLANNED):
            h.choose_substeps(p.w, 0.5)
        sched_refusal = TAPES_PLANNED if kind == "netsplit" else "a step schedule covers"
        with pytest.raises(colnde.ColndeError, match=sched_refusal):
            h.set_schedule([s1] * (p.cfg.n_save - 1))
        with pytest.raises(colnde.ColndeError, match=sched_refusal):
            h.choose_schedule(p.w, 0.5)
        h.set_substeps(s2)                                               # (the count in force: accepted, nothing changes)
        assert h.substeps == s2 and np.array_equal(R.grad_row(h, kind, p.w), r[2])
        R.same(R.run(h, kind, p.w), r, "after the refusals")


@pytest.mark.parametrize("kind", R.PLAIN_SINGLE)
def test_f_error_estimate_leaves_the_step_in_force(kind):
    """The doubled solve of colnde_error_estimate runs at twice the count (RKC2: with the stage table of the shorter step): neither is left in force."""
    p = R.problem(kind)
    want = R.fresh(kind, 1).res
    with _ready(kind) as h:
        est = h.error_estimate(p.w)
        assert np.isfinite(est) and h.substeps == p.cfg.substeps
        assert np.array_equal(h.forward(p.w), want[0])
        est2 = h.error_estimate(p.w)
        assert est2 == est
        R.same(R.run(h, kind, p.w), want, "after two error estimates")
        assert h.error_estimate(p.w) == est                              # ... and with the tapes planned


def test_f_step_counts_on_the_conv_handle():
    """colnde_set_substeps serves a conv handle before its tapes exist (f.1, f.3) and refuses afterwards (f.5); the error-controlled calls and the
    schedule are refused by name throughout."""
    kind = "fc32_conv2"
    p = R.problem(kind)
    s2 = p.cfg.substeps
    created, s1 = s2 + 1, 2 * s2
    why = R.refusal(kind)
    with _ready(kind, substeps=created) as h:
        assert h.substeps == created
        h.set_substeps(s1)
        assert h.substeps == s1 and np.array_equal(h.forward(p.w), R.fresh(kind, 1, substeps=s1).res[0])
        for name in ("colnde_choose_substeps", "colnde_error_estimate"):
            R.raw_refused(h, name, why)
        assert h.substeps == s1
        h.set_substeps(s2)
        r = R.run(h, kind, p.w)
        R.same(r, R.fresh(kind, 1).res, "substeps %d after %d (created) and %d" % (s2, created, s1))
        with pytest.raises(colnde.ColndeError, match=TAPES_PLANNED):
            h.set_substeps(s1)
        R.raw_refused(h, "colnde_choose_substeps", why)
        with pytest.raises(colnde.ColndeError, match=r"a step schedule covers .* a conv handle \(colnde_create_conv, conv=2\) runs the fc32 engine"):
            h.set_schedule([s1] * (p.cfg.n_save - 1))
        with pytest.raises(colnde.ColndeError, match=r"a step schedule covers .* a conv handle"):
            h.choose_schedule(p.w, 0.5)
        h.set_substeps(s2)
        assert h.substeps == s2 and np.array_equal(R.grad_row(h, kind, p.w), r[2])
        R.same(R.run(h, kind, p.w), r, "after the refusals")


@pytest.mark.parametrize("kind", R.ROWS)
def test_f_step_counts_refused_by_name_on_the_k_row_handles(kind):
    """Ensembles and the closure handle share one sub-step count fixed at creation: every call of sequence f is refused by name (the wind-mixing
    ensemble's schedule is served: sequence g), before and after the first loss_grad, and the bits stay."""
    p = R.problem(kind)
    want = R.fresh(kind, 1).res
    why = R.refusal(kind)
    sched = {"fc_ens": r"a step schedule covers .* a free-convection ensemble \(colnde_create_fc_ensemble\) runs the fc32 engine",
             "closure": r"a step schedule covers .* the closure engine \(colnde_create_closure\) steps with one substeps"}

    def refusals(h):
        for name in ("colnde_set_substeps", "colnde_choose_substeps", "colnde_choose_schedule", "colnde_error_estimate", "colnde_error_estimate_dev"):
            R.raw_refused(h, name, why)
        if kind in sched:
            with pytest.raises(colnde.ColndeError, match=sched[kind]):
                h.set_schedule([4] * (p.cfg.n_save - 1))
        assert h.substeps == p.cfg.substeps

    with _ready(kind) as h:
        refusals(h)
        assert np.array_equal(np.asarray(h.forward(p.w)), want[0])
        refusals(h)
        R.same(R.run(h, kind, p.w), want, "after the refusals")
        refusals(h)
        assert np.array_equal(R.grad_row(h, kind, p.w), want[2])
    R.hold(kind, want, tag="f")


# ---- g. ensembles ------------------------------------------------------------------------------------------------------------------------------------
def test_g_ensemble_physics_replaced():
    kind, p = "wm_ens", R.problem("wm_ens")
    with _ready(kind) as e:
        r1 = R.run(e, kind, p.w)
        R.same(r1, R.fresh(kind, 1, physics="PH1").res, "PH1")
        e.set_physics(R.PH2)
        r2 = R.run(e, kind, p.w)
        R.same(r2, R.fresh(kind, 1, physics="PH2").res, "PH2 after PH1")
        R.hold(kind, r2, physics="PH2", tag="g/PH2_after_PH1")
        assert not np.array_equal(r2[2][0], r1[2][0])                    # (the constants matter)
        bad = R.PH1.copy()
        bad[2, 1] = 100.0
        with pytest.raises(colnde.ColndeError, match="model 2"):
            e.set_physics(bad)
        R.same(R.run(e, kind, p.w), r2, "PH2 after the refusal")
        e.set_physics(R.PH1)
        R.same(R.run(e, kind, p.w), r1, "PH1 again")
    R.hold(kind, r1, physics="PH1", tag="g/PH1_again")


@pytest.mark.parametrize("ma", [BF, F32])
def test_g_ensemble_schedules_longer_shorter_longer(ma):
    kind, p = "wm_ens", R.problem("wm_ens")
    with _ready(kind, ma) as e:
        r0 = R.run(e, kind, p.w)
        R.same(r0, R.fresh(kind, 1, ma).res, "substeps")
        for sched in ((8, 2, 4), (2, 4, 2), (4, 8, 4)):                  # 14, 8, 16 steps against the 6 of substeps = 2: the tapes are planned again each time
            e.set_schedule(sched)
            assert e.schedule() == sched and e.n_steps == sum(sched)
            want = R.fresh(kind, 1, ma, schedule=sched)
            R.same(R.run(e, kind, p.w), want.res, "schedule %s" % (sched,))
            assert e.plan() == want.plan
        e.set_physics(R.PH2)                                             # ... and the constants under a schedule
        R.same(R.run(e, kind, p.w), R.fresh(kind, 1, ma, physics="PH2", schedule=(4, 8, 4)).res, "PH2 under (4, 8, 4)")
        e.set_physics(R.PH1)
        e.set_schedule(None)
        R.same(R.run(e, kind, p.w), r0, "substeps again")
        assert e.plan() == R.fresh(kind, 1, ma).plan
    R.hold(kind, r0, tag="g/schedules/%s" % ma)


def test_g_constants_that_outgrow_the_schedule_are_refused_at_the_solve():
    from tests.test_gpu_ensemble import _model_cfg
    kind, p = "wm_ens", R.problem("wm_ens")
    assert p.cfg.substeps == 2
    assert [colnde.min_substeps(_model_cfg(p.cfg, r)) for r in R.PH_LOW] == [1, 1, 1] and max(colnde.min_substeps(_model_cfg(p.cfg, r)) for r in R.PH1) == 2
    with _ready(kind, physics="LOW") as e:
        R.same(R.run(e, kind, p.w), R.fresh(kind, 1, physics="LOW").res, "LOW")
        e.set_schedule((1, 1, 2))                                        # one step per interval is stable under LOW
        r_s = R.run(e, kind, p.w)
        R.same(r_s, R.fresh(kind, 1, physics="LOW", schedule=(1, 1, 2)).res, "LOW under (1, 1, 2)")
        e.set_physics(R.PH1)                                             # accepted: substeps = 2 is stable; the schedule in force is not
        for call in (lambda: e.forward(p.w), lambda: e.loss(p.w, R.scalings(kind)), lambda: e.loss_grad(p.w, R.scalings(kind))):
            with pytest.raises(colnde.ColndeError, match=r"schedule\[0\] = 1 puts the RK4 step of save interval 0 outside its stability region: need >= 2"):
                call()
        e.set_schedule(None)
        r = R.run(e, kind, p.w)
        R.same(r, R.fresh(kind, 1, physics="PH1").res, "PH1 at substeps = 2")
    R.hold(kind, r, physics="PH1", tag="g/outgrown_schedule")


def test_g_on_the_free_convection_ensemble():
    """Its models differ in weights only: constants and a schedule are refused by name, between gradients that keep their bits."""
    kind, p = "fc_ens", R.problem("fc_ens")
    want = R.fresh(kind, 1).res
    with _ready(kind) as e:
        assert np.array_equal(R.grad_row(e, kind, p.w), want[2])
        with pytest.raises(colnde.ColndeError, match="a free-convection ensemble has no closure constants to vary"):
            e.set_physics(R.PH1[:2])
        with pytest.raises(colnde.ColndeError, match=r"a free-convection ensemble \(colnde_create_fc_ensemble\) runs the fc32 engine"):
            e.set_schedule((8, 2, 4, 2))
        e.set_schedule(None)                                             # (nothing to clear: accepted)
        R.same(R.run(e, kind, p.w), want, "after the refusals")
