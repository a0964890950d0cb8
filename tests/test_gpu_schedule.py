"""The per-save-interval step schedule on the GPU (colnde_set_schedule): the four-wave net-split kernels stepping save interval n with S_n RK4 steps.

Shapes are the smallest that cross the seams: 3, 17 and 40 columns (one partial tile; two tiles; three with a partial last one), 4 save points
(the uneven axis: 7), both matrix arithmetics, both tape kinds (rich: COLNDE_T16_SPLIT_RICH unset; plain: 0), single handles and K = 3 ensembles
with tests/test_gpu_ensemble.py's constants.  The float64 reference is the oracle unchanged, its `_step_times` replaced (tests/schedule_common.py)."""
import json
import os

import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.nde import ENGINE_REGTILE
from oracle import nde_oracle as O
from tests import schedule_common as C
from tests.test_gpu_ensemble import PHYS, _model_cfg, _weights

pytestmark = pytest.mark.gpu

MA = ["bf16x3_exact", "f32_mfma"]
TAPES = ["rich", "plain"]
SC = C.SC
PHYS3 = PHYS[:3]


def _tape(monkeypatch, tape):
    if tape == "plain":
        monkeypatch.setenv("COLNDE_T16_SPLIT_RICH", "0")             # before the handles are created
    else:
        monkeypatch.delenv("COLNDE_T16_SPLIT_RICH", raising=False)


_TRUTH = {}


def _truth(p):
    """the truth trajectories of a problem, solved once (float64 oracle at the configuration's own substeps) and shared"""
    key = (p.n_columns, p.cfg.save_times, p.cfg.diurnal)
    if key not in _TRUTH:
        _TRUTH[key] = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    return _TRUTH[key]


def _single(p, truth, ma, schedule=None, substeps=None, w=None, cfg=None):
    """(sol, (loss, terms), (total, terms, grad)) of one handle"""
    w = p.weights if w is None else w
    with colnde.ColumnNDE(cfg or p.cfg, p.n_columns, matrix_arithmetic=ma) as h:
        if substeps is not None:
            h.set_substeps(substeps)
        if schedule is not None:
            h.set_schedule(schedule)
            assert h.schedule() == tuple(schedule) and h.n_steps == sum(schedule)
            assert "schedule=%d/%d intervals" % (sum(schedule), len(schedule)) in h.describe()
        h.set_problem(p.x0, p.bcs, truth)
        sol = h.forward(w)
        lt, lterms = h.loss(w, SC)
        total, terms, g = h.loss_grad(w, SC)
        assert "net_split_forward=1 net_split_adjoint=1" in h.describe()
    return sol, (lt, lterms), (total, terms, g)


def _same(a, b):
    sol_a, (lt_a, lterms_a), (tot_a, terms_a, g_a) = a
    sol_b, (lt_b, lterms_b), (tot_b, terms_b, g_b) = b
    assert np.array_equal(sol_a, sol_b)
    assert lt_a == lt_b and np.array_equal(lterms_a, lterms_b)
    assert tot_a == tot_b and np.array_equal(terms_a, terms_b) and np.array_equal(g_a, g_b), np.abs(g_a - g_b).max()


def _ensemble(p, truth, W, ma, schedule=None, substeps=None):
    cfg = p.cfg if substeps is None else p.cfg.with_(substeps=substeps)
    with colnde.ColumnNDEEnsemble(cfg, p.n_columns, W.shape[0], physics=PHYS3, matrix_arithmetic=ma) as e:
        if schedule is not None:
            e.set_schedule(schedule)
            assert e.schedule() == tuple(schedule) and e.n_steps == sum(schedule)
        e.set_problem(p.x0, p.bcs, truth)
        return e.forward(W), e.loss(W, SC), e.loss_grad(W, SC)


# ---- 1. a uniform schedule keeps the bits of substeps = c ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tape", TAPES)
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("n_col", [3, 17, 40])
def test_uniform_schedule_keeps_the_bits(n_col, ma, tape, monkeypatch):
    _tape(monkeypatch, tape)
    p = C.base_problem(n_col)
    truth = _truth(p)
    for c in (2, 4):
        _same(_single(p, truth, ma, schedule=(c, c, c)), _single(p, truth, ma, substeps=c))


@pytest.mark.parametrize("tape", TAPES)
@pytest.mark.parametrize("ma", MA)
def test_uniform_schedule_keeps_the_bits_of_every_ensemble_row(ma, tape, monkeypatch):
    _tape(monkeypatch, tape)
    p = C.base_problem(17)
    truth, W = _truth(p), _weights(p.cfg, 3)
    for c in (2, 4):
        a, b = _ensemble(p, truth, W, ma, schedule=(c, c, c)), _ensemble(p, truth, W, ma, substeps=c)
        for x, y in zip(a, b):
            assert x.shape[0] == 3 and np.array_equal(x, y)


# ---- 2. the refined-axis identity, exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("diurnal", [False, True])
@pytest.mark.parametrize("ma", MA)
def test_schedule_is_substeps_on_the_refined_axis_bit_for_bit(ma, diurnal):
    """(8, 2, 4) on (0, 1, 2, 3)/256 takes the steps of substeps = 2 on (0, 1/4, 1/2, 3/4, 1, 2, 2.5, 3)/256: every dt and every stage time is the same
    float32 number, so the states at the four shared save points are the same bits.  diurnal: the top flux is evaluated at ts + ca dt."""
    p = C.base_problem(17, diurnal=diurnal)
    fine = C.with_axis(p, C.REFINED)
    with colnde.ColumnNDE(p.cfg, 17, matrix_arithmetic=ma) as h, colnde.ColumnNDE(fine.cfg, 17, matrix_arithmetic=ma) as f:
        h.set_schedule((8, 2, 4))
        h.set_problem(p.x0, p.bcs, None)
        f.set_problem(p.x0, p.bcs, None)
        a, b = h.forward(p.weights), f.forward(p.weights)
    assert np.array_equal(a, b[:, [0, 4, 5, 7]])
    assert np.abs(a[:, 3] - a[:, 0]).max() > 1e-3                    # (the columns do move)


# ---- 3. loss and gradient against float64 ---------------------------------------------------------------------------------------------------
def _errors(p, truth, schedule, got, monkeypatch):
    sol, (lt, _), (total, terms, g) = got
    C.oracle_schedule(monkeypatch, schedule)
    tot, terms_ref, g_ref, sol_ref = O.loss_and_grad(p.cfg, p.x0, p.bcs, p.weights, truth, np.array(SC, np.float64))
    return dict(sol=float(np.abs(sol - sol_ref).max()), loss=float(abs(lt - tot) / abs(tot)), loss_grad_total=float(abs(total - tot) / abs(tot)),
                grad=float(np.linalg.norm(g - g_ref) / np.linalg.norm(g_ref)))


def _assert_errors(err, what):
    print("schedule errors %s: %s" % (what, json.dumps(err)))
    assert err["sol"] < C.SOL_ATOL and err["loss"] <= C.LOSS_RTOL and err["loss_grad_total"] <= C.LOSS_RTOL and err["grad"] < C.GRAD_RTOL, (what, err)


@pytest.mark.parametrize("tape", TAPES)
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("schedule", [(8, 2, 4), (2, 2, 8)])
def test_loss_and_gradient_against_float64(schedule, ma, tape, monkeypatch):
    """Measured (profiles/schedule_errors.json): the float32 kernels against the float64 oracle stepping the same schedule."""
    _tape(monkeypatch, tape)
    p = C.base_problem(17)
    truth = _truth(p)
    _assert_errors(_errors(p, truth, schedule, _single(p, truth, ma, schedule=schedule), monkeypatch), (schedule, ma, tape))


# ---- 4. ensemble rows are single handles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tape", TAPES)
@pytest.mark.parametrize("ma", MA)
def test_ensemble_rows_are_single_handles_under_a_schedule(ma, tape, monkeypatch):
    _tape(monkeypatch, tape)
    p = C.base_problem(40)
    truth, W = _truth(p), _weights(p.cfg, 3)
    n = p.cfg.n_params
    sol, loss8, res = _ensemble(p, truth, W, ma, schedule=(8, 2, 4))
    for k in range(3):
        s1, (lt, lterms), (total, terms, g) = _single(p, truth, ma, schedule=(8, 2, 4), w=W[k], cfg=_model_cfg(p.cfg, PHYS3[k]))
        assert np.array_equal(sol[k], s1), k
        assert np.array_equal(res[k], np.concatenate([g, terms, [total, 0.0]]).astype(np.float32)), (k, np.abs(res[k, :n] - g).max())
        assert np.array_equal(loss8[k, :7], np.concatenate([lterms, [lt]]).astype(np.float32)), k


# ---- 5. the uneven axis ---------------------------------------------------------------------------------------------------------------------
def test_uneven_axis_minimal_schedule_against_float64(monkeypatch):
    p = C.with_axis(C.base_problem(17), C.UNEVEN)
    assert colnde.schedule_min(p.cfg) == C.UNEVEN_MIN
    S = tuple(C.pow2_ceil(v) for v in colnde.schedule_min(p.cfg))
    assert S == C.UNEVEN_POW2
    truth = _truth(p)
    got = _single(p, truth, "bf16x3_exact", schedule=S)              # (asserts colnde_schedule's counts and its total)
    assert sum(S) == 32
    _assert_errors(_errors(p, truth, S, got, monkeypatch), ("uneven", S))


def test_uneven_axis_chosen_schedule_beats_one_count():
    """choose_schedule at reltol = 1e-3 against choose_substeps on a twin.  The strict inequality rests on accuracy not forcing the unit intervals
    up to the long intervals' count: the same greedy run on the float64 oracle on this axis (8 columns) ends at the stability minima rounded to powers
    of two, 32 steps in all, where one count needs U = 16 in each of the 6 intervals."""
    reltol = 1e-3
    p = C.with_axis(C.base_problem(17), C.UNEVEN)
    with colnde.ColumnNDE(p.cfg, 17) as h, colnde.ColumnNDE(p.cfg, 17) as twin, colnde.ColumnNDE(p.cfg, 17) as a, colnde.ColumnNDE(p.cfg, 17) as b:
        for x in (h, twin, a, b):
            x.set_problem(p.x0, p.bcs, None)
        U, est_u = twin.choose_substeps(p.weights, reltol)
        S, est = h.choose_schedule(p.weights, reltol)
        print("uneven axis: choose_substeps U = %d (estimate %.3e), choose_schedule %r, total %d (estimate %.3e)" % (U, est_u, S, sum(S), est))
        assert U >= 16
        assert h.schedule() == S and h.n_steps == sum(S)
        for s, m in zip(S, C.UNEVEN_POW2):
            assert s >= m and s % m == 0 and (s // m) & (s // m - 1) == 0, (S, C.UNEVEN_POW2)      # a power-of-two multiple, not below the minimum
        assert est <= reltol
        a.set_schedule(S)
        b.set_schedule(tuple(2 * s for s in S))
        restated = C.estimate_norm(a.forward(p.weights), b.forward(p.weights), 16.0 / 15.0).max()
        assert abs(restated - est) <= 1e-3 * est, (restated, est)
        assert abs(h.error_estimate(p.weights) - est) <= 1e-3 * est           # colnde_error_estimate under the schedule: the same two solves
        assert sum(S) < 6 * U, (S, U)


# ---- 6. refusals, each by its message --------------------------------------------------------------------------------------------------------
def _refused(h, match, counts=None):
    with pytest.raises(colnde.ColndeError, match=match):
        h.set_schedule(counts if counts is not None else (4,) * (h.cfg.n_save - 1))


def test_refused_counts_and_planned_tapes():
    p = C.base_problem(3)
    truth = _truth(p)
    with colnde.ColumnNDE(p.cfg, 3) as h:
        _refused(h, r"schedule\[1\] = 1 is outside the stepper's stability bound on save interval 1: need >= 2", (2, 1, 2))
        _refused(h, r"schedule\[2\] = 0: every save interval takes at least one step", (2, 2, 0))
        _refused(h, r"schedule\[0\] = -3: every save interval", (-3, 2, 2))
        _refused(h, r"schedule\[1\] = 4097 is above 4096", (2, 4097, 2))
        with pytest.raises(ValueError, match="one count per save interval"):
            h.set_schedule((2, 2))
        assert h.schedule() == (2, 2, 2) and h.n_steps == 6          # nothing stuck
        h.set_problem(p.x0, p.bcs, truth)
        h.loss_grad(p.weights, SC)
        _refused(h, "sizes the tapes: set it before the first colnde_loss_grad", (4, 4, 4))
        with pytest.raises(colnde.ColndeError, match="sizes the tapes: choose it before the first colnde_loss_grad"):
            h.choose_schedule(p.weights, 1e-3)


def test_refused_engines():
    p = C.base_problem(3)
    with colnde.ColumnNDE(p.cfg.with_(stepper="rkc2"), 3) as h:
        _refused(h, "RK4 only: the RKC2 stage table depends on dt")
    big = synthetic.wind_mixing_problem(10000, n_frames=3, weight_divisor=1e2)
    with colnde.ColumnNDE(big.cfg, 10000) as h:
        _refused(h, "this handle runs regtile")
    with colnde.ColumnNDE(p.cfg, 3, engine=ENGINE_REGTILE) as h:
        _refused(h, "this handle runs regtile")
    wide = synthetic.wind_mixing_problem(16, n_frames=3, weight_divisor=1e2, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
    with colnde.ColumnNDE(wide.cfg, 16) as h:
        _refused(h, "runs the tile16 engine")
    fc = synthetic.free_convection_problem(8, Nz=32, n_save=4)
    with colnde.ColumnNDE(fc.cfg, 8) as h:
        _refused(h, "the free-convection models run the fc32 and tile16 engines")
    with colnde.FreeConvectionEnsemble(fc.cfg, 8, 2) as h:
        _refused(h, "a free-convection ensemble")
    cv = synthetic.free_convection_conv_problem(8, 3, Nz=32, n_save=4)
    with colnde.ColumnNDE(cv.cfg, 8, conv=3) as h:
        _refused(h, "a conv handle")
    with colnde.ClosureColumns(p.cfg, 3, 2) as h:
        _refused(h, "the closure engine")


def test_refused_switches_ensembles_and_shards(monkeypatch):
    p = C.base_problem(3)
    monkeypatch.setenv("COLNDE_T16_FWD_HELPER", "0")
    with colnde.ColumnNDE(p.cfg, 3) as h:
        _refused(h, "COLNDE_T16_FWD_HELPER=0 selects the three-wave or tile16 kernels")
    monkeypatch.delenv("COLNDE_T16_FWD_HELPER")
    with colnde.ColumnNDEEnsemble(p.cfg, 3, 3, physics=PHYS3) as e:
        with pytest.raises(colnde.ColndeError, match="this handle holds an ensemble of 3 models"):
            e.choose_schedule(p.weights, 1e-3)
    with colnde.ColumnNDE(p.cfg, 3) as h:
        h.set_problem(p.x0, p.bcs, None)
        h.set_global_columns(6)
        with pytest.raises(colnde.ColndeError, match="on a column shard"):
            h.choose_schedule(p.weights, 1e-3)


# ---- 7. lifecycle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
def test_lifecycle(ma):
    p = C.base_problem(17)
    truth = _truth(p)
    plain = _single(p, truth, ma)                                    # substeps = 2
    with colnde.ColumnNDE(p.cfg, 17, matrix_arithmetic=ma) as h:
        h.set_problem(p.x0, p.bcs, truth)
        h.set_schedule((8, 2, 4))
        s824 = h.forward(p.weights)
        assert not np.array_equal(s824, plain[0])
        h.set_schedule(None)                                         # back to the handle's substeps
        assert h.schedule() == (2, 2, 2) and "schedule=" not in h.describe()
        assert np.array_equal(h.forward(p.weights), plain[0])
        h.set_schedule((8, 2, 4))
        h.set_substeps(4)                                            # one count for every interval: clears the schedule
        assert h.schedule() == (4, 4, 4) and h.substeps == 4 and h.n_steps == 12
        h.set_schedule((8, 2, 4))
        g1 = h.loss_grad(p.weights, SC)
        g2 = h.loss_grad(p.weights, SC)
        assert g1[0] == g2[0] and np.array_equal(g1[1], g2[1]) and np.array_equal(g1[2], g2[2])
        assert np.array_equal(h.forward(p.weights), s824)
    # an ensemble's tapes, planned at creation, follow the schedule there and back
    W = _weights(p.cfg, 3)
    with colnde.ColumnNDEEnsemble(p.cfg, 17, 3, physics=PHYS3, matrix_arithmetic=ma) as e:
        e.set_problem(p.x0, p.bcs, truth)
        r0 = e.loss_grad(W, SC)
        e.set_schedule((8, 2, 4))
        r1 = e.loss_grad(W, SC)
        assert np.array_equal(r1, e.loss_grad(W, SC)) and not np.array_equal(r0, r1)
        e.set_schedule(None)
        assert np.array_equal(e.loss_grad(W, SC), r0)
