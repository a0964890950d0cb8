"""The closure-only engine (colnde_create_closure: engine_closure.hip) on the GPU against the float64 oracle at theta = 0: forward solve, loss,
the gradient with respect to the five Pacanowski-Philander constants (yardstick: the central finite difference of the float64 loss, itself held to
float64 autograd by tests/test_closure_host.py), edges, determinism, refusals, sharding and the optimiser trajectory.

Tolerances.  Forward solve and loss terms: those tests/test_gpu_parity.py applies to the wind-mixing forward solve (SOL_ATOL, LOSS_RTOL).  Gradient,
sharding and trajectory: at most 10x the error measured on the MI355X (the project's rule), the measured value next to each."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde import _lib
from colnde.config import to_c_config
from colnde.flux_compat import ADAM
from colnde.wind_mixing import optimise_modified_pacanowski_philander
from oracle import nde_oracle as O

from tests import closure_common as C
from tests.test_gpu_parity import LOSS_RTOL, SOL_ATOL, _record

pytestmark = pytest.mark.gpu

SC = np.array([1, 1, 1, 5e-3, 5e-3, 5e-3])
SETS = np.array([[1e-4, 1e-1, 1.0, 0.25, 1.0],            # the synthetic problem's own constants
                 [1.3e-4, 0.08, 0.8, 0.30, 0.5],           # Pr = 0.5: nu / Pr doubles the stiffest diffusivity
                 [2.6e-4, 0.05, 0.5, 0.40, 1.8]])
GRAD_RTOL = 5e-5             # per component, relative to that component: measured 1.5e-6 on the 3-column case, 5.1e-6 worst over the edge cases (1 column)
SHARD_RTOL = 1.4e-6          # halves summed against the whole, relative to the whole: measured 1.45e-7 (float32 summation order)
TRAJ_LOSS_RTOL = 3e-5        # loss sequence against the float64 loop: measured 3.0e-6
TRAJ_PARAM_RTOL = 3.8e-6     # final constants against the float64 loop: measured 3.9e-7


def _substeps(cfg, sets):
    return max(colnde.closure_min_substeps(cfg, s) for s in sets)


def _problem(n_columns, sets=SETS, **kw):
    p, theta0, truth = C.closure_problem(n_columns, **kw)
    need = _substeps(p.cfg, sets)
    if need > p.cfg.substeps:
        p, theta0, truth = C.closure_problem(n_columns, **dict(kw, substeps=need))
    return p, theta0, truth


def _engine(p, truth, K):
    eng = colnde.ClosureColumns(p.cfg, p.x0.shape[0], K)
    eng.set_problem(p.x0, p.bcs, truth)
    return eng


@pytest.fixture(scope="module")
def base():
    """3 columns x 5 frames, K = 3 sets, sub-steps from colnde_closure_min_substeps over the sets; float64 solves, losses and gradients once."""
    p, theta0, truth = _problem(3)
    sols = [C.f64_solve(p.cfg, p, s) for s in SETS]
    return dict(p=p, truth=truth, sols=sols,
                loss=[O.loss(p.cfg, s, truth, SC) for s in sols],
                grad=np.array([C.fd_grad(p.cfg, p, truth, s, SC) for s in SETS]))


@pytest.mark.parametrize("case", ["Nz32", "Nz20", "Nz64", "nonuniform_axis"])
def test_forward_against_the_float64_oracle(case):
    kw = {"Nz32": {}, "Nz20": dict(Nz=20), "Nz64": dict(Nz=64), "nonuniform_axis": {}}[case]
    sets = SETS[:2]
    p, theta0, truth = _problem(3, sets=sets, **kw)
    if case == "nonuniform_axis":                          # frames (0, 1, 3, 4)
        ts = p.cfg.save_times
        cfg = p.cfg.with_(save_times=(ts[0], ts[1], ts[3], ts[4]))
        cfg = cfg.with_(substeps=_substeps(cfg, sets))
        p.cfg = cfg
        truth = None
    with colnde.ClosureColumns(p.cfg, 3, 2) as eng:
        eng.set_problem(p.x0, p.bcs, truth)
        sol = eng.forward(sets.astype(np.float32))
    assert sol.shape == (2, 3, p.cfg.n_save, 3 * p.cfg.Nz)
    for k in range(2):
        err = np.abs(sol[k] - C.f64_solve(p.cfg, p, sets[k])).max()
        _record("closure/forward/%s/set%d" % (case, k), sol_abs=err)
        assert err < SOL_ATOL, (case, k, err)


def test_forward_cross_check_against_the_network_engine_at_zero_weights(base):
    p, truth = base["p"], base["truth"]
    with _engine(p, truth, 1) as eng, colnde.ColumnNDE(p.cfg, 3) as nde:
        sol = eng.forward(SETS[:1].astype(np.float32))[0]
        nde.set_problem(p.x0, p.bcs, truth)
        ref = nde.forward(np.zeros(p.cfg.n_params, np.float32))
    assert np.abs(sol - ref).max() < SOL_ATOL


@pytest.mark.parametrize("train_gradient", [True, False])
def test_loss_terms_and_total(base, train_gradient):
    p, truth = base["p"], base["truth"]
    sc = SC.copy()
    if not train_gradient:
        sc[3:] = 0.0
    with _engine(p, truth, 3) as eng:
        out = eng.loss(SETS.astype(np.float32), sc)
        rows = eng.loss_grad(SETS.astype(np.float32), sc)
    assert out.shape == (3, 8) and rows.shape == (3, 13)
    for k in range(3):
        tot, terms = O.loss(p.cfg, base["sols"][k], truth, sc)
        np.testing.assert_allclose(out[k, :6], terms, rtol=LOSS_RTOL, atol=1e-12)
        assert np.isclose(out[k, 6], tot, rtol=LOSS_RTOL) and out[k, 7] == 0.0
        np.testing.assert_array_equal(rows[k, 5:], out[k])            # loss and loss_grad share the forward kernel's sums
        if not train_gradient:
            assert (out[k, 3:6] == 0.0).all()


def test_gradient_against_the_float64_finite_difference(base):
    """K = 3 sets, one with Pr = 0.5; per component, relative to that component."""
    p, truth = base["p"], base["truth"]
    with _engine(p, truth, 3) as eng:
        rows = eng.loss_grad(SETS.astype(np.float32), SC)
    err = np.abs(rows[:, :5] / base["grad"] - 1)
    print("closure gradient, relative error per set and component:\n", err, "\nscaled gradients p dL/dp:\n", base["grad"] * SETS)
    _record("closure/gradient", max_rel=err.max(), **{"set%d_%s" % (k, C.KEYS[q]): err[k, q] for k in range(3) for q in range(5)})
    assert (np.abs(base["grad"] * SETS) > 1e-7).all()                # every component carries signal
    assert err.max() < GRAD_RTOL, err


@pytest.mark.parametrize("n_columns", [1, 3, 33, 65])
def test_edges_column_counts(n_columns):
    """wave and workgroup boundaries (4 columns per workgroup), K = 3 and K = 1: solve, loss and gradient against float64"""
    p, theta0, truth = _problem(n_columns)
    with _engine(p, truth, 3) as eng, _engine(p, truth, 1) as one:
        sol = eng.forward(SETS.astype(np.float32))
        rows = eng.loss_grad(SETS.astype(np.float32), SC)
        row1 = one.loss_grad(SETS[1:2].astype(np.float32), SC)
    np.testing.assert_array_equal(rows[1], row1[0])                  # row k of a K-set launch = a one-set launch of set k, bit for bit
    for k in (0, 2):
        assert np.abs(sol[k] - C.f64_solve(p.cfg, p, SETS[k])).max() < SOL_ATOL
        tot = C.f64_loss(p.cfg, p, truth, SETS[k], SC)[0]
        assert np.isclose(rows[k, 11], tot, rtol=LOSS_RTOL)
        g = C.fd_grad(p.cfg, p, truth, SETS[k], SC)
        err = np.abs(rows[k, :5] / g - 1)
        _record("closure/edges/cols%d/set%d" % (n_columns, k), max_rel=err.max())
        assert err.max() < GRAD_RTOL, (n_columns, k, err)


@pytest.mark.parametrize("case", ["n_save_2", "substeps_1"])
def test_edges_time_axis(case):
    sets = SETS[:1]
    if case == "n_save_2":
        p, theta0, truth = _problem(3, sets=sets, n_frames=2)
    else:                                                            # a quarter of tau: one RK4 step per save interval is stable
        p, theta0, truth = C.closure_problem(3, substeps=1, tau=43200.0)
        assert colnde.closure_min_substeps(p.cfg, sets[0]) == 1 and p.cfg.substeps == 1
    with _engine(p, truth, 1) as eng:
        sol = eng.forward(sets.astype(np.float32))
        rows = eng.loss_grad(sets.astype(np.float32), SC)
    assert np.abs(sol[0] - C.f64_solve(p.cfg, p, sets[0])).max() < SOL_ATOL
    g = C.fd_grad(p.cfg, p, truth, sets[0], SC)
    err = np.abs(rows[0, :5] / g - 1)
    _record("closure/edges/%s" % case, max_rel=err.max())
    assert err.max() < GRAD_RTOL, err


def test_determinism(base):
    import torch
    p, truth = base["p"], base["truth"]
    prm = torch.as_tensor(SETS.astype(np.float32)).cuda()
    with _engine(p, truth, 3) as eng:
        a = eng.loss_grad(prm, SC).clone()
        s1 = eng.forward(prm).clone()
        b = eng.loss_grad(prm, SC).clone()
        s2 = eng.forward(prm)
        assert torch.equal(a, b) and torch.equal(s1, s2)               # two launches on the same inputs: the same bits
    for k in range(3):
        with _engine(p, truth, 1) as one:
            r = one.loss_grad(prm[k:k + 1].contiguous(), SC)
            assert torch.equal(r[0], a[k]), k                            # row k of the K-set launch = the one-set launch of set k
            assert torch.equal(one.forward(prm[k:k + 1].contiguous())[0], s1[k])


def test_unstable_set_gives_a_non_finite_row_and_leaves_the_others_alone(base, monkeypatch):
    """Ric = 1e6 switches nu0 + nu_minus = 20 on at every face: lambda dt ~ 280 at the handle's sub-steps, growth ~1e8 per step.  NaN arithmetic, not a fault."""
    import torch
    p, truth = base["p"], base["truth"]
    bad = np.array([1e-4, 20.0, 1.0, 1e6, 1.0])
    sets = np.stack([SETS[0], bad, SETS[2]]).astype(np.float32)
    with _engine(p, truth, 3) as eng, _engine(p, truth, 2) as stable:
        with pytest.raises(colnde.ColndeError, match="set 1 "):          # the host twin sees the values and names the set
            eng.loss_grad(sets, SC)
        monkeypatch.setenv("COLNDE_ALLOW_UNSTABLE_DT", "1")
        rows = eng.loss_grad(torch.as_tensor(sets).cuda(), SC).cpu().numpy()
        ref = stable.loss_grad(torch.as_tensor(sets[[0, 2]]).cuda(), SC).cpu().numpy()
    assert not np.isfinite(rows[1, 11]) and not np.isfinite(rows[1, :5]).all()
    np.testing.assert_array_equal(rows[[0, 2]], ref)


REFUSED = dict(convective_adjustment=True, smooth_NN=True, smooth_Ri=True, diurnal=True, inplace_variant=True)


def test_refusals(base):
    p, truth = base["p"], base["truth"]
    L = _lib.lib()
    h = ctypes.c_void_p()
    for flag in REFUSED:
        c, keep = to_c_config(p.cfg, 3, 0, 0)
        setattr(c, flag, 1)
        assert L.colnde_create_closure(ctypes.byref(c), 1, ctypes.byref(h)) != 0
        assert flag.encode() in L.colnde_last_error(), (flag, L.colnde_last_error())
    for field, value, word in (("stepper", 1, b"RK4"), ("substeps", 0, b"substeps = 0"), ("engine", 1, b"engine"), ("Nz", 65, b"Nz"),
                               ("modified_pacanowski_philander", 0, b"modified_pacanowski_philander"), ("model", 1, b"model")):
        c, keep = to_c_config(p.cfg, 3, 0, 0)
        setattr(c, field, value)
        assert L.colnde_create_closure(ctypes.byref(c), 1, ctypes.byref(h)) != 0
        assert word in L.colnde_last_error(), (field, L.colnde_last_error())
    c, keep = to_c_config(p.cfg, 3, 0, 0)
    assert L.colnde_create_closure(ctypes.byref(c), 0, ctypes.byref(h)) != 0 and b"n_sets" in L.colnde_last_error()
    with _engine(p, truth, 2) as eng:
        assert eng.n_params == 5 and L.colnde_n_models(eng._h) == 2
        d = eng.describe()
        assert "engine=closure sets=2" in d and "tape_bytes=%d" % (2 * 3 * p.cfg.n_steps * 96 * 4) in d, d
        buf = (ctypes.c_float * 64)()
        sc = (ctypes.c_float * 6)(*SC)
        q = ctypes.cast(buf, ctypes.c_void_p)
        f = ctypes.c_float(0)
        weight_calls = [lambda: L.colnde_forward(eng._h, q, q), lambda: L.colnde_forward_dev(eng._h, q, q), lambda: L.colnde_loss_dev(eng._h, q, sc, q),
                        lambda: L.colnde_loss(eng._h, q, sc, buf, ctypes.byref(f)), lambda: L.colnde_loss_grad_dev(eng._h, q, sc, q),
                        lambda: L.colnde_loss_grad(eng._h, q, sc, buf, ctypes.byref(f), q), lambda: L.colnde_rhs(eng._h, q, q, q, 0.0, q, 1),
                        lambda: L.colnde_rhs_dev(eng._h, q, q, q, 0.0, q, 1), lambda: L.colnde_flux_dev(eng._h, q, q, q, 0.0, q, 1),
                        lambda: L.colnde_error_estimate(eng._h, q, ctypes.byref(f)), lambda: L.colnde_loss_per_tstep_dev(eng._h, q, q),
                        lambda: L.colnde_choose_substeps(eng._h, q, 0.0, None, None), lambda: L.colnde_infer_forcing_dev(eng._h, q, q, q, 1.0, q, 1),
                        lambda: L.colnde_ensemble_forward_dev(eng._h, q, q), lambda: L.colnde_ensemble_loss_grad_dev(eng._h, q, sc, q)]
        for call in weight_calls:
            assert call() != 0
            assert b"closure handle" in L.colnde_last_error(), L.colnde_last_error()
        # profiling ids 0, 1, 2
        eng.set_profiling(True)
        eng.loss_grad(SETS[:2].astype(np.float32), SC)
        for which in ("forward", "adjoint", "reduce"):
            ms, n = eng.kernel_time(which)
            assert n == 1 and ms > 0.0, which
    with colnde.ColumnNDE(p.cfg, 3) as nde:                              # and the closure calls refuse a network handle
        assert L.colnde_closure_forward_dev(nde._h, q, q) != 0 and b"not a closure handle" in L.colnde_last_error()


def test_sharding_two_halves_sum_to_the_whole():
    p, theta0, truth = _problem(4)
    prm = SETS.astype(np.float32)
    with _engine(p, truth, 3) as eng:
        whole = eng.loss_grad(prm, SC).astype(np.float64)
    parts = []
    for sl in (slice(0, 2), slice(2, 4)):
        with colnde.ClosureColumns(p.cfg, 2, 3) as half:
            half.set_global_columns(4)
            half.set_problem(p.x0[sl], p.bcs[sl], truth[sl])
            parts.append(half.loss_grad(prm, SC).astype(np.float64))
    err = np.abs((parts[0] + parts[1])[:, :12] / whole[:, :12] - 1)
    print("closure sharding, relative error of the summed halves:\n", err)
    _record("closure/sharding", max_rel=err.max())
    assert err.max() < SHARD_RTOL, err


def _f64_optimise(cfg, p, truth, starts, eta, iters, s_min=1e-3):
    """The optimiser loop in float64: O.solve / O.loss, the finite-difference gradient, O.adam_step on s = p / p_initial, the same clamp."""
    losses, finals = [], []
    for p0 in starts:
        s, m, v, bt = np.ones(5), np.zeros(5), np.zeros(5), (0.9, 0.999)
        seq = []
        for _ in range(iters):
            seq.append(C.f64_loss(cfg, p, truth, s * p0, SC)[0])
            g = C.fd_grad(cfg, p, truth, s * p0, SC) * p0
            s, m, v, bt = O.adam_step(s, g, m, v, eta, (0.9, 0.999), 1e-8, bt)
            s = np.clip(s, s_min, 10.0)
        losses.append(seq)
        finals.append(s * p0)
    return np.array(losses).T, np.array(finals)


def test_optimiser_trajectory_against_the_float64_loop():
    """5 iterations of ADAM(1e-2) from two starts 30 % off the truth's constants.  As tests/test_gpu_training_parity.py argues: ADAM's step is
    eta m^/(sqrt(v^) + eps); for |g| >> eps = 1e-8 it is eta sign(g) and blind to float32 error, for |g| ~ eps an absolute gradient error delta moves the step
    by up to eta delta / eps.  The scaled gradients here are 1e-5 .. 1e-2 >> eps, so the first step is eta sign(g) exactly and later steps move with the
    RELATIVE gradient error: the constants are held to a relative bound, the loss sequence to that file's LOSS_SEQ_RTOL."""
    eta, iters = 1e-2, 5
    starts = np.array([np.array(C.TRUTH) * 1.3, np.array(C.TRUTH) * 0.7])
    cfg0 = C.closure_problem(1)[0].cfg
    need = max(colnde.closure_min_substeps(cfg0, (2 * s[0], 2 * s[1], s[2], s[3], min(s[4], 1.0))) for s in starts)    # the optimiser's own margin
    p, theta0, truth = C.closure_problem(3, substeps=need)
    loss_o, par_o = _f64_optimise(p.cfg, p, truth, starts, eta, iters)
    seen = []
    p.truth = truth
    res = optimise_modified_pacanowski_philander(p, [ADAM(eta)], iters, starts=starts, cb=lambda *a: seen.append(a))
    assert res.losses.shape == (iters, 2) and res.terms.shape == (iters, 2, 6) and res.parameters.shape == (2, 5) and len(seen) == iters
    assert res.best == int(np.argmin(res.final_losses))
    e_loss = np.abs(res.losses / loss_o - 1).max()
    e_par = np.abs(res.parameters / par_o - 1).max()
    print("closure optimiser: loss sequence rel", e_loss, "final constants rel", e_par, "\n", res.losses, "\n", res.parameters)
    _record("closure/optimiser", loss_seq_rel=e_loss, params_rel=e_par)
    assert e_loss < TRAJ_LOSS_RTOL, (res.losses, loss_o)
    assert e_par < TRAJ_PARAM_RTOL, (res.parameters, par_o)
    for k in range(2):
        assert (np.diff(res.losses[:, k]) < 0).all() and res.final_losses[k] < res.losses[-1, k], res.losses[:, k]
