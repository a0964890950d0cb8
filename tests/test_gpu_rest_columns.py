"""Every device restatement of the Richardson-number closure on columns at rest (tests/rest_cases.py): u = v = 0 on whole columns or below a sheared
upper half, with stable, unstable and neutral stratification on the resting faces, and one sheared face with Ri == 0 exactly.  The training kernels
(ε = 1e-7 inside the gradients) see S2 = 5e-17 and Ri ~ ±1e15 there; the embedding kernels (no ε) see +Inf, −Inf and 0/0.

The reference is float64 on the same float32 inputs.  A comparison leaves out only the entries where the float64 reference is itself non-finite, and
every test asserts that this set is the neutral resting layer's (kind 2) and that the kernel's non-finite entries are exactly the reference's.

Bounds.  Training engines (but for the two T terms of the loss: T_TERMS_RTOL below), closure engine, implicit step, ∂z forcings: the existing
constants of tests/test_gpu_parity.py, tests/test_gpu_closure.py, tests/test_column_ops.py and tests/test_gpu_wm_embed.py; profile and
pre-training: those of tests/test_gpu_wm_profile.py, tests/test_gpu_pretrain.py and tests/test_gpu_wm_pretrain.py.  Face fluxes: 10 x the distance
of the float32 NumPy restatement from the float64 one ON THESE INPUTS over the finite entries, the larger over halos given / absent, computed on
the CPU by tests/test_rest_cases_host.py, which also asserts that the constants below lie between 10 x and 12 x that distance:
    baseline (uw, vw, wT)   ca = 0: 2.09e-8, 9.30e-8, 7.40e-8     ca = 1: 2.09e-8, 9.30e-8, 7.41e-9
    NN diagnosis            ca = 0: 2.20e-7, 2.84e-7, 7.80e-8     ca = 1: 2.20e-7, 2.84e-7, 3.11e-8
No bound here comes from a kernel's own output."""
import functools

import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as O
from tests import closure_common as C
from tests import rest_cases as RC
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W

pytestmark = pytest.mark.gpu

N, NZ, FRAMES = 16, 32, 5
DT = 60.0
FIELDS = ("uw", "vw", "wT")
BASE_BOUND = {0: (2.10e-7, 9.30e-7, 7.41e-7), 1: (2.10e-7, 9.30e-7, 7.41e-8)}
NN_BOUND = {0: (2.21e-6, 2.85e-6, 7.80e-7), 1: (2.21e-6, 2.85e-6, 3.11e-7)}
STEP_TOL = (2e-5, 2e-5, 2e-6)        # tests/test_column_ops.py test_gpu_implicit_diffusion_matches_oracle: u′, v′ of their range, T′ relative
TRAIN_SC = np.array([1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3])
# The two T terms of the training loss on this input: 10 x the distance of oracle.cref's float32 terms from the float64 oracle's, 7.75e-5 (the
# larger of the T and the dT/dz term over the three inputs of _train_ref; tests/test_rest_cases_host.py recomputes it).  T moves by ~1e-4 of an
# O(1) profile over the five frames, so these terms (1e-8, 1e-7 of a loss of 7e-5) are float32 round-off of the trajectories: the float32 C oracle
# alone uses up LOSS_RTOL = 8e-5, which leaves a kernel that sums in another order no room (the net-split and regtile kernels: 9.2e-5 on the
# MI355X).  The u and v terms and the total keep LOSS_RTOL.
T_TERMS_RTOL = 7.76e-4
MAS = ("bf16x3_exact", "f32_mfma")


def _record(case, **errs):
    from tests.test_gpu_parity import _record as rec
    rec("rest_columns/" + case, **errs)


def _cuda(*arrs):
    import torch
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


# ------------------------------------------------------------------------------------------------------------------ a. training engines
@functools.lru_cache(maxsize=None)
def _train_ref(n, smooth_Ri=False):
    """the rest_state problem (n = 1: one column of kind 0), its float32 truth and the float64 oracle's loss, terms, gradient and solution"""
    kw = dict(smooth_Ri=True) if smooth_Ri else {}
    rs = RC.rest_state(synthetic.wind_mixing_problem(n, n_frames=FRAMES, weight_divisor=1e2, **kw))
    p = rs.p
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    tot, terms, g, sol = O.loss_and_grad(p.cfg, p.x0, p.bcs, p.weights, truth, TRAIN_SC)
    assert np.isfinite(sol).all() and np.isfinite(g).all() and np.isfinite(terms).all()
    for a in (truth, g, sol, p.x0):
        a.setflags(write=False)
    return p, truth, tot, terms, g, sol


TRAIN_CASES = [(e, ma, N, False) for e in (0, 1, 2) for ma in MAS] + [(1, ma, N, True) for ma in MAS] + [(e, MAS[0], 1, False) for e in (0, 1, 2)]


@pytest.mark.parametrize("engine,ma,n,smooth_Ri", TRAIN_CASES)
def test_training_engines(engine, ma, n, smooth_Ri):
    """forward, loss and loss_grad of the net-split (engine 0 = AUTO at this size), tile16 and regtile kernels, both matrix arithmetics (regtile's
    physics has one code form per arithmetic), tile16 with the three-face Ri filter (it sums three Ri ~ 1e15), and one whole column at rest."""
    import colnde
    from tests.test_gpu_parity import GRAD_REL, LOSS_RTOL, SOL_ATOL, _rel
    p, truth, tot, terms, g, sol = _train_ref(n, smooth_Ri)
    with colnde.ColumnNDE(p.cfg, n, engine=engine, matrix_arithmetic=ma) as nde:
        nde.set_problem(p.x0, p.bcs, truth)
        sol_g = nde.forward(p.weights)
        tot_l, terms_l = nde.loss(p.weights, TRAIN_SC)
        tot_g, terms_g, grad_g = nde.loss_grad(p.weights, TRAIN_SC)
        plan = nde.plan()
    if engine:
        assert plan["engine"] == engine
    elif n == N:
        assert plan["split_forward"] and plan["split_adjoint"], plan
    errs = dict(sol_abs=float(np.abs(sol_g - sol).max()), loss_rel=abs(tot_g - tot) / abs(tot), grad_rel=_rel(grad_g, g))
    errs["T_terms_rel"] = float(np.abs(np.asarray(terms_g, np.float64)[[2, 5]] / terms[[2, 5]] - 1).max())
    print("rest columns, engine %d %s n=%d smooth_Ri=%d:" % (engine, ma, n, smooth_Ri), errs)
    _record("train/engine%d/%s/%d/%d" % (engine, ma, n, smooth_Ri), **errs)
    assert np.isfinite(sol_g).all() and np.isfinite(grad_g).all() and np.isfinite(terms_l).all() and np.isfinite(terms_g).all()
    assert errs["sol_abs"] < SOL_ATOL
    rtol = np.where(np.arange(6) % 3 == 2, T_TERMS_RTOL, LOSS_RTOL)
    for got in (terms_l, terms_g):
        assert (np.abs(got - terms) <= rtol * np.abs(terms) + 1e-12).all(), (got, terms)
    assert np.isclose(tot_l, tot, rtol=LOSS_RTOL) and np.isclose(tot_g, tot, rtol=LOSS_RTOL)
    assert errs["grad_rel"] < GRAD_REL


# ------------------------------------------------------------------------------------------------------------------ b. closure engine
@pytest.mark.parametrize("n,Nz", [(N, 32), (1, 20), (1, 64)])
def test_closure_engine(n, Nz):
    """ClosureColumns, K = 3: forward, loss terms and all five gradient components against the float64 finite difference.  A resting face has
    |y| ~ 1e15: sech² must be zero there, against Ri / S2 ~ 1e32."""
    import colnde
    from tests.test_gpu_closure import GRAD_RTOL, SC, SETS
    from tests.test_gpu_parity import LOSS_RTOL, SOL_ATOL
    rs, truth = RC.rest_closure_problem(n, SETS, Nz=Nz, n_frames=FRAMES)
    p = rs.p
    with colnde.ClosureColumns(p.cfg, n, 3) as eng:
        eng.set_problem(p.x0, p.bcs, truth)
        sol = eng.forward(SETS.astype(np.float32))
        out = eng.loss(SETS.astype(np.float32), SC)
        rows = eng.loss_grad(SETS.astype(np.float32), SC)
    assert np.isfinite(sol).all() and np.isfinite(out).all()
    for k in range(3):
        ref = C.f64_solve(p.cfg, p, SETS[k])
        err = float(np.abs(sol[k] - ref).max())
        tot, terms = O.loss(p.cfg, ref, truth, SC)
        g = C.fd_grad(p.cfg, p, truth, SETS[k], SC)
        with np.errstate(invalid="ignore"):
            gerr = np.abs(rows[k, :5] / g - 1)
        print("rest columns, closure n=%d Nz=%d set %d: sol %.3e, gradient %s against %s (rel %s)" % (n, Nz, k, err, rows[k, :5], g, gerr))
        _record("closure/%d/%d/set%d" % (n, Nz, k), sol_abs=err, **{C.KEYS[q]: gerr[q] for q in range(5)})
        assert err < SOL_ATOL, (k, err)
        np.testing.assert_allclose(out[k, :6], terms, rtol=LOSS_RTOL, atol=1e-12)
        assert np.isclose(out[k, 6], tot, rtol=LOSS_RTOL)
        np.testing.assert_array_equal(rows[k, 5:], out[k])
        assert np.isfinite(rows[k]).all(), rows[k]
        assert gerr.max() < GRAD_RTOL, (k, rows[k, :5], g)


# ------------------------------------------------------------------------------------------------------------------ c. implicit step
@functools.lru_cache(maxsize=None)
def _embed_state(n, Nz=32):
    """the columns at rest in ocean units, and a problem with the embedding tests' weights (weight_divisor = 1) on the same columns"""
    kw = {} if Nz == 32 else {"Nz": Nz}
    p = synthetic.wind_mixing_problem(n, n_frames=FRAMES, weight_divisor=1.0, **kw)
    rs = RC.rest_state(p)
    for a in (rs.u, rs.v, rs.T, rs.top, rs.halo_bottom, rs.halo_top):
        a.setflags(write=False)
    return rs


def _same_non_finite(got, ref, what):
    """the kernel is NaN exactly where the float64 reference is, and has no ±Inf (the reference has none either)"""
    assert not np.isinf(ref).any() and not np.isinf(got).any(), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.argwhere(np.isnan(got) != np.isnan(ref))[:8])
    return np.isfinite(ref)


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [False, True])
@pytest.mark.parametrize("Nz", [16, 20, 32, 64])
def test_implicit_step(Nz, ca, halo):
    """80 columns: one full 64-column block and a ragged one; Nz = 16, 32, 64 the LDS kernel, 20 the generic one"""
    import torch
    import colnde
    n = 80
    rs = _embed_state(n, Nz)
    dz = W.LZ / Nz
    hb = rs.halo_bottom if halo else None
    k2 = rs.mask(2)
    want = O.modified_pacanowski_philander_step(rs.u, rs.v, rs.T, DT, dz, convective_adjustment=ca, halo_bottom=hb, **W.MPP)
    hcfg = synthetic.free_convection_problem(1, Nz=Nz, n_save=2).cfg            # any handle kind: only Nz is the handle's
    with colnde.ColumnNDE(hcfg, 1) as nde:
        got = nde.implicit_diffusion(rs.u, rs.v, rs.T, DT, dz, W.mpp_params(), ca, hb)
        ud, vd, Td, hd = _cuda(rs.u, rs.v, rs.T, hb)
        dev = nde.implicit_diffusion(ud, vd, Td, DT, dz, W.mpp_params(), ca, hd)
        torch.cuda.synchronize()
        dev = tuple(d.cpu().numpy() for d in dev)
    errs = []
    for f, (g, d, w, tol) in enumerate(zip(got, dev, want, STEP_TOL)):
        w = w.copy()
        bad = ~np.isfinite(w).all(axis=1)
        if f == 2 and not ca:
            assert np.isnan(w[k2, 1:]).all()                                     # (T′[0] = T_bottom is written after the solve)
        assert np.array_equal(bad, k2 & (f < 2 or not ca)), (f, np.flatnonzero(bad))
        ok = _same_non_finite(g, w, "field %d" % f)
        assert np.array_equal(g, d, equal_nan=True)                              # the device twin: the same bits
        e = float(np.abs(g[ok] - w[ok]).max() / np.abs(w[ok]).max())
        errs.append(e)
        assert e <= tol, (f, e)
    assert np.array_equal(got[2][:, 0], rs.T[:, 0])                              # T′[1] = T_bottom bit for bit, kind 2 included
    print("rest columns, implicit step Nz=%d ca=%d halo=%d: u′ %.3e v′ %.3e T′ %.3e" % ((Nz, ca, halo) + tuple(errs)))
    _record("implicit/%d/%d/%d" % (Nz, ca, halo), **dict(zip(("u", "v", "T"), errs)))


# ------------------------------------------------------------------------------------------------------------------ d. flux diagnoses, fused step
def _flux_check(tag, got, ref, bounds, rs, ca):
    errs = []
    for k, (g, r, b) in enumerate(zip(got, ref, bounds)):
        nan = np.isnan(r)
        assert np.array_equal(nan.any(axis=1), rs.mask(2) & (k < 2 or not ca)), (tag, FIELDS[k])
        ok = _same_non_finite(g, r, (tag, FIELDS[k]))
        e = float(np.abs(g[ok].astype(np.float64) - r[ok]).max() / np.abs(r[ok]).max())
        errs.append(e)
        assert e <= b, (tag, FIELDS[k], e, b)
    if ca:
        assert np.isfinite(got[2][rs.mask(2)]).all()                             # NaN > 0 is false: ν_T = 1, the wT faces of the neutral layer are finite
    print("rest columns, %s: rel err uw %.3e vw %.3e wT %.3e" % ((tag,) + tuple(errs)))
    _record(tag, **dict(zip(FIELDS, errs)))


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
def test_flux_diagnoses_and_fused_step(ca, halo):
    """mpp_diagnose_flux, wm_diagnose_flux, wm_embedded_step and wm_embedded_step_flux on the 16 columns at rest"""
    import colnde
    from tests.test_gpu_wm_embed import DZ_BOUND
    rs = _embed_state(N)
    p = rs.p
    u, v, T, top, hb, ht = rs.u, rs.v, rs.T, rs.top, rs.halo_bottom, rs.halo_top
    halos = (hb, ht) if halo else None
    dz = W.LZ / NZ
    base_ref = R.diagnose_baseline_flux(u, v, T, top, dz, W.MPP, bool(ca), (hb, None) if halo else None)
    nn_ref = R.diagnose_NN_flux(p.cfg, p.weights_truth, u, v, T, top, W.LZ, W.MPP, bool(ca), halos)
    dz_ref = W.dz_fluxes(p.cfg, p.weights_truth, u, v, T, top, W.LZ)
    step_ref = O.modified_pacanowski_philander_step(u, v, T, DT, dz, convective_adjustment=bool(ca), halo_bottom=hb if halo else None, **W.MPP)
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        base = nde.mpp_diagnose_flux(u, v, T, top, dz, W.mpp_params(), ca, hb if halo else None)
        nn = nde.wm_diagnose_flux(p.weights_truth, u, v, T, top, W.LZ, W.mpp_params(), ca, halos)
        dz_s, st_s = nde.wm_embedded_step(p.weights_truth, u, v, T, top, W.LZ, DT, W.mpp_params(), ca, hb if halo else None)
        dz_f, st_f, fc_f = nde.wm_embedded_step_flux(p.weights_truth, u, v, T, top, W.LZ, DT, W.mpp_params(), ca, halos)
    _flux_check("mpp_diagnose_flux/%d/%d" % (ca, halo), base, base_ref, BASE_BOUND[ca], rs, ca)
    _flux_check("wm_diagnose_flux/%d/%d" % (ca, halo), nn, nn_ref, NN_BOUND[ca], rs, ca)
    for a, b in zip(tuple(dz_s) + tuple(st_s) + tuple(nn), tuple(dz_f) + tuple(st_f) + tuple(fc_f)):
        assert np.array_equal(a, b, equal_nan=True)                              # the fused call: the separate calls' bits, NaNs included
    for k, (g, r) in enumerate(zip(dz_s, dz_ref)):                               # the networks read the state alone: finite everywhere
        assert np.isfinite(g).all()
        assert np.abs(g - r).max() / np.abs(r).max() <= DZ_BOUND, FIELDS[k]
    errs = []
    for f, (g, w, tol) in enumerate(zip(st_s, step_ref, STEP_TOL)):
        assert np.array_equal(~np.isfinite(w).all(axis=1), rs.mask(2) & (f < 2 or not ca))
        ok = _same_non_finite(g, w, "step field %d" % f)
        errs.append(float(np.abs(g[ok] - w[ok]).max() / np.abs(w[ok]).max()))
        assert errs[-1] <= tol, (f, errs[-1])
    assert np.array_equal(st_s[2][:, 0], T[:, 0])
    _record("wm_embedded_step/%d/%d" % (ca, halo), **dict(zip(("u", "v", "T"), errs)))


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
def test_ensemble_embedding_row_k_is_the_single_model_call(ca, halo):
    """ColumnNDEEnsemble.wm_embedded, K = 3, every model on the columns at rest with its own weights and constants: the single-model call's bits,
    NaNs included"""
    import colnde
    from tests.test_gpu_wm_ens_embed import flat, model_params, single_model
    K = 3
    rs = _embed_state(N)
    p = rs.p
    w = np.stack([synthetic.perturb_weights(np.random.default_rng(100 + k), p.weights_truth, 0.05) for k in range(K)])
    st = [np.ascontiguousarray(np.stack([a] * K)) for a in (rs.u, rs.v, rs.T)]
    hb, ht = (np.ascontiguousarray(np.stack([h] * K)) if halo else None for h in (rs.halo_bottom, rs.halo_top))
    params = np.array([model_params(k) for k in range(K)], dtype=np.float32)
    with colnde.ColumnNDEEnsemble(p.cfg, 8, K) as ens:
        got = flat(ens.wm_embedded(w, st[0], st[1], st[2], rs.top, W.LZ, DT, params, ca, hb, ht))
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        for k in range(K):
            want = single_model(nde, w[k], rs.u, rs.v, rs.T, rs.top, rs.halo_bottom if halo else None, rs.halo_top if halo else None, params[k], ca, True, True)
            assert set(want) == set(got)
            for nm in want:
                assert np.array_equal(got[nm][k], want[nm], equal_nan=True), (k, nm)
                bad = ~np.isfinite(want[nm]).all(axis=1)
                assert not bad[~rs.mask(2)].any(), (k, nm)                       # non-finite on the neutral resting layer's columns only
            assert np.isnan(want["uw"][rs.mask(2)][:, 5:9]).all() and np.isnan(want["u_out"][rs.mask(2)]).all()


# ------------------------------------------------------------------------------------------------------------------ e. profile
@functools.lru_cache(maxsize=None)
def _profile_case():
    """K = 2 members; sol [K, 16, 5, 96]: frame 0 the columns at rest, frames 1..4 the float64 solve of the UNEDITED columns under the member's
    weights (sheared everywhere: the diagnosis takes any states, and no later frame drifts into float32 underflow of a decaying shear)"""
    from tests.test_gpu_wm_profile import PHYS
    K = 2
    p0 = synthetic.wind_mixing_problem(N, n_frames=FRAMES, weight_divisor=10)
    rs = RC.rest_state(p0)
    w = np.stack([synthetic.make_weights(synthetic._rng(11, k), p0.cfg, 10) for k in range(K)]).astype(np.float32)
    sol = np.stack([O.solve(p0.cfg, p0.x0, p0.bcs, w[k]) for k in range(K)]).astype(np.float32)
    sol[:, :, 0] = rs.p.x0
    truth = O.solve(p0.cfg, rs.p.x0, p0.bcs, p0.weights_truth).astype(np.float32)
    for a in (w, sol, truth):
        a.setflags(write=False)
    return rs, w, PHYS[:K], sol, truth


def test_profile_of_states_at_rest():
    """ColumnNDEEnsemble.profile: the stored Ri (no ε) is +Inf, −Inf and NaN exactly where the float64 restatement is, the finite faces are within
    RI_BOUND, an exact zero is an exact zero; the fluxes (ε inside) are finite and within FLUX_BOUND"""
    import colnde
    from tests import wm_profile_restatement as PR
    from tests.test_gpu_parity import _rel
    from tests.test_gpu_wm_profile import FLUX_BOUND, RI_BOUND
    rs, w, phys, sol, truth = _profile_case()
    p = rs.p
    with colnde.ColumnNDEEnsemble(p.cfg, N, 2, physics=phys) as ens:
        ens.set_problem(p.x0, p.bcs, truth)
        got = ens.profile(w, sol, losses=False)
    worst_f = worst_r = 0.0
    for k in range(2):
        c = PR.member_cfg(p.cfg, phys[k])
        for nm, r, g in zip(FIELDS, PR.fluxes(c, w[k], sol[k], p.bcs), (got.uw[k], got.vw[k], got.wT[k])):
            assert np.isfinite(r).all() and np.isfinite(g).all(), (k, nm)
            e = _rel(g[..., 1:NZ], r[..., 1:NZ])
            worst_f = max(worst_f, e)
            assert e < FLUX_BOUND, (k, nm, e)
        ri, rr = got.Ri[k], PR.local_richardson(p.cfg, sol[k])
        rr32 = PR.local_richardson(p.cfg, sol[k], np.float32)
        assert np.isnan(ri[..., 0]).all() and np.isnan(ri[..., NZ]).all()
        ri, rr, rr32 = ri[..., 1:NZ], rr[..., 1:NZ], rr32[..., 1:NZ]
        for f in (np.isposinf, np.isneginf, np.isnan, lambda a: a == 0):
            assert np.array_equal(f(rr), f(rr32)) and np.array_equal(f(ri), f(rr)), k
        assert np.isfinite(rr[:, 1:]).all()                                      # only frame 0 is at rest
        I = rr[:, 0]
        assert (int(np.isposinf(I).sum()), int(np.isneginf(I).sum()), int(np.isnan(I).sum()), int((I == 0).sum())) == (224, 4, 16, 4)
        assert np.array_equal(np.isnan(I).any(axis=1), rs.mask(2))
        ok = np.isfinite(rr) & (rr != 0)
        e = float(np.max(np.abs(ri[ok] - rr[ok]) / np.abs(rr[ok])))
        worst_r = max(worst_r, e)
        assert e < RI_BOUND, (k, e)
    print("rest columns, profile: flux rel %.3e, Ri rel %.3e" % (worst_f, worst_r))
    _record("profile", flux_rel=worst_f, ri_rel=worst_r)


# ------------------------------------------------------------------------------------------------------------------ f. pre-training
@functools.lru_cache(maxsize=None)
def _pretrain_samples():
    """16 samples whose profiles are the columns at rest, as tests/wm_pretrain_cases.samples builds a condition set's data: cfg, X [16, 96], B [16, 6],
    Y [3, 16, 33] (the fluxes of weights_truth plus noise, tests/pretrain_cases.fluxes) and W [2, P], different in every model and net"""
    from types import SimpleNamespace
    from tests import pretrain_cases as PC
    rs = RC.rest_state(synthetic.wind_mixing_problem(N, n_frames=2, weight_divisor=1.0))
    p = rs.p
    X, B = p.x0.copy(), p.bcs.copy()
    Y = np.stack(PC.fluxes(p, X.astype(np.float64), B.astype(np.float64))).astype(np.float32)
    theta, _ = PC._weights(p, 0, X.astype(np.float64), B.astype(np.float64))
    Wt = np.stack([theta, synthetic.perturb_weights(np.random.default_rng(501), theta, 0.1)]).astype(np.float32)
    for a in (X, B, Y, Wt):
        a.setflags(write=False)
    return SimpleNamespace(cond="mpp_zero_weights", cfg=p.cfg, X=X, B=B, Y=Y, W=Wt, n=N, K=2)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pretrain_pass_over_profiles_at_rest(k):
    """colnde_pretrain_flux_dev (pt_wm_face_const's fast_tanh at |y| ~ 1e15): one ADAM pass over the 16 samples against the float64 sequential loop,
    at the tolerances of tests/test_gpu_pretrain.py"""
    import colnde
    from types import SimpleNamespace
    from tests import pretrain_cases as PC
    from tests.test_gpu_pretrain import _check_pass, _dev_sample, _run
    d = _pretrain_samples()
    net = slice(k * d.cfg.net_size, (k + 1) * d.cfg.net_size)
    s = SimpleNamespace(case="rest-%s" % FIELDS[k], cfg=d.cfg, k=k, gs=1e-2, theta=d.W[0], X=d.X, B=d.B, Y=d.Y[k], net=net)
    ref = PC.sequential_pass(s, range(N))
    assert all(np.isfinite(a).all() for a in ref[:3]) and np.isfinite(ref[4]).all()
    with colnde.ColumnNDE(d.cfg, 1) as eng:
        got = _run(eng, s, _dev_sample(s), None)
    assert all(np.isfinite(a).all() for a in got[:3]) and np.isfinite(got[4])
    _check_pass(s, got, ref, "rest columns, pretrain %s" % FIELDS[k])


def test_ensemble_pretrain_pass_over_profiles_at_rest():
    """ColumnNDEEnsemble.pretrain_fluxes, K = 2, each model under its own constants: one pass of the six chains over the 16 samples against the float64
    sequential loop, at the tolerances of tests/test_gpu_wm_pretrain.py"""
    from tests import pretrain_cases as PC
    from tests import wm_pretrain_cases as WC
    from tests import test_gpu_wm_pretrain as T
    d = _pretrain_samples()
    etas = WC.ETAS[:2]
    with T._ens(d, physics=WC.PHYSICS[:2]) as ens:                              # (WC.chain gives model k the same row)
        theta, m, v, bt, loss = T._run(ens, d, d.W, etas, None)
    assert np.isfinite(theta).all() and np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(loss).all()
    for kk, j, c in WC.chains(d):
        ref = PC.sequential_pass(c, range(N), eta=float(etas[kk, j]))
        np.testing.assert_allclose(bt, ref[3], rtol=1e-15)
        e = WC.pass_errors(c, theta[kk][c.net], m[kk][c.net], v[kk][c.net], loss[kk, j], ref)
        print("rest columns, %s: %s" % (c.case, " ".join("%s %.2e" % kv for kv in e.items())))
        _record("pretrain_ens/%d/%s" % (kk, FIELDS[j]), **e)
        assert e["moved_least"] > 1e-3
        assert e["loss"] < T.TOL_LOSS
        assert e["theta"] < T.TOL_THETA and e["moved"] < T.TOL_MOVED, e
        assert e["m"] < T.TOL_M and e["v"] < T.TOL_V, e
