"""`colnde_ensemble_profile`: what NDE_profile (wind_mixing/src/training_postprocessing.jl:250-632) evaluates on the saved states of a solve, for all K
members of a wind-mixing ensemble in one launch (wm_profile_ens_kernel), and the Python layer on top of it.

Shapes: K = 3 members, 5 simulations, 7 frames (35 states per model: one full and one partial 32-state tile, tiles straddle simulations, a model's face
rows are 1,155 floats long so models 1 and 2 are misaligned) and 27 frames (135 states: two groups of four tiles).

Oracle parity.  The reference is float64 (tests/wm_profile_restatement.py) on the SAME float32 states the kernel reads, so input rounding is not counted.
Fluxes: relative L2 distance per net over the 31 interior faces of every state (the project's `_rel`, as tests/test_gpu_diagnostics.py holds colnde_flux);
Ri: the largest relative error of a single interior face (its values span 1e-7 .. 1e6).  The float32 restatement's own distance from float64 on these
states is 2.9e-7 (fluxes) and 3.7e-7 (Ri), measured on the CPU without the cast of the inputs; the bounds started at 10 x that (2.9e-6, 3.7e-6).
The first MI355X run (COLNDE_RECORD_ERRORS=1) recorded 2.9e-7 (fluxes; 1.3e-7 with the closure, 2.9e-7 without) and 3.1e-7 (Ri) at worst over the cases
below: FLUX_BOUND = 2.9e-6 stands (10 x the recorded error and 10 x the restatement's coincide), RI_BOUND was tightened from 3.7e-6 to 3.1e-6.  Both
numbers of each are in DESIGN §4q.
The boundary faces of the fluxes are boundary values, not network outputs: BC (- scaling(0)) is one float32 subtraction, and the diurnal top flux goes
through the solver's own hardware sine (absolute error <= 1e-6 on an amplitude |Q / (alpha g sigma_wT)| <= 3.1): held to 1e-5 absolute."""
import ctypes
import functools
import os

import numpy as np
import pytest

import colnde
from colnde import synthetic, wind_mixing
from oracle import nde_oracle as O
from tests import wm_profile_restatement as R
from tests.test_gpu_parity import SOL_ATOL, _record, _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N_COL = 3, 5
# (nu0, nu_minus, dRi, Ric, Pr): the first rows of tests/test_gpu_ensemble.py's PHYS
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2], [1e-3, 0.05, 1.3, 0.3, 1.0]], np.float32)
# (kappa = 0.1 as tests/test_oracle.py's conv_adj_branch: the explicit step of the solve stays stable)
BRANCH = {"closure": {}, "convadj": dict(modified_pacanowski_philander=False, zero_weights=False, convective_adjustment=True, kappa=0.1),
          "plain": dict(modified_pacanowski_philander=False, zero_weights=False)}
FLUX_BOUND = 2.9e-6          # 10 x the recorded 2.9e-7 (= 10 x the float32 restatement's own 2.9e-7)
RI_BOUND = 3.1e-6            # 10 x the recorded 3.1e-7 (started at 10 x the float32 restatement's own 3.7e-7)
FLUX_SINGLE_BOUND = 1e-6     # what tests/test_gpu_diagnostics.py holds colnde_flux to
BOUNDARY_ATOL = 1e-5
SC = (1.0, 1.0, 1.0, 5e-3, 5e-3, 5e-3)
NAMES = ("uw", "vw", "wT")


@functools.lru_cache(maxsize=None)
def _case(branch, diurnal, n_save):
    """the problem, the K weight vectors, the physics rows (None without the closure), the truth and the ensemble's own float32 solutions"""
    p = synthetic.wind_mixing_problem(N_COL, n_frames=n_save, weight_divisor=10, diurnal=diurnal, **BRANCH[branch])
    W = np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 10) for k in range(K)]).astype(np.float32)
    phys = PHYS if branch == "closure" else None
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    with colnde.ColumnNDEEnsemble(p.cfg, N_COL, K, physics=phys) as ens:
        ens.set_problem(p.x0, p.bcs, truth)
        sol = ens.forward(W)
    assert np.isfinite(sol).all()
    if branch == "convadj":
        # the solve keeps T stably stratified; the diagnosis takes any states: unstable stretches in every other simulation put kappa min(0, dT/dz) to work
        sol = sol.copy()
        sol[:, 1::2, :, 78:84] = sol[:, 1::2, :, 78:84][..., ::-1]
        assert (np.diff(sol[..., 64:], axis=-1) < 0).any()
    for a in (truth, sol):                                                             # shared among the tests: left unchanged
        a.setflags(write=False)
    return p, W, phys, truth, sol


def _ens(case, n_models=K, rows=None):
    p, W, phys, truth, sol = case
    ph = None if phys is None else (phys if rows is None else phys[rows])
    e = colnde.ColumnNDEEnsemble(p.cfg, N_COL, n_models, physics=ph)
    e.set_problem(p.x0, p.bcs, truth)
    return e


def _same(a, b):
    """bit equality, NaNs included"""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _hold_to_oracle(tag, case, got, rows):
    p, W, phys, truth, sol = case
    worst_f = worst_r = 0.0
    for k in range(K):
        c = R.member_cfg(p.cfg, None if rows is None else rows[k])
        ref = R.fluxes(c, W[k], sol[k], p.bcs)
        for nm, r, g in zip(NAMES, ref, (got.uw[k], got.vw[k], got.wT[k])):
            assert g.shape == (N_COL, p.cfg.n_save, 33) and np.isfinite(g).all()
            e = _rel(g[..., 1:32], r[..., 1:32])                                       # the 31 interior faces, all of them
            print("%s model %d %s: rel %.3g" % (tag, k, nm, e))
            worst_f = max(worst_f, e)
            assert e < FLUX_BOUND, (tag, k, nm, e)
            assert np.abs(g[..., [0, 32]] - r[..., [0, 32]]).max() <= BOUNDARY_ATOL, (tag, k, nm)
        if got.Ri is not None:
            ri, rr = got.Ri[k], R.local_richardson(p.cfg, sol[k])
            assert np.isnan(ri[..., 0]).all() and np.isnan(ri[..., 32]).all()        # 0 / 0 on the zero rows of D_face, as in the reference
            assert np.isfinite(rr[..., 1:32]).all() and np.isfinite(ri[..., 1:32]).all()
            e = float(np.max(np.abs(ri[..., 1:32] - rr[..., 1:32]) / np.abs(rr[..., 1:32])))
            print("%s model %d Ri: rel %.3g" % (tag, k, e))
            worst_r = max(worst_r, e)
            assert e < RI_BOUND, (tag, k, e)
    _record("wm_profile/" + tag, flux_rel=worst_f, ri_rel=worst_r)


@pytest.mark.parametrize("branch,diurnal,n_save", [(b, d, 7) for b in BRANCH for d in (False, True)] + [("closure", True, 27), ("convadj", False, 27)])
def test_oracle_parity(branch, diurnal, n_save):
    case = _case(branch, diurnal, n_save)
    with _ens(case) as ens:
        assert "wm_profile=f32" in ens.describe()
        got = ens.profile(case[1], case[4])
    _hold_to_oracle("%s/diurnal%d/%d" % (branch, diurnal, n_save), case, got, case[2])
    ref_l = np.stack([O.loss_per_tstep(case[0].cfg, case[4][k], case[3]) for k in range(K)])
    assert got.losses.shape == (K, N_COL, 6, n_save)
    np.testing.assert_allclose(got.losses, ref_l, rtol=2e-5, atol=1e-12)                  # (its bits are held below; this is the layout)


@pytest.mark.parametrize("diurnal", [False, True])
def test_networks_only_rows(diurnal):
    """physics rows with nu0 = nu_minus = 0 for this call only: the *_NN_only fluxes (constants_NN_only, :286, :474-495); the handle keeps its own"""
    case = _case("closure", diurnal, 7)
    rows = PHYS.copy()
    rows[:, :2] = 0.0
    with _ens(case) as ens:
        own = ens.profile(case[1], case[4], Ri=False, losses=False)
        got = ens.profile(case[1], case[4], physics=rows, Ri=False, losses=False)
        again = ens.profile(case[1], case[4], Ri=False, losses=False)
    assert got.Ri is None and got.losses is None
    _hold_to_oracle("nn_only/diurnal%d" % diurnal, case, got, rows)
    assert all(_same(getattr(own, nm), getattr(again, nm)) and not _same(getattr(own, nm), getattr(got, nm)) for nm in NAMES)


@pytest.mark.parametrize("branch,diurnal", [("closure", True), ("convadj", False), ("plain", False)])
def test_cross_check_against_single_handle_flux(branch, diurnal):
    """row k, frame n against ColumnNDE.flux(sol[k][:, n], W[k], bcs, t_n) of a single handle: within the sum of the two bounds"""
    case = _case(branch, diurnal, 7)
    p, W, phys, truth, sol = case
    with _ens(case) as ens:
        got = ens.profile(W, sol, Ri=False, losses=False)
    for k in range(K):
        with colnde.ColumnNDE(R.member_cfg(p.cfg, None if phys is None else phys[k]), N_COL) as one:
            ref = np.stack([one.flux(np.ascontiguousarray(sol[k][:, n]), W[k], p.bcs, float(np.float32(p.cfg.save_times[n]))) for n in range(7)], axis=1)
        for q, nm in enumerate(NAMES):
            e = _rel(getattr(got, nm)[k][..., 1:32], ref[:, :, q, 1:32].astype(np.float64))
            assert e < FLUX_BOUND + FLUX_SINGLE_BOUND, (k, nm, e)
            assert np.abs(getattr(got, nm)[k][..., [0, 32]] - ref[:, :, q][..., [0, 32]]).max() <= BOUNDARY_ATOL


@pytest.mark.parametrize("n_save", [7, 27])
def test_row_k_is_the_k1_ensemble(n_save):
    case = _case("closure", True, n_save)
    p, W, phys, truth, sol = case
    with _ens(case) as ens:
        got = ens.profile(W, sol)
    for k in range(K):
        with _ens(case, 1, [k]) as one:
            r = one.profile(W[k:k + 1], sol[k:k + 1])
        for nm in NAMES + ("Ri", "losses"):
            assert _same(getattr(got, nm)[k], getattr(r, nm)[0]), (k, nm)


@pytest.mark.parametrize("n_save", [7, 27])
def test_grid_cap_gives_the_same_bits(monkeypatch, n_save):
    """COLNDE_WM_PROFILE_GRID = 1, 2 and unset (read per call): a workgroup walks several models and re-copies the weight image at the boundaries"""
    case = _case("closure", True, n_save)
    res = []
    with _ens(case) as ens:
        for grid in (None, "1", "2"):
            if grid is None:
                monkeypatch.delenv("COLNDE_WM_PROFILE_GRID", raising=False)
            else:
                monkeypatch.setenv("COLNDE_WM_PROFILE_GRID", grid)
            res.append(ens.profile(case[1], case[4], losses=False))
            assert ("COLNDE_WM_PROFILE_GRID=%s" % grid in ens.describe()) == (grid is not None)
    for other in res[1:]:
        for nm in NAMES + ("Ri",):
            assert _same(getattr(res[0], nm), getattr(other, nm)), nm


def test_losses_are_the_single_handles_bits():
    """losses[k] = a single handle's loss_per_tstep for ens.forward's solution (which is the single handle's own solution, bit for bit)"""
    case = _case("closure", False, 7)
    p, W, phys, truth, sol = case
    with _ens(case) as ens:
        got = ens.profile(W, sol, flux=False, Ri=False)
    assert got.uw is None and got.Ri is None
    for k in range(K):
        with colnde.ColumnNDE(R.member_cfg(p.cfg, phys[k]), N_COL) as one:
            one.set_problem(p.x0, p.bcs, truth)
            assert _same(one.forward(W[k]), sol[k])
            assert _same(one.loss_per_tstep(W[k]), got.losses[k]), k


def test_single_handle_loss_per_tstep_keeps_the_parents_bits():
    """colnde_loss_per_tstep on a single handle against the bits of the commit before its kernel took a model index (tests/golden/)"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "loss_per_tstep_parent.npz"))
    p = synthetic.wind_mixing_problem(N_COL, n_frames=7, weight_divisor=10)
    with colnde.ColumnNDE(p.cfg, N_COL) as one:
        one.set_problem(p.x0, p.bcs, gold["truth"])
        out = one.loss_per_tstep(p.weights)
    assert _same(out, gold["loss_per_tstep"])


def test_sentinel_tail_and_device_tensors():
    import torch
    case = _case("closure", True, 7)
    p, W, phys, truth, sol = case
    n = K * N_COL * 7 * 33
    dev = torch.device("cuda", 0)
    with _ens(case) as ens:
        ref = ens.profile(W, sol)
        bufs = [torch.full((n + 64,), -7.5, dtype=torch.float32, device=dev) for _ in range(4)]
        lbuf = torch.full((K * N_COL * 6 * 7 + 64,), -7.5, dtype=torch.float32, device=dev)
        Wd, sd = torch.from_numpy(W.copy()).to(dev), torch.from_numpy(sol.copy()).to(dev)
        ens.use_torch_stream()
        colnde._lib.check(ens._L.colnde_ensemble_profile_dev(ens._h, Wd.data_ptr(), sd.data_ptr(), None, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                             bufs[3].data_ptr(), lbuf.data_ptr()))
        torch.cuda.synchronize()
        t = ens.profile(Wd, sd)                                                        # the wrapper on device tensors
        assert all(torch.is_tensor(x) for x in t)
    for b, nm in zip(bufs, NAMES + ("Ri",)):
        h = b.cpu().numpy()
        assert (h[n:] == -7.5).all(), nm                                               # nothing past the end
        assert _same(h[:n].reshape(K, N_COL, 7, 33), getattr(ref, nm)) and _same(getattr(t, nm).cpu().numpy(), getattr(ref, nm)), nm
    h = lbuf.cpu().numpy()
    assert (h[K * N_COL * 42:] == -7.5).all() and _same(h[:K * N_COL * 42].reshape(K, N_COL, 6, 7), ref.losses)


def test_a_nan_model_leaves_the_other_rows():
    case = _case("closure", False, 7)
    p, W, phys, truth, sol = case
    bad = sol.copy()
    bad[1] = np.nan
    with _ens(case) as ens:
        ref = ens.profile(W, sol)
        got = ens.profile(W, bad)
    for nm in NAMES + ("Ri", "losses"):
        g, r = getattr(got, nm), getattr(ref, nm)
        assert _same(g[0], r[0]) and _same(g[2], r[2]), nm
        inner = g[1][..., 1:32] if nm != "losses" else g[1]
        assert not np.isfinite(inner).any(), nm                                        # (the boundary faces of the fluxes are boundary values)


def _call(h, dev, weights, sol, physics, uw, vw, wT, Ri, losses):
    L = colnde._lib.lib()
    fn = L.colnde_ensemble_profile_dev if dev else L.colnde_ensemble_profile
    rc = fn(h, weights, sol, physics, uw, vw, wT, Ri, losses)
    return rc, L.colnde_last_error().decode()


def test_refusals_name_their_reason():
    import torch
    case = _case("closure", False, 7)
    p, W, phys, truth, sol = case
    dev = torch.device("cuda", 0)
    big = torch.zeros(K * N_COL * 7 * 96 + 16, dtype=torch.float32, device=dev)
    A = big.data_ptr()
    assert A % 16 == 0
    z = np.zeros(K * N_COL * 7 * 96, np.float32)
    H = z.ctypes.data
    # the handles that are refused
    fc = synthetic.free_convection_problem(9, n_save=5)
    cv = synthetic.free_convection_conv_problem(9, 3, n_save=5)
    with colnde.FreeConvectionEnsemble(fc.cfg, 9, 2) as e:
        rc, msg = _call(e._h, True, A, A, None, A, A, A, A, None)
        assert rc and "free-convection models" in msg and "colnde_ensemble_profile_dev" in msg
    with colnde.FreeConvectionEnsemble(cv.cfg, 9, 2, conv=3) as e:
        rc, msg = _call(e._h, False, H, H, None, H, H, H, H, None)
        assert rc and "convolutional first layer" in msg and "colnde_ensemble_profile" in msg
    with colnde.ClosureColumns(p.cfg, N_COL, 2) as e:
        rc, msg = _call(e._h, True, A, A, None, A, A, A, A, None)
        assert rc and "closure handle" in msg
    with colnde.ColumnNDE(p.cfg, N_COL) as e:
        rc, msg = _call(e._h, True, A, A, None, A, A, A, A, None)
        assert rc and "single-model handle" in msg
    with colnde.ColumnNDEEnsemble(p.cfg, N_COL, K, physics=phys) as e:
        for d, P in ((True, A), (False, H)):
            rc, msg = _call(e._h, d, P, P, None, P, P, P, P, None)
            assert rc and "colnde_set_problem has not been called" in msg, msg
        e.set_problem(p.x0, p.bcs)                                                     # no truth
        for d, P in ((True, A), (False, H)):
            rc, msg = _call(e._h, d, P, P, None, P, P, P, P, P)
            assert rc and "losses need truth" in msg, msg
            rc, msg = _call(e._h, d, None, P, None, P, P, P, P, None)
            assert rc and "null pointer argument" in msg, msg
            rc, msg = _call(e._h, d, P, None, None, P, P, P, P, None)
            assert rc and "null pointer argument" in msg, msg
            rc, msg = _call(e._h, d, P, P, None, P, None, P, P, None)
            assert rc and "one output group" in msg and "2 of 3 given" in msg, msg
            rc, msg = _call(e._h, d, P, P, None, None, None, None, None, None)
            assert rc and "no outputs" in msg, msg
            bad = (ctypes.c_float * 15)(*([1e-4, 0.1, 1.0, 0.25, 1.0] * 2 + [1e-4, 0.1, 0.0, 0.25, 1.0]))
            rc, msg = _call(e._h, d, P, P, bad, P, P, P, P, None)
            assert rc and "physics[2]: dRi = 0" in msg, msg
            bad[12] = float("nan")
            rc, msg = _call(e._h, d, P, P, bad, P, P, P, P, None)
            assert rc and "physics[2][2]" in msg and "not finite" in msg, msg
        for i in (1, 3, 4, 5, 6):                                                      # sol and each face output's base pointer, 4 bytes off
            args = [A, A, None, A, A, A, A, None]
            args[i] = A + 4
            rc, msg = _call(e._h, True, *args)
            assert rc and "16-byte aligned" in msg, (i, msg)
    with colnde.ColumnNDEEnsemble(p.cfg.with_(modified_pacanowski_philander=False, zero_weights=False), N_COL, K) as e:
        e.set_problem(p.x0, p.bcs)
        ok = (ctypes.c_float * 15)(*([1e-4, 0.1, 1.0, 0.25, 1.0] * 3))
        rc, msg = _call(e._h, True, A, A, ok, A, A, A, A, None)
        assert rc and "needs modified_pacanowski_philander = 1" in msg, msg


def _trajectories(case, mode, Wm):
    """the solve `ensemble_NDE_profile` runs in each mode, repeated here: its trajectories, bit for bit (the solves are deterministic)"""
    p, W, phys, truth, sol = case
    if mode == "ensemble":
        with _ens(case) as e:
            return e.forward(Wm)
    out = []
    for k in range(K):
        c = R.member_cfg(p.cfg, None if phys is None else phys[k]).with_(inplace_variant=True)
        with colnde.ColumnNDE(c, N_COL) as one:
            one.set_problem(p.x0, p.bcs, truth)
            out.append(one.forward(Wm[k]))
    return np.stack(out)


@pytest.mark.parametrize("branch", ["closure", "plain"])
def test_ensemble_NDE_profile_both_solves(branch):
    """wind_mixing.ensemble_NDE_profile with both solve modes against the float64 restatement on the trajectories each mode solves; the two modes'
    trajectories differ by less than SOL_ATOL (no diurnal forcing, no convective adjustment: eps in the closure's Ri is the only difference).
    Tolerances per key, from the formats: profiles, depths and times are float32 unscalings (4e-6 of the key's scale plus 4e-6 of the value, as in
    tests/test_wm_profile_host.py); the flux keys FLUX_BOUND in L2 plus four float32 roundings per element at the scale of the values before the subtraction; test_Ri RI_BOUND per
    element, truth_Ri 4e-6 (NumPy float32); the loss keys the project's LOSS_RTOL."""
    from tests.test_gpu_parity import LOSS_RTOL
    case = _case(branch, False, 7)
    p, W, phys, truth, sol = case
    M = "_modified_pacanowski_philander"
    wm = wind_mixing.WindMixingNDE(p.cfg, p.x0, p.bcs, truth)
    try:
        outs = {s: wind_mixing.ensemble_NDE_profile(wm, W, phys, SC, solve=s) for s in (("ensemble", "mutating") if branch == "closure" else ("ensemble",))}
        one = None
        if branch == "closure":                                                        # NDE_profile: K = 1, solve = "mutating", the problem's constants
            one = wind_mixing.NDE_profile(wm, W[0], SC)
            same = wind_mixing.ensemble_NDE_profile(wm, W[:1], None, SC, solve="mutating")[0]
        else:
            with pytest.raises(ValueError, match="hard-wires the Pacanowski-Philander closure"):
                wind_mixing.ensemble_NDE_profile(wm, W, phys, SC, solve="mutating")
    finally:
        wm.close()
    traj = {s: _trajectories(case, s, W) for s in outs}
    traj0 = {s: _trajectories(case, s, np.zeros_like(W)) for s in outs} if branch == "closure" else {s: [None] * K for s in outs}
    assert _same(traj["ensemble"], sol)
    if one is not None:
        d = float(np.abs(traj["ensemble"].astype(np.float64) - traj["mutating"]).max())
        print("ensemble vs mutating trajectories: %.3g" % d)
        assert d < SOL_ATOL
        assert set(one) == set(same)
        assert all(_same(np.asarray(one[key], np.float32), np.asarray(same[key], np.float32)) for key in one if one[key] is not None and key != "train_parameters")
    for s, res in outs.items():
        for k in range(K):
            got = res[k]
            assert _same(got["test_T"], np.swapaxes(np.float32(p.cfg.sigma[2]) * traj[s][k][..., 64:] + np.float32(p.cfg.mu[2]), 1, 2))
            ref = R.nde_profile(p.cfg, W[k], None if phys is None else phys[k], traj[s][k], traj0[s][k], p.bcs, truth, SC)
            assert set(got) == set(ref)
            for key, r in ref.items():
                if r is None or isinstance(r, dict):
                    continue
                g, r = np.asarray(got[key], np.float64), np.asarray(r, np.float64)
                fin = np.isfinite(r)
                assert g.shape == r.shape and np.array_equal(np.isfinite(g), fin), (s, k, key)
                err = np.abs(g - r)[fin]
                if key.startswith("test_Ri") or key == "truth_Ri":
                    ok = (err <= (RI_BOUND if key.startswith("test") else 4e-6) * np.abs(r[fin])).all()
                elif "loss" in key:
                    ok = (err <= LOSS_RTOL * np.abs(r[fin]) + 1e-30).all()
                elif key[:7] in ("test_uw", "test_vw", "test_wT"):
                    # the kernel's share in L2 on the scaled fluxes, and four float32 roundings per element at the scale of the unscaled values
                    # BEFORE the subtraction of test_uw[1, 1] (sigma y, + mu, the same two in the subtrahend): the difference cancels, its error does not
                    q = NAMES.index(key[5:7])
                    U = np.abs(r[fin]).max() + abs(p.cfg.mu[3 + q])
                    # (the bottom flux of these problems is zero, so test_uw[1, 1] = mu and the key is sigma y itself)
                    ok = np.linalg.norm(err) <= FLUX_BOUND * np.linalg.norm(r[fin]) + np.sqrt(err.size) * 4 * 2.0 ** -24 * U
                else:
                    ok = (err <= 4e-6 * np.abs(r[fin]).max() + 4e-6 * np.abs(r[fin])).all()
                assert ok, (s, k, key, float(err.max()))
            assert (M in "".join(got)) == (branch == "closure")


