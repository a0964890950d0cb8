"""Free-convection ensembles on the GPU (colnde_create_fc_ensemble): K networks of the fc32 shape on the same simulations, the model index in
blockIdx.y of the 16-column fc32 kernels.

Row k of every ensemble result must hold the bits a single `colnde.ColumnNDE` handle computes for model k's weights: the same kernels run with the
model's buffers at a fixed stride, tile16's dW GEMM keeps the slice count (hence the reduction order) of a single handle, and the models march
through the time segments together.  On top: the float64 oracle, the training loop, and the two judging kernels (column loss, causal penalty).
Inputs follow tests/test_gpu_fc.py (5 save points, 2 sub-steps, t_end = 0.01): every case takes a few seconds."""
import functools

import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.flux_compat import ADAM
from colnde.free_convection import (FreeConvectionNDE, compute_nde_solution_history, nde_loss_history, train_neural_differential_equation,
                                    train_neural_differential_equation_ensemble)
from colnde.nde import ColumnNDE
from oracle import nde_oracle as O
from oracle import training_oracle as TO
from tests.test_gpu_parity import FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL, _rel

pytestmark = pytest.mark.gpu

MA = ["bf16x3_exact", "f32_mfma"]
SC = [0, 0, 1, 0, 0, 0]
SIZES = [(32, 9), (32, 20), (64, 5)]          # one ragged tile; two tiles, the second ragged; 64 levels


def _weights(cfg, K, seed=11):
    return np.stack([synthetic.make_weights(synthetic._rng(seed, k), cfg, 1e2) for k in range(K)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problem(Nz, n, kind="fc"):
    """(cfg, x0, bcs, truth) — kind: fc | ca_rk4 | ca_rkc2 (the latter two with an inverted layer in two columns: the switch tape is live)."""
    if kind == "fc":
        p = synthetic.free_convection_problem(n, Nz=Nz, n_save=5, substeps=2, t_end=0.01)
        cfg = p.cfg
    elif kind == "ca_rk4":
        p = synthetic.free_convection_problem(n, Nz=Nz, n_save=5, substeps=20 * (Nz // 32) ** 2, convective_adjustment=True, t_end=0.01)
        cfg = p.cfg
    else:
        p = synthetic.free_convection_problem(n, Nz=Nz, n_save=9, substeps=2, convective_adjustment=True, t_end=0.06)
        cfg = p.cfg.with_(stepper="rkc2")
    x0 = p.x0.copy()
    if kind != "fc":
        x0[:2, Nz // 2:Nz // 2 + 6] = x0[:2, Nz // 2:Nz // 2 + 6][:, ::-1]
    truth = O.solve(cfg, x0, p.bcs, p.weights_truth).astype(np.float32)
    for a in (x0, p.bcs, truth):
        a.setflags(write=False)                                       # shared among the tests: left unchanged
    return cfg, x0, p.bcs, truth


def _single(cfg, x0, bcs, truth, w, ma):
    """(sol, [grad; terms; total; 0], [terms; total], the same row from a second loss_grad) of one ColumnNDE built in this process."""
    with ColumnNDE(cfg, x0.shape[0], matrix_arithmetic=ma) as h:
        h.set_problem(x0, bcs, truth)
        sol = h.forward(w)
        lt, lterms = h.loss(w, SC)
        total, terms, g = h.loss_grad(w, SC)
        total2, terms2, g2 = h.loss_grad(w, SC)
        row = lambda t, te, gr: np.concatenate([gr, te, [t, 0.0]]).astype(np.float32)
        return sol, row(total, terms, g), np.concatenate([lterms, [lt]]).astype(np.float32), row(total2, terms2, g2), h.describe()


def _ensemble(cfg, x0, bcs, truth, W, ma):
    with colnde.FreeConvectionEnsemble(cfg, x0.shape[0], W.shape[0], matrix_arithmetic=ma) as e:
        e.set_problem(x0, bcs, truth)
        sol = e.forward(W)
        loss8 = e.loss(W, SC)
        res = e.loss_grad(W, SC)
        res2 = e.loss_grad(W, SC)
        desc = e.describe()
    return sol, res, loss8, res2, desc


def _assert_rows_are_the_single_handles_bits(prob, W, ma, idx, ens=None):
    cfg, x0, bcs, truth = prob
    sol, res, loss8, res2, desc = ens if ens is not None else _ensemble(cfg, x0, bcs, truth, W, ma)
    assert sol.shape == (W.shape[0], x0.shape[0], cfg.n_save, cfg.Nz) and res.shape == (W.shape[0], cfg.n_params + 8)
    for k in idx:
        s1, r1, l1, r1b, d1 = _single(cfg, x0, bcs, truth, W[k], ma)
        assert np.array_equal(sol[k], s1), k
        assert np.array_equal(loss8[k, :7], l1), k
        assert np.array_equal(res[k], r1), (k, np.abs(res[k] - r1).max())
        assert np.array_equal(res2[k], r1b) and np.array_equal(res2[k], res[k]), k
    return desc, d1


# ---- 1. rows are the single handle's bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("Nz,n", SIZES)
def test_rows_are_the_single_handles_bits(Nz, n, ma):
    prob = _problem(Nz, n)
    desc, d1 = _assert_rows_are_the_single_handles_bits(prob, _weights(prob[0], 3), ma, range(3))
    assert "engine=fc32" in desc and "models=3" in desc and "tape_bytes_per_model=" in desc and "time_segments=0" in desc and "tile_width=16" in desc
    assert "dw_slices=" + d1.split("dw_slices=")[1].split()[0] in desc                 # the slice count a single handle of this size plans


# ---- 2, 3. ConvectiveAdjustmentNDE: the per-model switch tape, RK4 and RKC2 (shared coefficient table) ---------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("kind", ["ca_rk4", "ca_rkc2"])
def test_convective_adjustment_nde_bit_for_bit(kind, ma):
    prob = _problem(32, 9, kind)
    if kind == "ca_rkc2":
        assert colnde.rkc_stages(prob[0]) >= 4
    desc, _ = _assert_rows_are_the_single_handles_bits(prob, _weights(prob[0], 3, seed=3), ma, range(3))
    assert ("stepper=rkc2" in desc) == (kind == "ca_rkc2")


# ---- 4. time segments: all models march through them together, lambda carried per model ---------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
def test_time_segments_bit_for_bit(ma, monkeypatch):
    monkeypatch.setenv("COLNDE_FC_SEG", "2")                            # before both sides are created: 4 save intervals -> 2 segments
    prob = _problem(32, 20)
    desc, d1 = _assert_rows_are_the_single_handles_bits(prob, _weights(prob[0], 3, seed=4), ma, range(3))
    assert "time_segments=2" in desc and "time_segments=2" in d1


# ---- 5. position and isolation: more workgroups than CUs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
def test_position_and_isolation(ma):
    K = 300
    prob = _problem(32, 9)
    cfg, x0, bcs, truth = prob
    W = _weights(cfg, K, seed=5)
    base = _ensemble(cfg, x0, bcs, truth, W, ma)
    _assert_rows_are_the_single_handles_bits(prob, W, ma, [0, 1, K // 2, K - 1], ens=base)
    j = K // 3
    Wn = W.copy()
    Wn[j, -1] = np.nan                                               # the last output bias (relu's fmax would swallow a NaN of the hidden layers)
    nan = _ensemble(cfg, x0, bcs, truth, Wn, ma)
    n = cfg.n_params
    others = np.arange(K) != j
    assert not np.isfinite(nan[1][j, n + 6]) and not np.isfinite(nan[0][j]).all()
    assert np.isfinite(nan[1][others]).all() and np.isfinite(nan[0][others]).all()
    assert np.array_equal(nan[1][others], base[1][others]) and np.array_equal(nan[0][others], base[0][others])
    assert np.array_equal(nan[2][others], base[2][others])


# ---- 6. against the float64 oracle ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_rows(Nz, n):
    cfg, x0, bcs, truth = _problem(Nz, n)
    W = _weights(cfg, 3)
    return W, [O.loss_and_grad(cfg, x0, bcs, W[k], truth, np.array(SC, np.float64)) for k in range(3)]


@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("Nz,n", [(32, 9), (64, 5)])
def test_rows_against_the_float64_oracle(Nz, n, ma):
    cfg, x0, bcs, truth = _problem(Nz, n)
    W, ref = _oracle_rows(Nz, n)
    sol, res, loss8, _, _ = _ensemble(cfg, x0, bcs, truth, W, ma)
    P = cfg.n_params
    for k, (tot, terms, g, sol_o) in enumerate(ref):
        assert np.abs(sol[k] - sol_o).max() < FC_SOL_ATOL, k
        assert np.isclose(res[k, P + 6], tot, rtol=FC_LOSS_RTOL) and np.isclose(loss8[k, 6], tot, rtol=FC_LOSS_RTOL), k
        assert _rel(res[k, :P], g) < FC_GRAD_REL, k
    assert not np.array_equal(res[0], res[1]) and not np.array_equal(sol[0], sol[1])          # different weights, different rows


# ---- 7. the training loop -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _training_problem():
    p = synthetic.free_convection_problem(6, Nz=32, n_save=9, substeps=4, t_end=0.0625)
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    return p, truth


@pytest.mark.parametrize("ma", MA)
def test_training_loop_follows_the_float64_loop(ma):
    p, truth = _training_problem()
    K, epochs = 3, 6
    etas = (1e-3, 5e-4, 2e-3)
    W = _weights(p.cfg, K, seed=7)
    theta, hist = train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, p.cfg, W, etas, epochs, matrix_arithmetic=ma)
    assert theta.shape == W.shape and hist.shape == (epochs, K)
    for k in range(K):
        theta_o, hist_o = TO.train_neural_differential_equation(p.cfg, p.x0, p.bcs, truth, W[k], etas[k], epochs)
        e_loss = np.abs(hist[:, k] / np.array(hist_o) - 1).max()
        e_theta = _rel(theta[k], theta_o)
        print("training model %d: loss sequence rel %.3e, theta rel L2 %.3e" % (k, e_loss, e_theta))
        assert e_loss < 3e-3, (k, hist[:, k], hist_o)                   # test_flux_train_trajectory_matches_the_float64_loop's tolerances
        assert e_theta < 2e-3, (k, e_theta)
        assert np.abs(theta[k] - W[k]).max() > 0.5 * etas[k]


# ---- 8. column loss -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz,n", [(32, 9), (64, 5)])
def test_column_loss(Nz, n):
    import torch
    cfg, x0, bcs, truth = _problem(Nz, n)
    W = _weights(cfg, 3)
    with colnde.FreeConvectionEnsemble(cfg, n, 3) as e:
        e.set_problem(x0, bcs, truth)
        sol = e.forward(torch.from_numpy(W).cuda())
        cl = e.column_loss(sol)
        cl2 = e.column_loss(sol)
        cl_np = e.column_loss(sol.cpu().numpy())
        loss8 = e.loss(W, SC)
    assert cl.shape == (3, n, cfg.n_save)
    a = cl.cpu().numpy()
    assert np.array_equal(a, cl2.cpu().numpy()) and np.array_equal(a, cl_np)          # fixed-order sums
    ref = ((sol.cpu().numpy().astype(np.float64) - truth.astype(np.float64)[None]) ** 2).mean(axis=3)
    err = np.abs(a - ref).max() / ref.max()
    print("column loss: worst error %.3e of the largest entry" % err)
    np.testing.assert_allclose(a, ref, rtol=1e-5, atol=0.0)                          # relative 1e-5 > Nz 2^-24 (a 64-term f32 mean); save point 0 is exactly 0
    np.testing.assert_allclose(a.astype(np.float64).mean(axis=(1, 2)), loss8[:, 6], rtol=1e-5)


def test_history_functions_are_one_forward_call(monkeypatch):
    """compute_nde_solution_history / nde_loss_history (free_convection/src/testing.jl): E networks, one ensemble, unscaled solutions."""
    cfg, x0, bcs, truth = _problem(32, 9)
    W = _weights(cfg, 4, seed=9)
    hist = compute_nde_solution_history(x0, bcs, cfg, W)
    assert hist.shape == (4, 9, 32, cfg.n_save)
    with ColumnNDE(cfg, 9) as h:
        h.set_problem(x0, bcs, truth)
        s2 = h.forward(W[2])
    assert np.array_equal(hist[2], np.transpose(cfg.sigma[2] * s2 + cfg.mu[2], (0, 2, 1)))
    per_epoch, per_t = nde_loss_history(x0, bcs, truth, cfg, W)
    assert per_epoch.shape == (4, 9) and per_t.shape == (4, 9, cfg.n_save)
    ref = ((s2.astype(np.float64) - truth) ** 2).mean(axis=2)
    np.testing.assert_allclose(per_t[2], ref, rtol=1e-5, atol=0.0)
    np.testing.assert_allclose(per_epoch[2], ref.mean(axis=1), rtol=1e-5)


# ---- 9. causal penalty --------------------------------------------------------------------------------------------------------------------------------
def _w1_mask(cfg):
    """Boolean [n_params]: the entries W1[r, q], r < q, of the first Dense weight (4Nz x Nz, column-major: W1[r, q] at q * 4Nz + r)."""
    Nz, H = cfg.Nz, 4 * cfg.Nz
    m = np.zeros(cfg.n_params, bool)
    r, q = np.meshgrid(np.arange(H), np.arange(Nz), indexing="ij")
    m[(q * H + r)[r < q]] = True
    return m


@pytest.mark.parametrize("Nz,n", [(32, 9), (64, 5)])
def test_causal_penalty(Nz, n):
    import torch
    cfg, x0, bcs, truth = _problem(Nz, n)
    P = cfg.n_params
    W = _weights(cfg, 3)
    c = np.array([0.0, 1.0, 0.5], np.float32)
    mask = _w1_mask(cfg)
    n_mask = int(mask.sum())
    assert n_mask == Nz * (Nz - 1) // 2
    with colnde.FreeConvectionEnsemble(cfg, n, 3) as e:
        e.set_problem(x0, bcs, truth)
        base = e.loss_grad(W, SC)
        out = e.causal_penalty(W, c, base)                                            # NumPy in, NumPy out
        t = torch.from_numpy(base).cuda()
        assert e.causal_penalty(torch.from_numpy(W).cuda(), torch.from_numpy(c).cuda(), t) is t       # device tensors: in place
        assert np.array_equal(t.cpu().numpy(), out)
        zero = e.causal_penalty(W, c, np.zeros_like(base))                            # on a zero buffer the increments stand alone
    assert np.array_equal(out[0], base[0])                                            # c = 0: row 0 is bit-unchanged
    tol = n_mask * 2.0 ** -24                                                         # worst case of an f32 sum of n_mask positive terms
    assert abs(tol - (3e-5 if Nz == 32 else 1.2e-4)) < 0.05 * tol
    for k in (1, 2):
        w = W[k].astype(np.float64)
        pen = float(c[k]) * float((w[mask] ** 2).sum())
        inc = float(zero[k, P + 6])
        print("causal penalty model %d: increment %.9e, float64 %.9e, rel %.3e (tolerance %.3e)" % (k, inc, pen, abs(inc / pen - 1), tol))
        assert abs(inc - pen) <= tol * pen
        # added to the total of the row: the f32 sum of the two, within an ulp of it
        assert abs(float(out[k, P + 6]) - (float(base[k, P + 6]) + inc)) <= np.spacing(np.float32(out[k, P + 6]))
        # gradient entries: the f32 value of g + 2 c W1 within 2 ulp (contraction to an FMA allowed)
        want = (base[k, :P].astype(np.float64) + 2.0 * float(c[k]) * w)[mask]
        got = out[k, :P][mask]
        assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all()
        assert not np.array_equal(got, base[k, :P][mask])
        # nothing outside the strict upper triangle of W1 changes a bit (the total aside)
        keep = np.ones(P + 8, bool)
        keep[:P][mask] = False
        keep[P + 6] = False
        assert np.array_equal(out[k][keep], base[k][keep])
    assert not zero[0].any()


def test_causal_penalty_in_the_training_loop():
    """One epoch of the ensemble loop with a coefficient, K = 1, against the host loop of FreeConvectionNDE(causal_penalty=...)."""
    p, truth = _training_problem()
    mask = _w1_mask(p.cfg)

    def penalty(th):
        g = np.zeros_like(th)
        g[mask] = 2.0 * th[mask]
        return float((th[mask].astype(np.float64) ** 2).sum()), g

    W = _weights(p.cfg, 1, seed=8)
    theta, hist = train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, p.cfg, W, [1e-3], 1, causal_coeff=[1.0])
    nde = FreeConvectionNDE(p.cfg, p.x0, p.bcs, truth, causal_penalty=penalty)
    try:
        theta_h, hist_h = train_neural_differential_equation(nde, W[0], ADAM(1e-3), 1)
        plain = nde.engine.loss(W[0], SC)[0]
    finally:
        nde.close()
    assert hist.shape == (1, 1) and hist_h[0] > plain                     # the history holds the penalty, as nde_loss returns it
    assert abs(hist[0, 0] / hist_h[0] - 1) < 3e-3
    assert _rel(theta[0], theta_h) < 2e-3
    assert np.abs(theta[0] - W[0]).max() > 0.5e-3


# ---- 10. refusals on the GPU --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu():
    cfg, x0, bcs, truth = _problem(32, 9)
    L = colnde._lib.lib()
    W = _weights(cfg, 3)
    top = np.ascontiguousarray(bcs[:, 1])
    with colnde.FreeConvectionEnsemble(cfg, 9, 3) as e:
        assert L.colnde_n_models(e._h) == 3 and e.n_params == cfg.n_params
        e.set_problem(x0, bcs, truth)
        for call in (lambda: ColumnNDE.forward(e, W[0]), lambda: ColumnNDE.loss(e, W[0], SC), lambda: ColumnNDE.loss_grad(e, W[0], SC),
                     lambda: e.rhs(x0, W[0], bcs), lambda: e.flux(x0, W[0], bcs), lambda: e.loss_per_tstep(W[0]), lambda: e.error_estimate(W[0]),
                     lambda: e.choose_substeps(W[0]), lambda: e.set_substeps(4), lambda: e.set_global_columns(16),
                     lambda: e.infer_forcing(W[0], x0, top, 128.0), lambda: e.infer_dz_wT(W[0], x0, top, 128.0),
                     lambda: e.fc_embedded_step(W[0], x0, top, 128.0, 60.0, 10.0), lambda: e.fc_diagnose_wT(W[0], x0, top, 128.0, 10.0)):
            with pytest.raises(colnde.ColndeError, match="colnde_ensemble_"):
                call()
        with pytest.raises(colnde.ColndeError, match="no closure constants"):
            e.set_physics(np.tile(np.array([[1e-4, 0.1, 1.0, 0.25, 1.0]], np.float32), (3, 1)))
        z = np.zeros((3, 9, 32), np.float32)
        with pytest.raises(colnde.ColndeError, match="wind-mixing"):
            e.wm_embedded(W, z, z, z, np.zeros((3, 9), np.float32), 128.0, step=False)
        assert np.isfinite(e.loss(W, SC)).all()                           # the handle is still good
    with ColumnNDE(cfg, 9) as s:
        assert L.colnde_n_models(s._h) == 1
        with pytest.raises(colnde.ColndeError, match="not an ensemble handle"):
            colnde._lib.check(L.colnde_ensemble_column_loss_dev(s._h, None, None))
    with pytest.raises(colnde.ColndeError, match="free-convection"):
        colnde.ColumnNDEEnsemble(cfg, 9, 3)
