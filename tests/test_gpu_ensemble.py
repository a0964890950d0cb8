"""Ensembles on the GPU (colnde_create_ensemble): K wind-mixing NDEs of one architecture in one launch per kernel.

Model k of an ensemble must compute exactly what a single handle built with model k's constants computes — bit for bit: the same kernels
run with the model index in the launch grid, the closure constants come from the same host expression, and the dW GEMM keeps the slice count
(hence the reduction order) of a single handle.  Horizons are short (5 save points) so the file stays quick."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.flux_compat import ADAM
from colnde.wind_mixing import WindMixingNDE, train_NDE_ensemble
from oracle import nde_oracle as O
from oracle import training_oracle as TO

pytestmark = pytest.mark.gpu

MA = ["bf16x3_exact", "f32_mfma"]
SC = [1, 1, 1, 5e-3, 5e-3, 5e-3]
# (nu0, nu_minus, dRi, Ric, Pr): inside the default constants' stability bound (nu0 + nu_minus <= 0.1001, Pr >= 1)
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2], [1e-3, 0.05, 1.3, 0.3, 1.0], [2e-4, 0.09, 0.6, 0.15, 2.0],
                 [3e-4, 0.07, 1.1, 0.35, 1.5]], np.float32)


def _problem(n_col, **kw):
    p = synthetic.wind_mixing_problem(n_col, n_frames=5, weight_divisor=1e2, **kw)
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    return p, truth


def _weights(cfg, K, seed=11):
    return np.stack([synthetic.make_weights(synthetic._rng(seed, k), cfg, 1e2) for k in range(K)]).astype(np.float32)


def _model_cfg(cfg, row):
    return cfg.with_(**dict(zip(colnde.nde.PHYSICS_KEYS, [float(x) for x in row])))


def _single(cfg, p, truth, w, ma):
    """(sol, [grad; terms; total; 0], [terms; total]) of one ColumnNDE: the reference for one row of the ensemble."""
    with colnde.ColumnNDE(cfg, p.n_columns, matrix_arithmetic=ma) as h:
        h.set_problem(p.x0, p.bcs, truth)
        sol = h.forward(w)
        lt, lterms = h.loss(w, SC)
        total, terms, g = h.loss_grad(w, SC)
        return sol, np.concatenate([g, terms, [total, 0.0]]).astype(np.float32), np.concatenate([lterms, [lt]]).astype(np.float32)


def _ensemble(p, truth, W, physics, ma):
    with colnde.ColumnNDEEnsemble(p.cfg, p.n_columns, W.shape[0], physics=physics, matrix_arithmetic=ma) as e:
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        res = e.loss_grad(W, SC)
        loss8 = e.loss(W, SC)
        desc = e.describe()
    return sol, res, loss8, desc


def _assert_rows_bit_identical(p, truth, W, physics, ma, idx, cfg_of=None):
    sol, res, loss8, desc = _ensemble(p, truth, W, physics, ma)
    assert res.shape == (W.shape[0], p.cfg.n_params + 8)
    for k in idx:
        cfg = cfg_of(k) if cfg_of else (p.cfg if physics is None else _model_cfg(p.cfg, physics[k]))
        s1, r1, l1 = _single(cfg, p, truth, W[k], ma)
        assert np.array_equal(sol[k], s1), k
        assert np.array_equal(res[k], r1), (k, np.abs(res[k] - r1).max())
        assert np.array_equal(loss8[k, :7], l1), k                        # colnde_ensemble_loss against colnde_loss
    return desc


@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("n_col", [8, 40])
def test_models_match_single_handles_bit_for_bit(ma, n_col):
    p, truth = _problem(n_col)
    W = _weights(p.cfg, 5)
    desc = _assert_rows_bit_identical(p, truth, W, PHYS, ma, range(5))
    assert "models=5" in desc and "rich_tape=1" in desc


@pytest.mark.parametrize("ma", MA)
def test_plain_tape_matches_single_handles_bit_for_bit(ma, monkeypatch):
    monkeypatch.setenv("COLNDE_T16_SPLIT_RICH", "0")                 # before both sides are created
    p, truth = _problem(8)
    desc = _assert_rows_bit_identical(p, truth, _weights(p.cfg, 5), PHYS, ma, range(5))
    assert "rich_tape=0" in desc


@pytest.mark.parametrize("ma", MA)
def test_models_match_the_float64_oracle(ma):
    p, truth = _problem(8)
    W = _weights(p.cfg, 5)
    _, res, _, _ = _ensemble(p, truth, W, PHYS, ma)
    n = p.cfg.n_params
    for k in range(5):
        cfg = _model_cfg(p.cfg, PHYS[k])
        tot, terms, g, sol = O.loss_and_grad(cfg, p.x0, p.bcs, W[k], truth, np.array(SC, np.float64))
        assert abs(res[k, n + 6] - tot) <= 8e-5 * abs(tot), (k, res[k, n + 6], tot)
        assert np.linalg.norm(res[k, :n] - g) / np.linalg.norm(g) < 2e-4, k
    # the constants matter: models 0 and 1 with the SAME weights differ
    W2 = np.stack([W[0], W[0]])
    _, r2, _, _ = _ensemble(p, truth, W2, PHYS[:2], ma)
    assert not np.array_equal(r2[0], r2[1])


@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("K", [64, 300])
def test_position_and_isolation(ma, K, monkeypatch):
    if K > 128:
        monkeypatch.setenv("COLNDE_T16_SPLIT_RICH", "0")             # > 128 tiles in flight: the plain tape; the single handles run the same kernels
    p, truth = _problem(8)
    W = _weights(p.cfg, K, seed=5)
    phys = PHYS[np.arange(K) % 5]
    _assert_rows_bit_identical(p, truth, W, phys, ma, [0, 1, K // 2, K - 1])
    # NaN weights in model j: its row is not finite, every other row is unchanged
    j = K // 3
    Wn = W.copy()
    Wn[j, 7] = np.nan
    _, base, _, _ = _ensemble(p, truth, W, phys, ma)
    _, nanr, _, _ = _ensemble(p, truth, Wn, phys, ma)
    n = p.cfg.n_params
    assert not np.isfinite(nanr[j, n + 6])
    others = np.arange(K) != j
    assert np.isfinite(nanr[others]).all()
    assert np.array_equal(nanr[others], base[others])


@pytest.mark.parametrize("ma", MA)
def test_rkc2_convective_adjustment_branch_bit_for_bit(ma):
    p, truth = _problem(8, modified_pacanowski_philander=False, zero_weights=False, convective_adjustment=True, kappa=10.0, stepper="rkc2", substeps=1)
    _assert_rows_bit_identical(p, truth, _weights(p.cfg, 3, seed=3), None, ma, range(3))


@pytest.mark.parametrize("ma", MA)
def test_train_NDE_ensemble_follows_the_float64_loop(ma):
    p, truth = _problem(8)
    K, iters = 3, 5
    W = _weights(p.cfg, K, seed=7)
    etas = np.array([3e-4, 1e-4, 5e-4], np.float32)
    wm = WindMixingNDE(p.cfg, p.x0, p.bcs, truth, matrix_arithmetic=ma)
    try:
        res = train_NDE_ensemble(wm, W, PHYS[:K], etas, epochs=1, maxiters=iters)
        sc = wm.loss_scalings
    finally:
        wm.close()
    assert len(res) == K
    for k in range(K):
        cfg = _model_cfg(p.cfg, PHYS[k])
        theta_o, hist_o = TO.train_NDE(cfg, p.x0, p.bcs, truth, W[k], sc, [float(etas[k])], epochs=1, maxiters=iters)
        lo = np.array([h["total"] for h in hist_o])
        lg = np.array([h["total"] for h in res[k].history])
        assert len(lg) == iters
        assert np.abs(lg / lo - 1).max() < 1e-4, (k, lg, lo)                              # test_gpu_training_parity's tolerances
        th = res[k].weights.astype(np.float64)
        assert np.linalg.norm(th - theta_o) / np.linalg.norm(theta_o) < 1.5e-4, k
        assert np.abs(th - theta_o).max() / etas[k] < 0.05, k
        assert np.abs(res[k].weights - W[k]).max() > 0.5 * etas[k]


def test_refusals_name_the_reason():
    p, truth = _problem(8)
    L = colnde._lib.lib()
    for cfg, what in ((p.cfg.with_(substeps=0), "substeps = 0"), (p.cfg.with_(inplace_variant=True), "inplace_variant"),
                      (synthetic.free_convection_problem(8, n_save=3).cfg, "free-convection")):
        with pytest.raises(colnde.ColndeError, match=what):
            colnde.ColumnNDEEnsemble(cfg, 8, 2)
    with pytest.raises(colnde.ColndeError, match="8,192 columns"):
        colnde.ColumnNDEEnsemble(p.cfg, 8193, 2)
    wide = synthetic.wind_mixing_problem(8, n_frames=3, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
    with pytest.raises(colnde.ColndeError, match="net-split shape"):
        colnde.ColumnNDEEnsemble(wide.cfg, 8, 2)
    with pytest.raises(colnde.ColndeError, match="engine forced"):
        c, keep = colnde.config.to_c_config(p.cfg, 8, 0, colnde.nde.ENGINE_TILE16)
        h = ctypes.c_void_p()
        colnde._lib.check(L.colnde_create_ensemble(ctypes.byref(c), 2, None, ctypes.byref(h)))
    with pytest.raises(colnde.ColndeError, match="modified_pacanowski_philander = 1"):
        colnde.ColumnNDEEnsemble(p.cfg.with_(modified_pacanowski_philander=False, zero_weights=False), 8, 2, physics=PHYS[:2])
    bad = PHYS[:3].copy()
    bad[2, 1] = 100.0
    with pytest.raises(colnde.ColndeError, match="model 2"):
        colnde.ColumnNDEEnsemble(p.cfg, 8, 3, physics=bad)
    W = _weights(p.cfg, 3)
    with colnde.ColumnNDEEnsemble(p.cfg, 8, 3, physics=PHYS[:3]) as e:
        assert L.colnde_n_models(e._h) == 3
        with pytest.raises(colnde.ColndeError, match="model 2"):
            e.set_physics(bad)
        e.set_physics(PHYS[2:5])
        e.set_problem(p.x0, p.bcs, truth)
        for call in (lambda: colnde.nde.ColumnNDE.forward(e, W[0]), lambda: colnde.nde.ColumnNDE.loss(e, W[0], SC),
                     lambda: colnde.nde.ColumnNDE.loss_grad(e, W[0], SC), lambda: e.rhs(p.x0, W[0], p.bcs), lambda: e.flux(p.x0, W[0], p.bcs),
                     lambda: e.loss_per_tstep(W[0]), lambda: e.error_estimate(W[0]), lambda: e.choose_substeps(W[0]), lambda: e.set_substeps(4),
                     lambda: e.set_global_columns(16), lambda: e.infer_forcing(W[0], p.x0[:, :32], p.bcs[:, 5], 256.0)):
            with pytest.raises(colnde.ColndeError, match="colnde_ensemble_"):
                call()
    with colnde.ColumnNDE(p.cfg, 8) as s:
        assert L.colnde_n_models(s._h) == 1
