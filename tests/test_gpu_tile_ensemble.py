"""Tile ensembles on the GPU (colnde_create_tile_ensemble): K wind-mixing NDEs of ANY tile16 architecture in one launch per kernel.

Row k of an ensemble must hold exactly what a single handle on the tile16 engine computes with model k's weights and constants — bit for bit: the
kernels are the single handle's text with the model index in the launch grid, the launch geometry is decided from ONE model's tiles, the closure
constants come from the same host expression and the dW GEMM keeps the single handle's slice count.  The shapes cover every kernel form: rows in global
memory with bf16 planes (96-400-400-31), the reference's third architecture (96-32-400-31), rows in LDS with the weights streamed (96-400-31), weights in
LDS (96-24-31), tile16's kernels on the net-split shape (96-50-20-31), and another grid (Nz = 16, 48-20-15).  Horizons are short (4 save points)."""
import functools

import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.nde import ENGINE_TILE16
from colnde.wind_mixing import WindMixingNDE, train_NDE_ensemble
from oracle import nde_oracle as O
from oracle import training_oracle as TO

from tests.test_gpu_ensemble import PHYS, SC
from tests.test_gpu_parity import GRAD_REL, LOSS_RTOL, SOL_ATOL, _record

pytestmark = pytest.mark.gpu

MA = ["bf16x3_exact", "f32_mfma"]
SHAPES = {
    "96-400-400-31_swish": dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity")),
    "96-32-400-31_swish": dict(layer_sizes=(96, 32, 400, 31), activations=("swish", "swish", "identity")),
    "96-400-31_mish": dict(layer_sizes=(96, 400, 31), activations=("mish", "identity")),
    "96-24-31_tanh": dict(layer_sizes=(96, 24, 31), activations=("tanh", "identity")),
    "96-50-20-31_mish": dict(layer_sizes=(96, 50, 20, 31), activations=("mish", "mish", "identity")),
    "Nz16_48-20-15_leakyrelu": dict(Nz=16, layer_sizes=(48, 20, 15), activations=("leakyrelu", "identity")),
}
ORACLE_SHAPES = ["96-400-400-31_swish", "96-32-400-31_swish", "96-400-31_mish"]


@functools.lru_cache(maxsize=None)
def _problem(shape, n_col, **kw):
    p = synthetic.wind_mixing_problem(n_col, n_frames=4, weight_divisor=1e2, **SHAPES[shape], **dict(kw))
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    return p, truth


def _weights(cfg, K, seed=11):
    return np.stack([synthetic.make_weights(synthetic._rng(seed, k), cfg, 1e2) for k in range(K)]).astype(np.float32)


def _model_cfg(cfg, row):
    return cfg.with_(**dict(zip(colnde.nde.PHYSICS_KEYS, [float(x) for x in row])))


def _single(cfg, p, truth, w, ma):
    """(sol, [grad; terms; total; 0], [terms; total]) of one ColumnNDE on the tile16 engine: the reference for one row of the ensemble"""
    with colnde.ColumnNDE(cfg, p.n_columns, engine=ENGINE_TILE16, matrix_arithmetic=ma) as h:
        h.set_problem(p.x0, p.bcs, truth)
        sol = h.forward(w)
        lt, lterms = h.loss(w, SC)
        total, terms, g = h.loss_grad(w, SC)
        return sol, np.concatenate([g, terms, [total, 0.0]]).astype(np.float32), np.concatenate([lterms, [lt]]).astype(np.float32)


def _run(e, W):
    return e.forward(W), e.loss_grad(W, SC), e.loss(W, SC)


def _ensemble(p, truth, W, physics, ma):
    with colnde.TileNDEEnsemble(p.cfg, p.n_columns, W.shape[0], physics=physics, matrix_arithmetic=ma) as e:
        e.set_problem(p.x0, p.bcs, truth)
        sol, res, loss8 = _run(e, W)
        desc = e.describe()
    return sol, res, loss8, desc


def _assert_rows(p, truth, got, W, physics, ma, idx):
    sol, res, loss8 = got[:3]
    assert res.shape == (W.shape[0], p.cfg.n_params + 8)
    for k in idx:
        cfg = p.cfg if physics is None else _model_cfg(p.cfg, physics[k])
        s1, r1, l1 = _single(cfg, p, truth, W[k], ma)
        assert np.array_equal(sol[k], s1), k
        assert np.array_equal(res[k], r1), (k, np.abs(res[k] - r1).max())
        assert np.array_equal(loss8[k, :7], l1), k


# ---- 1. rows are the single handle's bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("n_col", [8, 40])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rows_are_the_single_handles_bits(shape, n_col, ma):
    p, truth = _problem(shape, n_col)
    W = _weights(p.cfg, 5)
    got = _ensemble(p, truth, W, PHYS, ma)
    _assert_rows(p, truth, got, W, PHYS, ma, range(5))
    desc = got[3]
    assert "models=5" in desc and "tile_ensemble" in desc and "engine=tile16 " in desc
    assert ("activation_rows=global_memory" in desc) == (shape == "96-400-400-31_swish")


# ---- 2. rows against float64 --------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300)


def _check_against_oracle(shape, n_col, ma, blocks):
    """Bounds: the project's wind-mixing bounds (tests/test_gpu_parity.py).  The float32 C port of the oracle is off, across these shapes and members, by at most
    3.5e-7 (solution), 4.4e-6 (total), 1.9e-5 (whole gradient) and 1.3e-5 (worst layer block, members 1-4): a tenth of the bounds or less.  Member 0
    carries the truth's constants, its loss is ~1e-5 and its worst block 4.0e-4 in float32: its blocks are not checked."""
    p, truth = _problem(shape, n_col)
    W = _weights(p.cfg, 5)
    sol, res, _, _ = _ensemble(p, truth, W, PHYS, ma)
    n = p.cfg.n_params
    sizes = p.cfg.layer_sizes
    for k in range(5):
        cfg = _model_cfg(p.cfg, PHYS[k])
        tot, terms, g, sol64 = O.loss_and_grad(cfg, p.x0, p.bcs, W[k], truth, np.array(SC, np.float64))
        worst = 0.0
        off = 0
        for net in range(3):
            for a, b in zip(sizes[:-1], sizes[1:]):
                for m in (a * b, b):
                    worst = max(worst, _rel(res[k, off:off + m], g[off:off + m]))
                    off += m
        assert off == n
        _record("tile_ens/%s/%d/%s/member%d" % (shape, n_col, ma, k), sol_abs=np.abs(sol[k] - sol64).max(), loss_rel=abs(res[k, n + 6] - tot) / abs(tot),
                grad_rel=_rel(res[k, :n], g), worst_block=worst)
        assert np.abs(sol[k] - sol64).max() < SOL_ATOL, k
        assert abs(res[k, n + 6] - tot) <= LOSS_RTOL * abs(tot), (k, res[k, n + 6], tot)
        assert _rel(res[k, :n], g) < GRAD_REL, k
        if blocks and k >= 1:
            assert worst < 4 * GRAD_REL, (k, worst)


@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_rows_against_the_float64_oracle(shape, ma):
    _check_against_oracle(shape, 8, ma, blocks=True)


@pytest.mark.parametrize("n_col", [8, 40])
def test_another_grid_against_the_float64_oracle(n_col):
    _check_against_oracle("Nz16_48-20-15_leakyrelu", n_col, "bf16x3_exact", blocks=False)


@pytest.mark.parametrize("shape", ["96-400-400-31_swish", "96-24-31_tanh"])
def test_constants_matter_and_rows_follow_their_weights(shape):
    p, truth = _problem(shape, 8)
    W = _weights(p.cfg, 3)
    # two members with the same weights and different constants differ
    _, r2, _, _ = _ensemble(p, truth, np.stack([W[0], W[0]]), PHYS[:2], MA[0])
    assert not np.array_equal(r2[0], r2[1])
    # exchanging two members' weight rows (same constants) exchanges their result rows bit for bit
    ph = PHYS[[1, 1, 2]]
    sa, ra, la, _ = _ensemble(p, truth, W, ph, MA[0])
    sb, rb, lb, _ = _ensemble(p, truth, W[[1, 0, 2]], ph, MA[0])
    for a, b in ((sa, sb), (ra, rb), (la, lb)):
        assert np.array_equal(a[[1, 0, 2]], b) and not np.array_equal(a[0], a[1])


# ---- 3. position and isolation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K", [("96-24-31_tanh", 70), ("96-400-400-31_swish", 9)])
def test_position_and_isolation(shape, K):
    ma = MA[0]
    p, truth = _problem(shape, 8)
    W = _weights(p.cfg, K, seed=5)
    phys = PHYS[np.arange(K) % 5]
    base = _ensemble(p, truth, W, phys, ma)
    _assert_rows(p, truth, base, W, phys, ma, [0, 1, K // 2, K - 1])
    # NaN weights in model j: its row is not finite, every other row is unchanged
    j = K // 3
    Wn = W.copy()
    n = p.cfg.n_params
    Wn[j, n // 3 - 1] = np.nan                          # the last output bias of net 0 (identity layer: the engine's tanh squashes a NaN further in)
    nanr = _ensemble(p, truth, Wn, phys, ma)[1]
    assert not np.isfinite(nanr[j, n + 6])
    others = np.arange(K) != j
    assert np.isfinite(nanr[others]).all()
    assert np.array_equal(nanr[others], base[1][others])


# ---- 4. RKC2, convective-adjustment branch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("shape", ["96-400-400-31_swish", "96-24-31_tanh"])
def test_rkc2_convective_adjustment_branch_bit_for_bit(shape, ma):
    p, truth = _problem(shape, 8, modified_pacanowski_philander=False, zero_weights=False, convective_adjustment=True, kappa=10.0, stepper="rkc2", substeps=1)
    W = _weights(p.cfg, 3, seed=3)
    got = _ensemble(p, truth, W, None, ma)
    _assert_rows(p, truth, got, W, None, ma, range(3))
    assert "rkc2" in got[3]


# ---- 5. set_matrix_arithmetic after the first loss_grad, and set_physics ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["96-400-400-31_swish", "96-400-31_mish"])
def test_reconfigured_ensemble_equals_a_fresh_one(shape):
    p, truth = _problem(shape, 8)
    W = _weights(p.cfg, 3)
    fresh = _ensemble(p, truth, W, PHYS[2:5], "f32_mfma")
    with colnde.TileNDEEnsemble(p.cfg, p.n_columns, 3, physics=PHYS[:3], matrix_arithmetic="bf16x3_exact") as e:
        e.set_problem(p.x0, p.bcs, truth)
        first = _run(e, W)
        e.set_matrix_arithmetic("f32_mfma")
        e.set_physics(PHYS[2:5])
        again = _run(e, W)
    assert not np.array_equal(first[1], again[1])
    for a, b in zip(again, fresh[:3]):
        assert np.array_equal(a, b)


# ---- 6. train_NDE_ensemble on the reference's third architecture ---------------------------------------------------------------------------------------------
def test_train_NDE_ensemble_follows_the_float64_loop():
    p, truth = _problem("96-32-400-31_swish", 8)
    K, iters = 3, 5
    W = _weights(p.cfg, K, seed=7)
    etas = np.array([3e-4, 1e-4, 5e-4], np.float32)
    wm = WindMixingNDE(p.cfg, p.x0, p.bcs, truth, matrix_arithmetic=MA[0])
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
        assert np.abs(lg / lo - 1).max() < 1e-4, (k, lg, lo)                              # tests/test_gpu_ensemble.py's tolerances
        th = res[k].weights.astype(np.float64)
        assert np.linalg.norm(th - theta_o) / np.linalg.norm(theta_o) < 1.5e-4, k
        assert np.abs(th - theta_o).max() / etas[k] < 0.05, k
        assert np.abs(res[k].weights - W[k]).max() > 0.5 * etas[k]


# ---- 7. refusals that need a handle ------------------------------------------------------------------------------------------------------------------------
def test_calls_that_do_not_serve_a_tile_ensemble_name_themselves():
    import torch
    p, truth = _problem("96-24-31_tanh", 8)
    W = _weights(p.cfg, 2)
    L = colnde._lib.lib()
    wide, _ = _problem("96-400-400-31_swish", 8)
    with pytest.raises(colnde.ColndeError, match="net-split shape"):
        colnde.ColumnNDEEnsemble(wide.cfg, 8, 2)
    with colnde.TileNDEEnsemble(p.cfg, 8, 2, physics=PHYS[:2]) as e:
        assert L.colnde_n_models(e._h) == 2
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        dev = torch.device("cuda", 0)
        Wd = torch.as_tensor(W).to(dev)
        z = torch.zeros((2, p.cfg.n_params), device=dev)
        nsave = len(p.cfg.save_times)
        state = tuple(np.zeros((2, 8, 32), np.float32) for _ in range(3))
        calls = {
            "colnde_ensemble_set_member_loss": lambda: e.set_member_loss(np.ones((2, 6), np.float32), None),
            "colnde_ensemble_member_loss_dev": lambda: e.member_loss(W),
            "colnde_ensemble_member_loss_grad_dev": lambda: e.member_loss_grad(Wd),
            "colnde_ensemble_member_loss_grad": lambda: e.member_loss_grad(W),
            "colnde_set_schedule": lambda: e.set_schedule([2] * (nsave - 1)),
            "colnde_ensemble_wm_embedded": lambda: e.wm_embedded(W, *state, np.zeros((3, 8), np.float32), 256.0, step=False),
            "colnde_ensemble_profile": lambda: e.profile(W, sol),
            "colnde_ensemble_pretrain_wm_flux_dev": lambda: e.pretrain_fluxes(Wd, z, z.clone(), torch.zeros((4, 96), device=dev), torch.zeros((4, 6), device=dev),
                                                                               torch.zeros((3, 4, 33), device=dev), None, 1.0, torch.ones((2, 3), device=dev)),
        }
        for name, call in calls.items():
            with pytest.raises(colnde.ColndeError, match=name):
                call()
        single = {
            "colnde_forward": lambda: colnde.nde.ColumnNDE.forward(e, W[0]), "colnde_loss": lambda: colnde.nde.ColumnNDE.loss(e, W[0], SC),
            "colnde_loss_grad": lambda: colnde.nde.ColumnNDE.loss_grad(e, W[0], SC), "colnde_rhs": lambda: e.rhs(p.x0, W[0], p.bcs),
            "colnde_flux": lambda: e.flux(p.x0, W[0], p.bcs), "colnde_loss_per_tstep": lambda: e.loss_per_tstep(W[0]),
            "colnde_error_estimate": lambda: e.error_estimate(W[0]), "colnde_choose_substeps": lambda: e.choose_substeps(W[0]),
            "colnde_set_substeps": lambda: e.set_substeps(4), "colnde_set_global_columns": lambda: e.set_global_columns(16),
            "colnde_choose_schedule": lambda: e.choose_schedule(W[0]), "colnde_infer_forcing": lambda: e.infer_forcing(W[0], p.x0[:, :32], p.bcs[:, 5], 256.0),
        }
        for name, call in single.items():
            with pytest.raises(colnde.ColndeError, match=name):
                call()
        # the handle still serves what it serves
        assert np.array_equal(e.forward(W), sol)


# ---- 8. side stream ------------------------------------------------------------------------------------------------------------------------------------
def test_loss_grad_on_a_side_stream_equals_the_null_stream_bits():
    from tests import stream_cases as S
    shape = "96-400-400-31_swish"
    p, truth = _problem(shape, 8)
    q = synthetic.wind_mixing_problem(8, n_frames=4, weight_divisor=1e2, seed=synthetic.SEED + 1, **SHAPES[shape])
    truth_q = O.solve(q.cfg, q.x0, q.bcs, q.weights_truth).astype(np.float32)
    W = _weights(p.cfg, 3)
    late = S.Late(x0=(p.x0, q.x0), bcs=(p.bcs, q.bcs), truth=(truth, truth_q), w=(W, S.half(W)))
    side = S.side_streams()[0]
    make = lambda: colnde.TileNDEEnsemble(p.cfg, 8, 3, physics=PHYS[:3])

    def warm(h):
        h.set_problem(q.x0, q.bcs, truth_q)
        h.loss_grad(S.half(W), SC)

    def body(h, t, still):
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
        g = h.loss_grad(t["w"], SC)
        still("ensemble_loss_grad_dev")
        return (g,)

    got, ref = S.late_inputs(side, make, late, body, warm=warm, tag="tile_ensemble")
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(ref[0], _ensemble(p, truth, W, PHYS[:3], MA[0])[1])
