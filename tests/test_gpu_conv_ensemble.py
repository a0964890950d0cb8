"""Conv ensembles on the GPU (colnde_create_conv_ensemble): K `--conv c` networks of one filter length on the same simulations, the model index in
blockIdx.y of the 16-column fc32 kernels' third entry points and of the padding, filter-gradient and fold kernels.

The yardstick is exact: row k of every ensemble result must hold the bits a single `colnde.ColumnNDE(cfg, n, conv=c)` handle computes for model k's
weights — the same kernel text on the model's buffers at a stride, the same records, slices, slab rows and orders of summation.  Behind it stands the
float64 Toeplitz oracle of tests/conv_cases.py, held to the single conv handle's bounds.  Shapes are tests/test_gpu_conv.py's: one lane group, a
ragged tile and three tiles; Nz = 32 (a filter shift reads the wave's other column) and 64; the shortest and the longest filter."""
import ctypes
import functools

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde.flux_compat import ADAM
from colnde.free_convection import (FreeConvectionNDE, compute_nde_solution_history, conv_n_params, nde_loss_history,
                                    train_neural_differential_equation_device, train_neural_differential_equation_ensemble)
from colnde.nde import ColumnNDE, ENGINE_FC32
from tests.conv_cases import CPU_CHECKED, FC_KW, blocks, kw_items, oracle_loss_grad, reference
from tests.test_gpu_parity import _record, _rel, FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL

pytestmark = pytest.mark.gpu

MA = ["bf16x3_exact", "f32_mfma"]
SC = [0, 0, 1.0, 0, 0, 0]
CASES = [(32, 2, 1), (32, 3, 19), (32, 8, 33), (64, 2, 5), (64, 5, 17)]


@functools.lru_cache(maxsize=None)
def _members(Nz, c, ncol, kw, stepper="rk4", K=3, seed=21):
    """(problem, cfg, truth, W [K, n_params]): the case's own vector and K - 1 seeded perturbations of it (every entry scaled by 1 + 5 % noise)."""
    p, cfg, truth, _, _, _ = reference(Nz, c, ncol, kw, stepper=stepper) if stepper != "rk4" else reference(Nz, c, ncol, kw)      # (conv_cases' cache keys)
    rows = [p.weights]
    for k in range(1, K):
        r = synthetic._rng(seed, k)
        rows.append((p.weights * (1.0 + 0.05 * r.standard_normal(p.weights.shape))).astype(np.float32))
    W = np.stack(rows).astype(np.float32)
    W.setflags(write=False)
    return p, cfg, truth, W


def _single(cfg, c, p, truth, w, ma):
    """(sol, [grad; terms; total; 0], [terms; total], the row of a second loss_grad, describe, plan) of one conv handle built in this process."""
    with ColumnNDE(cfg, p.x0.shape[0], conv=c, matrix_arithmetic=ma) as h:
        assert h.engine == ENGINE_FC32
        h.set_problem(p.x0, p.bcs, truth)
        sol = h.forward(w)
        lt, lterms = h.loss(w, SC)
        total, terms, g = h.loss_grad(w, SC)
        total2, terms2, g2 = h.loss_grad(w, SC)
        row = lambda t, te, gr: np.concatenate([gr, te, [t, 0.0]]).astype(np.float32)
        return sol, row(total, terms, g), np.concatenate([lterms, [lt]]).astype(np.float32), row(total2, terms2, g2), h.describe(), h.plan()


def _ensemble(cfg, c, p, truth, W, ma):
    with colnde.FreeConvectionEnsemble(cfg, p.x0.shape[0], W.shape[0], matrix_arithmetic=ma, conv=c) as e:
        assert e.engine == ENGINE_FC32 and e.n_params == conv_n_params(cfg.Nz, c)
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        loss8 = e.loss(W, SC)
        res = e.loss_grad(W, SC)
        res2 = e.loss_grad(W, SC)
        return sol, res, loss8, res2, e.describe(), e.plan()


@functools.lru_cache(maxsize=None)
def _case_ensemble(Nz, c, ncol, ma):
    """The K = 3 ensemble of a case of test 1, run once and shared with the oracle test (read-only)."""
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    out = _ensemble(cfg, c, p, truth, W, ma)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def _assert_rows_are_the_single_handles_bits(c, members, ma, ens=None, idx=None):
    p, cfg, truth, W = members
    sol, res, loss8, res2, desc, plan = ens if ens is not None else _ensemble(cfg, c, p, truth, W, ma)
    K, P = W.shape[0], conv_n_params(cfg.Nz, c)
    assert sol.shape == (K, p.x0.shape[0], cfg.n_save, cfg.Nz) and res.shape == (K, P + 8) and loss8.shape == (K, 8)
    assert np.array_equal(res2, res)                                        # two ensemble calls: identical bits
    assert plan["conv"] == c and ("conv=%d" % c) in desc and ("models=%d" % K) in desc
    d1 = p1 = None
    for k in (range(K) if idx is None else idx):
        s1, r1, l1, r1b, d1, p1 = _single(cfg, c, p, truth, W[k], ma)
        assert np.array_equal(sol[k], s1), k
        assert np.array_equal(loss8[k, :7], l1), k
        assert np.array_equal(res[k], r1), (k, np.abs(res[k] - r1).max(), np.flatnonzero(res[k] != r1)[:8])
        assert np.array_equal(r1b, r1), k
    assert plan["dw_slices"] == p1["dw_slices"] and plan["time_segments"] == p1["time_segments"]      # the single handle's plan, hence its order of sums
    return desc, d1, plan


# ---- 1. rows are the single conv handle's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("Nz,c,ncol", CASES)
def test_rows_are_the_single_conv_handles_bits(Nz, c, ncol, ma):
    members = _members(Nz, c, ncol, kw_items(FC_KW))
    desc, _, plan = _assert_rows_are_the_single_handles_bits(c, members, ma, ens=_case_ensemble(Nz, c, ncol, ma))
    assert "engine=fc32" in desc and "tape_bytes_per_model=" in desc and "time_segments=0" in desc and "tile_width=16" in desc
    assert not np.array_equal(_case_ensemble(Nz, c, ncol, ma)[1][0], _case_ensemble(Nz, c, ncol, ma)[1][1])      # different weights, different rows


@pytest.mark.parametrize("ma", MA)
def test_one_model_is_the_single_conv_handle(ma):
    p, cfg, truth, W = _members(32, 3, 19, kw_items(FC_KW))
    _assert_rows_are_the_single_handles_bits(3, (p, cfg, truth, W[:1]), ma)


# ---- 2. ConvectiveAdjustmentNDE, RK4 and RKC2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("stepper", ["rk4", "rkc2"])
@pytest.mark.parametrize("case,ncol", [("ca/32/c8", 19), ("ca/64/c2", 5)])
def test_convective_adjustment_nde_bit_for_bit(case, ncol, stepper, ma):
    Nz, c, kw = CPU_CHECKED[case]
    if stepper == "rkc2":
        kw = dict(kw, substeps=2)                                           # two steps per save interval, automatic stage count
    members = _members(Nz, c, ncol, kw_items(kw), stepper)
    if stepper == "rkc2":
        assert colnde.rkc_stages(members[1]) >= 4
    desc, _, _ = _assert_rows_are_the_single_handles_bits(c, members, ma)
    assert ("stepper=rkc2" in desc) == (stepper == "rkc2")


# ---- 3. time segments -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("model,seg", [("fc", 2), ("fc", 3), ("ca_rkc2", 2), ("ca_rkc2", 3)])
def test_time_segments_bit_for_bit(model, seg, ma, monkeypatch):
    """COLNDE_FC_SEG set before both sides are created: the models march through the segments together, lambda and the conv tape per model."""
    Nz, c, ncol = 32, 3, 19
    kw = dict(FC_KW, n_save=6) if model == "fc" else dict(CPU_CHECKED["ca/32/c8"][2], n_save=6, substeps=2)
    members = _members(Nz, c, ncol, kw_items(kw), "rkc2" if model == "ca_rkc2" else "rk4")
    monkeypatch.setenv("COLNDE_FC_SEG", str(seg))
    desc, d1, plan = _assert_rows_are_the_single_handles_bits(c, members, ma)
    assert plan["time_segments"] == -(-5 // seg) >= 2
    assert ("time_segments=%d" % plan["time_segments"]) in desc and ("time_segments=%d" % plan["time_segments"]) in d1


# ---- 4. position and isolation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
def test_position_and_isolation(ma):
    Nz, c, ncol = 32, 3, 19
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    base = _case_ensemble(Nz, c, ncol, ma)
    perm = np.array([2, 0, 1])
    moved = _ensemble(cfg, c, p, truth, np.ascontiguousarray(W[perm]), ma)
    for a, b in zip(moved[:4], base[:4]):                                   # permuting the weight vectors permutes the rows, the last model included
        assert np.array_equal(a, b[perm])
    P = conv_n_params(Nz, c)
    others = np.arange(3) != 1
    # A NaN filter bias: every pre-activation of member 1's filter is NaN and the filter's relu lets it through (Flux's max(0, x)), into the record the
    # dW GEMM contracts: the member's W1 gradient is NaN.  Its solution and total stay finite — the dense chain's relu is fmaxf, which answers 0 to a
    # NaN, in every fc32 kernel — so the row is told apart by its gradient.  The other members keep every bit.
    Wn = W.copy()
    Wn[1, c] = np.nan
    nan = _ensemble(cfg, c, p, truth, Wn, ma)
    print("NaN filter bias: non-finite entries of row 1: %d of %d, total %r" % ((~np.isfinite(nan[1][1])).sum(), P + 8, nan[1][1, P + 6]))
    assert not np.isfinite(nan[1][1]).all()
    for a, b in zip(nan[:4], base[:4]):
        assert np.isfinite(a[others]).all() and np.array_equal(a[others], b[others])
    # A NaN that reaches the solution (the last output bias, as tests/test_gpu_fc_ensemble.py): solution, loss and total of the member are not finite
    Wn = W.copy()
    Wn[1, -1] = np.nan
    nan = _ensemble(cfg, c, p, truth, Wn, ma)
    assert not np.isfinite(nan[1][1, P + 6]) and not np.isfinite(nan[0][1]).all() and not np.isfinite(nan[2][1, 6])
    for a, b in zip(nan[:4], base[:4]):
        assert np.isfinite(a[others]).all() and np.array_equal(a[others], b[others])


# ---- 5. against the float64 oracle --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_rows(Nz, c, ncol):
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    _, _, _, tot, g, sol = reference(Nz, c, ncol, kw_items(FC_KW))
    return [(tot, g, sol)] + [oracle_loss_grad(cfg, c, p.x0, p.bcs, W[k], truth) for k in range(1, W.shape[0])]


@pytest.mark.parametrize("ma", MA)
@pytest.mark.parametrize("Nz,c,ncol", CASES)
def test_rows_against_the_float64_oracle(Nz, c, ncol, ma):
    """Every row held to the bounds tests/test_gpu_conv.py holds the single conv handle to: sol within FC_SOL_ATOL, loss within FC_LOSS_RTOL, the whole
    gradient within FC_GRAD_REL and every block of conv_cases.blocks within twice that."""
    sol, res, loss8, _, _, _ = _case_ensemble(Nz, c, ncol, ma)
    P = conv_n_params(Nz, c)
    for k, (tot, g, sol_o) in enumerate(_oracle_rows(Nz, c, ncol)):
        errs = dict(sol_abs=np.abs(sol[k] - sol_o).max(), loss_rel=abs(res[k, P + 6] - tot) / abs(tot), loss_only_rel=abs(loss8[k, 6] - tot) / abs(tot),
                    grad_rel=_rel(res[k, :P], g))
        for name, a, b in blocks(Nz, c):
            errs["grad_rel_" + name] = _rel(res[k, a:b], g[a:b])
        label = "conv_ens/fc/%s/%d/%d/%d/model%d" % (ma, Nz, c, ncol, k)
        _record(label, **errs)
        print(label, {n: "%.3e" % v for n, v in errs.items()})
        assert errs["sol_abs"] < FC_SOL_ATOL, k
        assert errs["loss_rel"] < FC_LOSS_RTOL and errs["loss_only_rel"] < FC_LOSS_RTOL, k
        assert errs["grad_rel"] < FC_GRAD_REL, k
        for name, a, b in blocks(Nz, c):
            assert errs["grad_rel_" + name] < 2 * FC_GRAD_REL, (k, name)


# ---- 6. the training loop -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ma", MA)
def test_training_loop_is_the_single_handles_and_follows_the_oracle(ma):
    """Five epochs, K = 3, rates (1e-3, 5e-4, 2e-3).  Member k's loss sequence and final weights equal, bit for bit, those of
    train_neural_differential_equation_device on a single conv handle with rate k: the gradients are the same bits (test 1) and the two ADAM kernels
    evaluate one expression on one element each.  Member 0 also follows the float64 loop on the folded oracle gradient within FC_LOSS_RTOL per step
    (tests/test_gpu_conv.py::test_conv_device_adam_follows_the_folded_oracle_gradient)."""
    Nz, c, ncol, epochs = 32, 3, 19, 5
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    etas = (1e-3, 5e-4, 2e-3)
    theta, hist = train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W, etas, epochs, matrix_arithmetic=ma, conv=c)
    assert theta.shape == W.shape and hist.shape == (epochs, 3)
    for k in range(3):
        nde = FreeConvectionNDE(cfg, p.x0, p.bcs, truth, conv=c, matrix_arithmetic=ma)
        try:
            theta_1, hist_1 = train_neural_differential_equation_device(nde, W[k].copy(), ADAM(etas[k]), epochs)
        finally:
            nde.close()
        print("model %d: ensemble %s single %s" % (k, hist[:, k], hist_1))
        assert np.array_equal(hist[:, k], np.array(hist_1, np.float32)), k
        assert np.array_equal(theta[k], theta_1), k
        assert np.abs(theta[k] - W[k]).max() > 0.5 * etas[k]
    th, opt, ref_hist = W[0].astype(np.float64), ADAM(etas[0]), []
    for _ in range(epochs):
        t, gr, _ = oracle_loss_grad(cfg, c, p.x0, p.bcs, th, truth)
        ref_hist.append(t)
        opt.update(th, gr)
    _record("conv_ens/adam5/%s" % ma, **{"loss_rel_step%d" % i: abs(a - b) / abs(b) for i, (a, b) in enumerate(zip(hist[:, 0], ref_hist))})
    for a, b in zip(hist[:, 0], ref_hist):
        assert np.isclose(a, b, rtol=FC_LOSS_RTOL), (hist[:, 0], ref_hist)


# ---- 7. causal penalty ----------------------------------------------------------------------------------------------------------------------------------------
def _w1_mask(n_params, H, M, off):
    """Boolean [n_params]: the entries W1[r, q], r < q, of a first Dense weight H x M at `off` (column-major: W1[r, q] at off + q H + r) —
    `mask = [x < y for x in 1:nrows, y in 1:ncols]`, train_free_convection_nde.jl:192-193."""
    m = np.zeros(n_params, bool)
    r, q = np.meshgrid(np.arange(H), np.arange(M), indexing="ij")
    m[off + (q * H + r)[r < q]] = True
    return m


def _check_penalty(base, out, zero, W, coeff, mask):
    """The bounds of tests/test_gpu_fc_ensemble.py::test_causal_penalty, against float64 `sum(abs2, W[mask])` and `2 c W[mask]`."""
    P = W.shape[1]
    n_mask = int(mask.sum())
    tol = n_mask * 2.0 ** -24                                               # worst case of an f32 sum of n_mask positive terms
    for k in range(W.shape[0]):
        if coeff[k] == 0:
            assert np.array_equal(out[k], base[k]) and not zero[k].any()   # c = 0: the row keeps its bits
            continue
        w = W[k].astype(np.float64)
        pen = float(coeff[k]) * float((w[mask] ** 2).sum())
        inc = float(zero[k, P + 6])
        print("causal penalty model %d: increment %.9e, float64 %.9e, rel %.3e (tolerance %.3e)" % (k, inc, pen, abs(inc / pen - 1), tol))
        assert abs(inc - pen) <= tol * pen
        assert abs(float(out[k, P + 6]) - (float(base[k, P + 6]) + inc)) <= np.spacing(np.float32(out[k, P + 6]))
        want = (base[k, :P].astype(np.float64) + 2.0 * float(coeff[k]) * w)[mask]
        got = out[k, :P][mask]
        assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all()
        assert not np.array_equal(got, base[k, :P][mask])
        keep = np.ones(P + 8, bool)
        keep[:P][mask] = False
        keep[P + 6] = False
        assert np.array_equal(out[k][keep], base[k][keep])                 # nothing outside the mask changes a bit (the total aside)
    return n_mask


@pytest.mark.parametrize("Nz,c,ncol", [(32, 3, 9), (64, 5, 5)])
def test_causal_penalty_on_the_conv_chains_first_dense(Nz, c, ncol):
    import torch
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    coeff = np.array([1.0, 0.0, 0.5], np.float32)
    P, H, M = conv_n_params(Nz, c), 4 * Nz, Nz - c + 1
    mask = _w1_mask(P, H, M, c + 1)
    with colnde.FreeConvectionEnsemble(cfg, ncol, 3, conv=c) as e:
        e.set_problem(p.x0, p.bcs, truth)
        base = e.loss_grad(W, SC)
        out = e.causal_penalty(W, coeff, base)
        t = torch.from_numpy(base).cuda()
        assert e.causal_penalty(torch.from_numpy(np.array(W)).cuda(), torch.from_numpy(coeff).cuda(), t) is t
        assert np.array_equal(t.cpu().numpy(), out)
        zero = e.causal_penalty(W, coeff, np.zeros_like(base))
    assert _check_penalty(base, out, zero, W, coeff, mask) == M * (M - 1) // 2
    assert not mask[:c + 1].any() and not mask[c + 1 + H * M:].any()       # the filter and everything behind W1 are outside the mask


def test_plain_ensembles_causal_penalty_keeps_its_bits():
    """The plain network through the kernel's new (H, M, offset) arguments: 4Nz x Nz at offset 0.  The increments on a zero buffer are compared with
    values computed from the same restatement's mask: the gradient entries are exactly 2 c W (one f32 product), the sum within its f32 bound."""
    Nz, n = 32, 9
    pl = synthetic.free_convection_problem(n, Nz=Nz, n_save=5, substeps=2, t_end=0.01)
    P = pl.cfg.n_params
    W = np.stack([synthetic.make_weights(synthetic._rng(11, k), pl.cfg, 1e2) for k in range(3)]).astype(np.float32)
    coeff = np.array([1.0, 0.0, 0.5], np.float32)
    mask = _w1_mask(P, 4 * Nz, Nz, 0)
    with colnde.FreeConvectionEnsemble(pl.cfg, n, 3) as e:
        e.set_problem(pl.x0, pl.bcs, None)
        zero = e.causal_penalty(W, coeff, np.zeros((3, P + 8), np.float32))
    for k in range(3):
        want = np.zeros(P, np.float32)
        want[mask] = np.float32(2.0) * coeff[k] * W[k][mask]
        assert np.array_equal(zero[k, :P], want), k                        # bit for bit: 2 c W on the 4Nz x Nz mask, zero elsewhere
        pen = float(coeff[k]) * float((W[k].astype(np.float64)[mask] ** 2).sum())
        assert abs(float(zero[k, P + 6]) - pen) <= int(mask.sum()) * 2.0 ** -24 * pen
    assert int(mask.sum()) == Nz * (Nz - 1) // 2


# ---- 8. column loss and the history functions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz,c,ncol", [(32, 3, 19), (64, 5, 17)])
def test_column_loss(Nz, c, ncol):
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    with colnde.FreeConvectionEnsemble(cfg, ncol, 3, conv=c) as e:
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        cl = e.column_loss(sol)
        cl2 = e.column_loss(sol)
    assert cl.shape == (3, ncol, cfg.n_save) and np.array_equal(cl, cl2)
    ref = ((sol.astype(np.float64) - truth.astype(np.float64)[None]) ** 2).mean(axis=3)
    np.testing.assert_allclose(cl, ref, rtol=1e-5, atol=0.0)                # relative 1e-5 > Nz 2^-24 (a 64-term f32 mean)


def test_history_functions_are_one_forward_call(monkeypatch):
    """compute_nde_solution_history / nde_loss_history with conv=c: E = 4 networks, one ensemble, ONE forward launch (kernel_time's launch count)."""
    Nz, c, ncol = 32, 3, 19
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW), K=4)
    counts = []
    set_problem, close = colnde.FreeConvectionEnsemble.set_problem, colnde.FreeConvectionEnsemble.close

    def profiled_set_problem(self, *a, **k):
        set_problem(self, *a, **k)
        self.set_profiling(True)

    def counting_close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            counts.append(self.kernel_time("forward")[1])
        close(self)

    monkeypatch.setattr(colnde.FreeConvectionEnsemble, "set_problem", profiled_set_problem)
    monkeypatch.setattr(colnde.FreeConvectionEnsemble, "close", counting_close)
    hist = compute_nde_solution_history(p.x0, p.bcs, cfg, W, conv=c)
    assert counts == [1]
    per_epoch, per_t = nde_loss_history(p.x0, p.bcs, truth, cfg, W, conv=c)
    assert counts == [1, 1]
    monkeypatch.undo()
    assert hist.shape == (4, ncol, Nz, cfg.n_save) and per_epoch.shape == (4, ncol) and per_t.shape == (4, ncol, cfg.n_save)
    for k in range(4):
        with ColumnNDE(cfg, ncol, conv=c) as h:
            h.set_problem(p.x0, p.bcs, truth)
            s = h.forward(W[k])
        assert np.array_equal(hist[k], np.transpose(cfg.sigma[2] * s + cfg.mu[2], (0, 2, 1))), k
        ref = ((s.astype(np.float64) - truth) ** 2).mean(axis=2)
        np.testing.assert_allclose(per_t[k], ref, rtol=1e-5, atol=0.0)
        np.testing.assert_allclose(per_epoch[k], ref.mean(axis=1), rtol=1e-5)


# ---- 9. refusals on the GPU -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_gpu():
    Nz, c, ncol = 32, 3, 19
    p, cfg, truth, W = _members(Nz, c, ncol, kw_items(FC_KW))
    L = _lib.lib()
    x0, bcs, w = p.x0, p.bcs, W[0]
    top = np.ascontiguousarray(bcs[:, 1])
    with colnde.FreeConvectionEnsemble(cfg, ncol, 3, conv=c) as e:
        assert L.colnde_n_models(e._h) == 3 and L.colnde_conv_filter(e._h) == c and e.n_params == conv_n_params(Nz, c)
        e.set_problem(x0, bcs, truth)
        assert "models=3" in e.describe() and "conv=3" in e.describe() and e.plan()["conv"] == 3
        refused = {
            "colnde_forward": lambda: ColumnNDE.forward(e, w),
            "colnde_loss": lambda: ColumnNDE.loss(e, w, SC),
            "colnde_loss_grad": lambda: ColumnNDE.loss_grad(e, w, SC),
            "colnde_rhs": lambda: e.rhs(x0, w, bcs, 0.0),
            "colnde_flux": lambda: e.flux(x0, w, bcs),
            "colnde_loss_per_tstep": lambda: e.loss_per_tstep(w),
            "colnde_error_estimate": lambda: e.error_estimate(w),
            "colnde_choose_substeps": lambda: e.choose_substeps(w, 1e-3),
            "colnde_set_substeps": lambda: e.set_substeps(4),
            "colnde_set_global_columns": lambda: e.set_global_columns(64),
            "colnde_infer_forcing": lambda: e.infer_forcing(w, x0, top, 128.0),
            "colnde_infer_dz_wT": lambda: e.infer_dz_wT(w, x0, top, 128.0),
            "colnde_fc_embedded_step": lambda: e.fc_embedded_step(w, x0, top, 128.0, 60.0, 10.0, None),
            "colnde_fc_diagnose_wT": lambda: e.fc_diagnose_wT(w, x0, top, 128.0, 10.0, None),
        }
        for name, call in refused.items():
            with pytest.raises(colnde.ColndeError, match=name + r"\w* takes one weight vector.*ensemble of 3 models"):
                call()
        z = ctypes.c_void_p()
        f = ctypes.c_float()
        bt = (ctypes.c_double * 2)(0.9, 0.999)
        assert L.colnde_pretrain_flux_dev(e._h, 2, z, z, z, z, z, z, z, 1, 1.0, 1e-3, 0.9, 0.999, 1e-8, bt, 0, ctypes.byref(f)) != 0
        assert "colnde_pretrain_flux_dev" in L.colnde_last_error().decode()
        with pytest.raises(colnde.ColndeError, match="colnde_ensemble_set_physics.*no closure constants"):
            e.set_physics(np.tile(np.array([[1e-4, 0.1, 1.0, 0.25, 1.0]], np.float32), (3, 1)))
        zs = np.zeros((3, ncol, Nz), np.float32)
        with pytest.raises(colnde.ColndeError, match="wind-mixing"):
            e.wm_embedded(W, zs, zs, zs, np.zeros((3, ncol), np.float32), 128.0, step=False)
        assert np.isfinite(e.loss(W, SC)).all()                             # the handle is still good
    with ColumnNDE(cfg, ncol, conv=c) as s:                                 # a single conv handle stays outside the ensemble calls
        assert L.colnde_n_models(s._h) == 1
        for call in (lambda: L.colnde_ensemble_forward_dev(s._h, z, z), lambda: L.colnde_ensemble_column_loss_dev(s._h, z, z)):
            assert call() != 0
            msg = L.colnde_last_error().decode()
            assert "colnde_ensemble_" in msg and "conv" in msg, msg
