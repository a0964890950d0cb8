"""The regtile engine's layer-1 pre-activation tape (Z1): the forward kernel stores its ten layer-1 accumulator tiles as they are, the adjoint
kernel's loads rename them into its per-net registers.  A mis-addressed record permutes or mixes hidden features, so every layer block of every
net is checked, on column counts that exercise each way the record can be addressed: one 32-column tile (32), a second tile with part of half 0
live and a dead half 1 (40), a partly live half 1 (49), and several tape blocks through one buffer (96 columns as blocks of 32)."""
import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.nde import ENGINE_REGTILE
from oracle import nde_oracle as O
# the tolerances tests/test_gpu_parity.py applies to the regtile engine on this weight set (weights/1e2, a few frames)
from tests.test_gpu_parity import LOSS_RTOL, GRAD_REL, _rel

pytestmark = pytest.mark.gpu

CASES = [(32, None), (40, None), (49, None), (96, "32")]          # (columns, COLNDE_RT_BLOCK)
ARITHMETICS = ["bf16x3_exact", "f32_mfma"]
SCALINGS = np.array([1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3])

_cases = {}


def _case(n_col):
    """Problem (3 save points x 2 sub-steps, weights/1e2 so that layer 1 matters) and its float64 oracle results: computed once per column count."""
    if n_col not in _cases:
        p = synthetic.wind_mixing_problem(n_col, n_frames=3, substeps=2, weight_divisor=1e2)
        truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
        tot, terms, g, _ = O.loss_and_grad(p.cfg, p.x0, p.bcs, p.weights, truth, SCALINGS)
        for a in (terms, g):
            a.setflags(write=False)
        _cases[n_col] = (p, truth, tot, terms, g)
    return _cases[n_col]


def _blocks(cfg):
    """(name, slice) of every layer block of every net in Flux.destructure order: W1, b1, W2, b2, W3, b3 per net."""
    out, o, s = [], 0, cfg.layer_sizes
    for n in range(cfg.n_params // cfg.net_size):
        for i in range(len(s) - 1):
            for nm, sz in (("W", s[i] * s[i + 1]), ("b", s[i + 1])):
                out.append(("net%d/%s%d" % (n, nm, i + 1), slice(o, o + sz)))
                o += sz
    assert o == cfg.n_params
    return out


def _loss_grad(monkeypatch, n_col, block, ma, ztape="1", calls=1):
    p, truth = _case(n_col)[:2]
    monkeypatch.setenv("COLNDE_RT_ZTAPE", ztape)
    if block:
        monkeypatch.setenv("COLNDE_RT_BLOCK", block)
    else:
        monkeypatch.delenv("COLNDE_RT_BLOCK", raising=False)
    with colnde.ColumnNDE(p.cfg, p.n_columns, engine=ENGINE_REGTILE, matrix_arithmetic=ma) as nde:
        assert nde.engine == ENGINE_REGTILE
        nde.set_problem(p.x0, p.bcs, truth)
        res = [nde.loss_grad(p.weights, SCALINGS) for _ in range(calls)]
        plan = nde.plan()
    assert plan["z1_taped"] == (ztape == "1") and plan["matrix_arithmetic"] == ma
    return res if calls > 1 else res[0]


@pytest.mark.parametrize("ma", ARITHMETICS)
@pytest.mark.parametrize("n_col,block", CASES)
def test_taped_gradient_against_oracle_per_layer_block(n_col, block, ma, monkeypatch):
    """Loss and gradient of the taped path against the float64 oracle; the gradient tolerance holds for every layer block of every net, so a
    permuted or misplaced hidden feature cannot hide in the norm of the whole.  (Measured: loss terms 3.7e-5, whole gradient 3.0e-6, worst
    block 7.1e-5.)"""
    p, _, tot, terms, g = _case(n_col)
    tot_g, terms_g, grad_g = _loss_grad(monkeypatch, n_col, block, ma)
    errs = {name: _rel(grad_g[s], g[s]) for name, s in _blocks(p.cfg)}
    print("n_col %d %s: loss rel %.3e, grad rel %.3e, worst block %s %.3e" % (n_col, ma, abs(tot_g - tot) / abs(tot), _rel(grad_g, g),
                                                                             max(errs, key=errs.get), max(errs.values())))
    np.testing.assert_allclose(terms_g, terms, rtol=LOSS_RTOL, atol=1e-12)
    assert np.isclose(tot_g, tot, rtol=LOSS_RTOL)
    assert _rel(grad_g, g) < GRAD_REL
    for name, e in errs.items():
        assert e < GRAD_REL, (name, e)


# Distance between the gradient from the taped Z1 and the one whose adjoint recomputes layer 1 (COLNDE_RT_ZTAPE=0; that adjoint runs f32 MFMA,
# so under bf16x3_exact the two also differ in the W1^T products' arithmetic), as MEASURED on the commit before this record format, largest of
# the four column counts: whole gradient 3.7e-8 (bf16x3_exact) / 2.1e-11 (f32_mfma), worst layer block 1.65e-7 / 8.5e-8.  Bounds: 4x that.
TAPED_VS_RECOMPUTED = {"bf16x3_exact": (4 * 3.7e-8, 4 * 1.65e-7), "f32_mfma": (4 * 2.1e-11, 4 * 8.5e-8)}


@pytest.mark.parametrize("ma", ARITHMETICS)
@pytest.mark.parametrize("n_col,block", CASES)
def test_taped_layer1_equals_recomputed_layer1(n_col, block, ma, monkeypatch):
    """Same inputs, two handles: the adjoint reads the Z1 tape / recomputes layer 1 from the stage tape.  The two pre-activations are the same
    numbers up to the order of the additions, so the gradients agree to arithmetic-order noise — bounds above (measured before this record
    format: 3.7e-8 / 2.1e-11 whole, 1.65e-7 / 8.5e-8 per block; this format measures the same)."""
    p = _case(n_col)[0]
    _, _, g_tape = _loss_grad(monkeypatch, n_col, block, ma, ztape="1")
    _, _, g_rec = _loss_grad(monkeypatch, n_col, block, ma, ztape="0")
    whole, per_block = TAPED_VS_RECOMPUTED[ma]
    errs = {name: _rel(g_tape[s], g_rec[s].astype(np.float64)) for name, s in _blocks(p.cfg)}
    print("n_col %d %s: taped vs recomputed %.3e, worst block %s %.3e" % (n_col, ma, _rel(g_tape, g_rec.astype(np.float64)),
                                                                         max(errs, key=errs.get), max(errs.values())))
    assert _rel(g_tape, g_rec.astype(np.float64)) < whole
    for name, e in errs.items():
        assert e < per_block, (name, e)


@pytest.mark.parametrize("n_col,block", CASES)
def test_consecutive_calls_are_bit_identical(n_col, block, monkeypatch):
    """Two loss_grad calls on one handle write and read the same tape buffers: nothing of the first call's record may leak into the second."""
    (t1, e1, g1), (t2, e2, g2) = _loss_grad(monkeypatch, n_col, block, "bf16x3_exact", calls=2)
    assert t1 == t2 and np.array_equal(e1, e2) and np.array_equal(g1, g2)
