"""The regtile engine's Z1 tape record, stacked by net: a net's twelve full quads of hidden features (0 .. 47) are three whole layer-1 tiles of the forward
kernel, read by the adjoint as six 16-byte loads; the three nets' last quads (features 48, 49) share one tile and are read by one 4-byte load each.  Layer 2
sees the hidden features only through W2, so a W2 that is zero except chosen columns makes the chosen part of the record the only thing the layer-2 and
layer-3 gradient blocks can see: a mis-addressed element cannot hide behind the 48 others.  33 columns = one full 32-column tile and a ragged one, both
16-column halves of the first; 2 save points x 2 sub-steps = 8 records per tile; mish and relu; both matrix arithmetics.

Tolerance: the rule of tests/test_gpu_z1_tape_record.py (the float32 engine against the float64 oracle), but not its constant, which was measured on dense
weights.  Here the bound is a multiple of the float32 ORACLE's own distance from the float64 oracle on the same weights: the same algorithm in the same
precision, differing from the engine in the order of its additions only (MFMA trees, the exact bf16 split, fixed-order reductions), so the two distances are
of one order of magnitude.  Bound = 10 x the worst layer block of the float32 oracle, for every block."""
import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.nde import ENGINE_REGTILE
from oracle import nde_oracle as O
from tests.test_gpu_parity import _rel

pytestmark = pytest.mark.gpu

N_COL = 33
ACTS = ["mish", "relu"]
ARITHMETICS = ["bf16x3_exact", "f32_mfma"]
SCALINGS = np.array([1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3])
KEEP = {"last_quad": (48, 49), "full_quads": (0, 1, 2, 3, 44, 45, 46, 47)}      # hidden features whose W2 columns stay
F32_MULTIPLE = 10.0

_problems, _oracle = {}, {}


def _problem(act):
    if act not in _problems:
        p = synthetic.wind_mixing_problem(N_COL, n_frames=2, substeps=2, weight_divisor=1e2, activations=(act, act, "identity"))
        truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
        _problems[act] = (p, truth)
    return _problems[act]


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


def _weights(p, keep, net):
    """p.weights with every net's W2 zero, except the columns `keep` (hidden features) of net `net`.  W2 is stored input-major: [feature][output]."""
    w = p.weights.copy()
    s = p.cfg.layer_sizes
    for name, sl in _blocks(p.cfg):
        if name.endswith("/W2"):
            W2 = w[sl].reshape(s[1], s[2])
            kept = W2[list(keep)].copy()
            W2[:] = 0.0
            if name == "net%d/W2" % net:
                W2[list(keep)] = kept
    return w


def _case(act, kind, net):
    """Weights, float64 oracle gradient and the bound from the float32 oracle: computed once per (activation, kept features, net)."""
    key = (act, kind, net)
    if key not in _oracle:
        p, truth = _problem(act)
        w = _weights(p, KEEP[kind], net)
        g64 = O.loss_and_grad(p.cfg, p.x0, p.bcs, w, truth, SCALINGS)[2]
        g32 = O.loss_and_grad(p.cfg, p.x0, p.bcs, w, truth, SCALINGS, dtype=np.float32)[2]
        bound = F32_MULTIPLE * max(_rel(g32[s], g64[s]) for _, s in _blocks(p.cfg))
        for a in (w, g64):
            a.setflags(write=False)
        _oracle[key] = (w, g64, bound)
    return _oracle[key]


def _loss_grad(monkeypatch, act, ma, w, calls=1):
    p, truth = _problem(act)
    monkeypatch.setenv("COLNDE_RT_ZTAPE", "1")
    monkeypatch.delenv("COLNDE_RT_BLOCK", raising=False)
    with colnde.ColumnNDE(p.cfg, p.n_columns, engine=ENGINE_REGTILE, matrix_arithmetic=ma) as nde:
        assert nde.engine == ENGINE_REGTILE
        nde.set_problem(p.x0, p.bcs, truth)
        res = [nde.loss_grad(w, SCALINGS) for _ in range(calls)]
        plan = nde.plan()
    assert plan["z1_taped"] and plan["matrix_arithmetic"] == ma
    return res if calls > 1 else res[0]


def _check_blocks(monkeypatch, act, ma, kind, net):
    p = _problem(act)[0]
    w, g64, bound = _case(act, kind, net)
    _, _, g = _loss_grad(monkeypatch, act, ma, w)
    assert np.isfinite(g).all()
    errs = {name: _rel(g[s], g64[s]) for name, s in _blocks(p.cfg)}
    print("%s %s %s net %d: worst block %s %.3e, bound %.3e (float32 oracle's worst block %.3e)"
          % (act, ma, kind, net, max(errs, key=errs.get), max(errs.values()), bound, bound / F32_MULTIPLE))
    # the part of the record under test reaches layers 2 and 3 of `net`: their blocks must not be trivially zero
    for name, s in _blocks(p.cfg):
        if name in ("net%d/W3" % net, "net%d/b2" % net):
            assert np.linalg.norm(g64[s]) > 0
    for name, e in errs.items():
        assert e <= bound, (name, e, bound)


@pytest.mark.parametrize("ma", ARITHMETICS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("net", [0, 1, 2])
def test_last_quad_alone_feeds_layers_2_and_3(net, act, ma, monkeypatch):
    """(i) W2 zero except the columns of features 48, 49 of one net: the adjoint's only 4-byte load (element `net` of tile 9's first group) is all that the
    net's layer-2 and layer-3 blocks see of the record; every layer block of every net against the float64 oracle."""
    _check_blocks(monkeypatch, act, ma, "last_quad", net)


@pytest.mark.parametrize("ma", ARITHMETICS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("net", [0, 1, 2])
def test_first_and_last_full_quads_alone_feed_layers_2_and_3(net, act, ma, monkeypatch):
    """(ii) the same with features 0 .. 3 and 44 .. 47: the first and the last full quad of the net's three tiles."""
    _check_blocks(monkeypatch, act, ma, "full_quads", net)


@pytest.mark.parametrize("ma", ARITHMETICS)
@pytest.mark.parametrize("act", ACTS)
def test_three_calls_are_bit_identical(act, ma, monkeypatch):
    """(iii) three loss_grad calls on one handle: a record element consumed before its load has landed holds the previous stage's or call's value, and shows
    as a difference between calls."""
    p = _problem(act)[0]
    r = _loss_grad(monkeypatch, act, ma, p.weights, calls=3)
    for t, e, g in r[1:]:
        assert t == r[0][0] and np.array_equal(e, r[0][1]) and np.array_equal(g, r[0][2])
