"""Wind-mixing cases whose hidden pre-activations sit in the TAILS of the five activations (tests/test_activation_range_host.py,
tests/test_gpu_activation_range.py): at the clamps of mish (20) and tanh (+-15), where swish's exp(-z) overflows (ln FLT_MAX = 88.72), where exp(z) is
a float32 subnormal, at |z| = 120, and within 1e-3 of the relu / leakyrelu kink.

A case is a tests/distinct_nets.py case (distinct nets, `D.weights`, `D._reference`) with three changes, all made through `D.blocks` and an index
vector pushed through `O.unpack` (the parameter layout is not stated here): every hidden bias block is overwritten by a LADDER of pre-activations;
the rows of the weight matrices that feed a ladder unit are scaled down so that the unit's z stays at its rung over the whole solve (an ordinary
unit keeps its row, W1 / 4 overall, and moves within [-3, 3]); and the layers behind a hidden layer are scaled down (W2 / 30, the output layer / 3e3: a
saturated mish, relu or swish unit emits its z, 120) so that the nets' outputs keep the size the other parity tests have.  The truth is an ordinary
`D.weights(cfg, seed, divisor=1e2)` draw: the loss is not near zero.

The per-unit check of the hidden bias gradients (`per_unit_errors`; dL/db_j = act'(z_j) (...) shows the derivative unit by unit, where a block norm
is dominated by the unsaturated units): entries with |ref_j| >= 1e-3 max|ref| of their block agree relatively to PER_UNIT, the others absolutely to
PER_UNIT * 1e-3 max|ref|.

PER_UNIT = 1.2e-03: ten times the float32 restatement's own worst per-entry error over the committed 96-50-20-31 cases (WM_CASES under the C port,
VARIANT_CASES under the float32 NumPy oracle), rounded up by a quarter.  Measured by
tests/test_activation_range_host.py::test_per_unit_figure_is_ten_times_the_ports_worst: 9.5e-05 (PORT_WORST; swish at 70 columns, vw/b1, an ordinary
unit of the absolute class whose entry is a sum over columns and stages that cancels to just under 1e-3 of the block's largest; tanh: 5.6e-05, 1 - t^2 of
a saturated unit, a difference of two float32 numbers next to 1).
That test fails if the port's worst leaves [PER_UNIT / 20, PER_UNIT / 10] or moves away from PORT_WORST by a quarter."""
import functools

import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O
from tests import distinct_nets as D

ACTS = ("relu", "mish", "swish", "tanh", "leakyrelu")
SEED = 31                                                         # weights: this seed; truth: the next, / 1e2
W1_SCALE, W2_SCALE, OUT_SCALE = 1.0 / 4, 1.0 / 30, 1.0 / 3e3     # ordinary rows of layer 1; layer 2 (and every further hidden layer); the output layer
RUNG, KINK = 0.05, 2e-5                                           # further scale of a row that feeds a rung of width ~1; a rung at the kink
PER_UNIT = 1.2e-3
PORT_WORST = 9.5e-5

# rungs: (pre-activation, row scale).  The intervals tests/test_activation_range_host.py asserts, per activation (REQUIRED below).
_BIG = ((120.0, RUNG), (-120.0, RUNG), (104.0, RUNG), (-104.5, RUNG))
RUNGS = {
    "mish": _BIG + ((19.5, RUNG), (20.5, RUNG), (45.0, RUNG), (-20.0, RUNG), (-95.0, RUNG), (-12.0, RUNG), (30.0, RUNG)),
    "tanh": _BIG + ((14.5, RUNG), (15.5, RUNG), (-14.5, RUNG), (-15.5, RUNG), (7.0, RUNG), (-7.0, RUNG), (5.6, RUNG), (-5.6, RUNG)),
    "swish": _BIG + ((-89.4, RUNG), (-87.9, RUNG), (35.0, RUNG), (-30.0, RUNG), (-88.5, RUNG), (-89.0, RUNG), (60.0, RUNG)),
    "relu": _BIG + ((5e-4, KINK), (-5e-4, KINK), (2e-4, KINK), (-2e-4, KINK), (8e-4, KINK), (-8e-4, KINK)),
}
RUNGS["leakyrelu"] = RUNGS["relu"]

# (lo, hi, how many units at least stay inside at EVERY stage evaluation); a fraction: that share of the layer
_EVERY = ((-3.0, 3.0, 1.0 / 3), (100.0, np.inf, 1), (-np.inf, -100.0, 1))
REQUIRED = {
    "mish": _EVERY + ((19.0, 20.0, 1), (20.0, 21.0, 1), (40.0, np.inf, 1), (-30.0, -10.0, 1), (-104.0, -87.4, 1)),
    "tanh": _EVERY + ((14.0, 15.0, 1), (15.0, 16.0, 1), (-15.0, -14.0, 1), (-16.0, -15.0, 1), (5.0, 9.0, 1), (-9.0, -5.0, 1)),
    "swish": _EVERY + ((-90.0, -88.73, 1), (-88.72, -87.0, 1), (30.0, np.inf, 1)),
    "relu": _EVERY + ((1e-4, 1e-3, 1), (-1e-3, -1e-4, 1)),
}
REQUIRED["leakyrelu"] = REQUIRED["relu"]


def ladder(act, width, net=0):
    """(pre-activations [width], row scales [width]): the rungs of `act` and ordinary units behind them, the whole rolled by 7 units per net and the
    ordinary units shifted by 0.05 per net (the nets stay distinct in every block).  The ordinary units are spread over [-2, 2] (relu, leakyrelu:
    over 0.9 <= |z| <= 2.1, so that with rows of W1_SCALE no unit reaches its kink) with rows of scale 1."""
    rungs = RUNGS[act][:max(0, min(len(RUNGS[act]), width - (width + 2) // 3 - 1))]
    m = width - len(rungs)
    if act in ("relu", "leakyrelu"):
        mag = np.linspace(0.9, 2.0, (m + 1) // 2)
        rest = np.concatenate([mag + 0.05 * net, -mag[:m // 2] - 0.05 * net])
    else:
        rest = np.linspace(-2.0, 2.0, m) + 0.013 + 0.05 * net       # no unit exactly at 0
    z = np.roll(np.concatenate([[v for v, _ in rungs], rest]), 7 * net)
    s = np.roll(np.concatenate([[r for _, r in rungs], np.ones(m)]), 7 * net)
    assert z.shape == s.shape == (width,)
    return z, s


@functools.lru_cache(maxsize=None)
def _rows(layer_sizes, nn):
    """{(net, layer): index matrix [n_out, n_in] of the weight block}, from `O.unpack` of an index vector"""
    P = nn * sum(layer_sizes[i] * layer_sizes[i + 1] + layer_sizes[i + 1] for i in range(len(layer_sizes) - 1))
    nets = O.unpack(np.arange(P, dtype=np.float64), layer_sizes, nn)
    return {(k, l): W.astype(np.int64) for k, layers in enumerate(nets) for l, (W, _) in enumerate(layers)}


FORWARD_OUT_SCALE = 1.0 / 30                                     # the output layer of a net that is evaluated, not integrated (`forward_weights`)


def weights(cfg, seed, act, out_scale=OUT_SCALE):
    """`D.weights(cfg, seed)` with the ladders in the hidden bias blocks and the rows and layers scaled as the module's docstring says; float32"""
    w = D.weights(cfg, seed).astype(np.float64)
    sizes = tuple(cfg.layer_sizes)
    rows = _rows(sizes, D.n_nets(cfg))
    last = len(sizes) - 2
    for k, l, kind, s in D.blocks(cfg):
        if l == last:
            if kind == "W":
                w[s] *= out_scale
            continue
        z, scale = ladder(act, sizes[l + 1], k)
        if kind == "b":
            w[s] = z
        else:
            w[rows[(k, l)]] *= (W1_SCALE if l == 0 else W2_SCALE) * scale[:, None]
    w = w.astype(np.float32)
    D.assert_distinct_and_biased(cfg, w)
    return w


def forward_weights(cfg, act, seed=SEED):
    """the same nets for the forward-only kernel families: nothing is integrated there, so the output layer is scaled by 1 / 30 only and a saturated
    unit (120 x 0.3 / 30) weighs as much in a net's output as the output bias does; behind / 3e3 an activation error would be 100 times fainter"""
    return weights(cfg, seed, act, FORWARD_OUT_SCALE)


def hidden_bias_blocks(c):
    """((name, slice), ...) of the case's hidden bias blocks"""
    last = len(c.cfg.layer_sizes) - 2
    return tuple((name, s) for (name, s), (k, l, kind, _) in zip(c.blocks, D.blocks(c.cfg)) if kind == "b" and l < last)


def per_unit_errors(got, ref, c):
    """[(block, worst relative error among the entries with |ref| >= 1e-3 max|ref|, worst |error| of the others / (1e-3 max|ref|), how many are in the
    relative class)] over the hidden bias blocks; both figures are held to PER_UNIT"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = []
    for name, s in hidden_bias_blocks(c):
        g, r = got[s], ref[s]
        floor = 1e-3 * np.abs(r).max()
        big = np.abs(r) >= floor
        assert floor > 0 and big.any()
        rel = float((np.abs(g - r)[big] / np.abs(r[big])).max())
        small = float((np.abs(g - r)[~big] / floor).max()) if (~big).any() else 0.0
        out.append((name, rel, small, int(big.sum())))
    return out


def worst_per_unit(got, ref, c):
    """(block, the larger of its two per-unit figures) of the worst hidden bias block"""
    name, rel, small, _ = max(per_unit_errors(got, ref, c), key=lambda t: max(t[1], t[2]))
    return name, max(rel, small)


@functools.lru_cache(maxsize=None)
def wm_case(act, n, stepper="rk4", layer_sizes=None, frames=D.FRAMES):
    """wind mixing on the ladders of `act`: n columns, `frames` frames, 2 sub-steps, activations act on every hidden layer"""
    sizes = (96, 50, 20, 31) if layer_sizes is None else tuple(layer_sizes)
    acts = (act,) * (len(sizes) - 2) + ("identity",)
    p = synthetic.wind_mixing_problem(n, n_frames=frames, substeps=D.SUBSTEPS, weight_divisor=1e2, layer_sizes=sizes, activations=acts)
    cfg = p.cfg if stepper == "rk4" else p.cfg.with_(stepper=stepper)
    return D._reference(p, cfg, weights(cfg, SEED, act), D.weights(cfg, SEED + 1, divisor=1e2), D.WM_SC, act=act)


@functools.lru_cache(maxsize=None)
def wm_schedule_case(act, n, schedule=D.SCHEDULE):
    """`wm_case(act, n)` stepped with schedule[i] RK4 steps in save interval i; the truth stays the uniform solve's"""
    from types import SimpleNamespace
    b = wm_case(act, n)
    tot, terms, g, sol = D.oracle_under_schedule(schedule, lambda: O.loss_and_grad(b.cfg, b.p.x0, b.p.bcs, b.w, b.truth, D.WM_SC))
    return D._freeze(SimpleNamespace(p=b.p, cfg=b.cfg, w=b.w, w_truth=b.w_truth, truth=b.truth, sc=b.sc, tot=float(tot), terms=terms, g=g, sol=sol,
                                     blocks=b.blocks, schedule=tuple(schedule), act=act))


# every case tests/test_gpu_activation_range.py holds to the oracle, by name (tests/test_activation_range_host.py checks each of them).
# WM_CASES: 96-50-20-31 under RK4, the ones the C port restates; they and VARIANT_CASES (float32 NumPy oracle: the port has neither RKC2 nor a
# schedule) carry the per-unit check and give PER_UNIT.  WIDE_CASES: the other tile16 kernel forms, ladders on the 400-wide layers, 8 columns, 4 frames.
WM_CASES = {"%s/%d" % (a, n): functools.partial(wm_case, a, n) for n in (21, 70) for a in ACTS}
VARIANT_CASES = {"swish/21/rkc2": functools.partial(wm_case, "swish", 21, "rkc2"), "relu/21/schedule": functools.partial(wm_schedule_case, "relu", 21)}
WIDE_SHAPES = {"96-400-31": (96, 400, 31), "96-400-400-31": (96, 400, 400, 31)}
WIDE_ACTS = ("mish", "swish")
WIDE_N, WIDE_FRAMES = 8, 4
WIDE_CASES = {"%s/%s/%d" % (a, nm, WIDE_N): functools.partial(wm_case, a, WIDE_N, "rk4", sz, WIDE_FRAMES) for nm, sz in WIDE_SHAPES.items() for a in WIDE_ACTS}


# ---- the forward-only kernel families on the same ladders (`forward_weights`) ------------------------------------------------------------------
FORWARD_N = (8, 17)
EMBED_ACTS = ("tanh", "swish")                                     # colnde_wm_infer_dz_flux on 96-50-20-31 (csrc/wm_net_layer1.inc, wm_net_layer23.inc)
GENERIC_SHAPE, GENERIC_ACTS = (96, 400, 31), ("relu", "leakyrelu")  # the any-architecture embedding (csrc/engine_wm_embed_any.hip); tanh: the NaN case
PROFILE_ACT = "mish"                                               # colnde_ensemble_profile (csrc/engine_wm_profile.hip)
PRETRAIN_ACTS, PRETRAIN_NET, PRETRAIN_GS = ("mish", "tanh"), 1, 1e-2   # colnde_pretrain_flux_dev (csrc/pretrain_sample.h): the vw net


@functools.lru_cache(maxsize=None)
def embed_case(act, layer_sizes=(96, 50, 20, 31)):
    """17 columns of the embedding's inputs (tests/wm_embed_common.py) with the ladder nets and their float64 forcings: SimpleNamespace(p, w, u, v, T,
    top, ref) — the fields tests/wm_generic_cases.py's `case` has, and the three dz arrays"""
    from types import SimpleNamespace
    from tests import wm_embed_common as W
    sizes = tuple(layer_sizes)
    p = synthetic.wind_mixing_problem(max(FORWARD_N), n_frames=3, weight_divisor=1.0, layer_sizes=sizes, activations=(act,) * (len(sizes) - 2) + ("identity",))
    u, v, T, top = W.embed_inputs(p)
    w = forward_weights(p.cfg, act)
    ref = W.dz_fluxes(p.cfg, w, u, v, T, top, W.LZ)
    return D._freeze(SimpleNamespace(p=p, w=w, u=u, v=v, T=T, top=top, ref=ref, act=act))


def first_columns(c, n):
    """the first n columns of an `embed_case`, contiguous"""
    from types import SimpleNamespace
    cut = lambda a: np.ascontiguousarray(a[:n])
    return SimpleNamespace(p=c.p, w=c.w, u=cut(c.u), v=cut(c.v), T=cut(c.T), top=np.ascontiguousarray(c.top[:, :n]), ref=tuple(r[:n] for r in c.ref))


@functools.lru_cache(maxsize=None)
def profile_case(n):
    """the saved states of `wm_case(PROFILE_ACT, n)` as float32 and two members' ladder nets (`forward_weights`, seeds SEED and SEED + 5) for
    colnde_ensemble_profile with the closure's constants at 0 (the networks' own share of the fluxes): SimpleNamespace(p, cfg, W, rows, sol, truth)"""
    from types import SimpleNamespace
    c = wm_case(PROFILE_ACT, n)
    W = np.stack([forward_weights(c.cfg, PROFILE_ACT), forward_weights(c.cfg, PROFILE_ACT, SEED + 5)])
    rows = np.array([[0.0, 0.0, 1.0, 0.25, 1.0], [0.0, 0.0, 0.8, 0.2, 1.2]], np.float32)
    return D._freeze(SimpleNamespace(p=c.p, cfg=c.cfg, W=W, rows=rows, sol=np.stack([c.sol.astype(np.float32)] * 2), truth=c.truth))


@functools.lru_cache(maxsize=None)
def pretrain_case(act, n):
    """n samples of flux pre-training (tests/pretrain_cases.py's `data`) for the vw net of the ladder nets, in `sample`'s fields, and the float64
    reference of ONE call over the samples in order with beta = (0.5, 0.5) and eta = 0 from zero moments: m = sum_i 2^-(n - i) g_i, mean loss"""
    from types import SimpleNamespace
    from tests import pretrain_cases as PC
    p = synthetic.wind_mixing_problem(1, n_frames=max(2, n), weight_divisor=1.0, activations=(act, act, "identity"))
    X, B, Y = PC.data(p, n)
    X, B, Y = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, B, Y[PRETRAIN_NET]))
    s = SimpleNamespace(case="activation_range/%s/%d" % (act, n), p=p, cfg=p.cfg, k=PRETRAIN_NET, gs=PRETRAIN_GS, theta=forward_weights(p.cfg, act), X=X, B=B, Y=Y,
                        net=PC._net(p.cfg, PRETRAIN_NET), act=act)
    s.m_ref, s.loss_ref = pretrain_moment(s, PC.oracle_loss_grad)
    return D._freeze(s)


def pretrain_moment(s, loss_grad, dtype=np.float64):
    """(m, mean loss) of that call under `loss_grad(s, theta_net, i)` (tests/pretrain_cases.py: `oracle_loss_grad`, `f32_loss_grad`)"""
    m, losses = np.zeros(s.net.stop - s.net.start, dtype), []
    for i in range(s.X.shape[0]):
        loss, g = loss_grad(s, s.theta[s.net], i)
        m = dtype(0.5) * m + dtype(0.5) * np.asarray(g, dtype)
        losses.append(loss)
    return m, float(np.mean(losses))
