"""Inputs on which a training kernel can be told from a subtly wrong one (tests/test_distinct_nets_host.py, tests/test_gpu_distinct_nets.py).

`synthetic.make_weights(..., same_init=True)`, the weights of every other parity test of the training engines, gives the three flux nets the same
draw and zero biases and, divided by 1e2, pre-activations below 0.05: a wrong per-net offset, a dropped bias add or an activation curve that is
wrong away from 0 computes the same numbers there.  `weights` draws the nets separately (`same_init=False`), undivided, and overwrites every bias
block with bias * U(-1, 1).  The block layout is read off `O.unpack` / `O.pack_grads` (an index vector pushed through them), not stated a second
time.

The reference cases are computed once per process by the float64 oracle and shared read-only: problem, weights, the float32 truth of `O.solve` at
a second draw of the same kind, and the oracle's total, terms, gradient and solution."""
import functools
from types import SimpleNamespace

import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O

WM_SC = np.array([1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3])               # the scalings of tests/test_gpu_parity.py's wind-mixing tests
WM_SC.setflags(write=False)
NET_NAMES = ("uw", "vw", "wT")
FRAMES, SUBSTEPS = 5, 2
ACTS = ("mish", "swish", "tanh")
WM_SEED = 1                                                       # weights: this seed; truth: the next
SCHEDULE = (2, 3, 2, 4)
FC_SEEDS = (5, 6, 7, 8, 9)                                        # relu kinks: the first seed on which the float32 C port is within a tenth of the bounds
FC_SEED = {(32, False): 5, (64, False): 5, (32, True): 5, "conv": 5}   # ... asserted to be that seed by tests/test_distinct_nets_host.py


def n_nets(cfg):
    return 3 if cfg.model == O.WIND_MIXING else 1


@functools.lru_cache(maxsize=None)
def _blocks(layer_sizes, nn):
    P = nn * sum(layer_sizes[i] * layer_sizes[i + 1] + layer_sizes[i + 1] for i in range(len(layer_sizes) - 1))
    idx = np.arange(P, dtype=np.float64)
    nets = O.unpack(idx, layer_sizes, nn)
    assert np.array_equal(O.pack_grads(nets), idx)                  # pack_grads inverts unpack: one layout for the weights and the gradient
    out = []
    for k, layers in enumerate(nets):
        for l, (W, b) in enumerate(layers):
            for kind, a in (("W", W), ("b", b)):
                ix = np.sort(a.reshape(-1)).astype(np.int64)
                assert np.array_equal(ix, np.arange(ix[0], ix[0] + ix.size))
                out.append((k, l, kind, slice(int(ix[0]), int(ix[0] + ix.size))))
    assert sum(s.stop - s.start for *_, s in out) == P
    return tuple(out)


def blocks(cfg):
    """((net, layer, "W" | "b", slice), ...) of the parameter vector, in `O.unpack`'s order"""
    return _blocks(tuple(cfg.layer_sizes), n_nets(cfg))


def named_blocks(cfg):
    """((name, slice), ...): "uw/W1", "uw/b1", ... "wT/b3" (a T-only model: "W1" ... "b3")"""
    one = n_nets(cfg) == 1
    return tuple((("" if one else NET_NAMES[k] + "/") + "%s%d" % (kind, l + 1), s) for k, l, kind, s in blocks(cfg))


def assert_distinct_and_biased(cfg, w):
    """the nets differ pairwise in every block; no bias is zero"""
    bl = blocks(cfg)
    for k, l, kind, s in bl:
        if kind == "b":
            assert (w[s] != 0).all(), (k, l)
        for k2, l2, kind2, s2 in bl:
            if k2 > k and (l2, kind2) == (l, kind):
                assert (w[s] != w[s2]).mean() > 0.99, (k, k2, l, kind)


def weights(cfg, seed, divisor=1.0, bias=1.0):
    """distinct nets (`make_weights(..., same_init=False)` / divisor) with every bias block bias * U(-1, 1); float32"""
    rng = synthetic._rng(synthetic.SEED + 1000 + int(seed), 9)
    w = synthetic.make_weights(rng, cfg, divisor, same_init=False).astype(np.float64)
    for k, l, kind, s in blocks(cfg):
        if kind == "b":
            b = rng.uniform(-1.0, 1.0, size=s.stop - s.start)
            w[s] = bias * np.where(b == 0, 0.5, b)
    w = w.astype(np.float32)
    assert_distinct_and_biased(cfg, w)
    return w


def block_errors(got, ref, named):
    """[(name, relative L2 error of the block, the block's share of ||ref||)] for the blocks `named` (`named_blocks(cfg)`, a case's `.blocks`)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == (named[-1][1].stop,)
    nrm = np.linalg.norm(ref)
    return [(name, float(np.linalg.norm(got[s] - ref[s]) / (np.linalg.norm(ref[s]) + 1e-300)), float(np.linalg.norm(ref[s]) / nrm)) for name, s in named]


def worst_block(got, ref, named):
    """(name, error) of the block with the largest relative error"""
    name, e, _ = max(block_errors(got, ref, named), key=lambda t: t[1])
    return name, e


def stage_inputs(cfg, x0, bcs, w):
    """every state at which the float64 oracle's solve evaluates the right-hand side: [stage evaluations * columns, n_state]"""
    m = O.Model(cfg)
    nets = m.unpack(w)
    b = np.asarray(bcs, np.float64)
    _, tape = O.solve(cfg, x0, bcs, w, return_tape=True)
    if getattr(cfg, "stepper", "rk4") == "rkc2":
        return np.concatenate([Y for Ys in tape for Y in Ys])
    out = []
    for x, (t, dt, _) in zip(tape, O._step_times(cfg)):
        X2 = x + dt / 2 * m.rhs(x, b, nets, t)
        X3 = x + dt / 2 * m.rhs(X2, b, nets, t + dt / 2)
        X4 = x + dt * m.rhs(X3, b, nets, t + dt / 2)
        out += [x, X2, X3, X4]
    return np.concatenate(out)


def preactivations(cfg, w, X):
    """{(net, hidden layer): z [len(X), width]} at the states X, from `O.mlp_forward`'s own tape (the output layer is the identity)"""
    m = O.Model(cfg)
    out = {}
    for k, layers in enumerate(m.unpack(w)):
        _, tape = O.mlp_forward(layers, m.acts, np.asarray(X, np.float64))
        for l in range(len(layers) - 1):
            out[(k, l)] = tape[l][1]
    return out


def swap_nets(cfg, w, a, b):
    """w with the parameter slices of nets a and b exchanged"""
    out = np.array(w)
    where = {(k, l, kind): s for k, l, kind, s in blocks(cfg)}
    for (k, l, kind), s in where.items():
        if k == a:
            s2 = where[(b, l, kind)]
            out[s], out[s2] = w[s2], w[s]
    return out


def zero_biases(cfg, w):
    out = np.array(w)
    for k, l, kind, s in blocks(cfg):
        if kind == "b":
            out[s] = 0
    return out


def _freeze(case):
    for a in list(vars(case).values()) + [case.p.x0, case.p.bcs]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _reference(p, cfg, w, w_truth, sc, **extra):
    truth = O.solve(cfg, p.x0, p.bcs, w_truth).astype(np.float32)
    tot, terms, g, sol = O.loss_and_grad(cfg, p.x0, p.bcs, w, truth, sc)
    assert np.isfinite(sol).all() and np.isfinite(g).all() and np.isfinite(terms).all()
    extra.setdefault("blocks", named_blocks(cfg))
    return _freeze(SimpleNamespace(p=p, cfg=cfg, w=w, w_truth=w_truth, truth=truth, sc=np.array(sc, np.float64), tot=float(tot), terms=terms, g=g, sol=sol,
                                   **extra))


@functools.lru_cache(maxsize=None)
def wm_case(act, n, stepper="rk4", member=None):
    """wind mixing: n columns, 5 frames, 2 sub-steps, activations (act, act, identity).  member = k: ensemble member k's case — weights of seed 20 + k,
    the closure constants of row k of tests/test_gpu_ensemble.py's PHYS and that file's scalings; the truth is the plain case's (the second draw)."""
    p = synthetic.wind_mixing_problem(n, n_frames=FRAMES, substeps=SUBSTEPS, weight_divisor=1e2, activations=(act, act, "identity"))
    cfg = p.cfg if stepper == "rk4" else p.cfg.with_(stepper=stepper)
    w_truth = weights(cfg, WM_SEED + 1)
    if member is None:
        return _reference(p, cfg, weights(cfg, WM_SEED), w_truth, WM_SC)
    from tests.test_gpu_ensemble import PHYS, SC, _model_cfg
    return _reference(p, _model_cfg(cfg, PHYS[member]), weights(cfg, 20 + member), w_truth, np.array(SC, np.float64))


def oracle_under_schedule(schedule, call):
    """call() with the oracle stepping save interval i in schedule[i] steps (tests/schedule_common.py's replacement of `_step_times`)"""
    from tests import schedule_common as C
    saved = O._step_times
    O._step_times = C.schedule_step_times(schedule)
    try:
        return call()
    finally:
        O._step_times = saved


@functools.lru_cache(maxsize=None)
def wm_schedule_case(act, n, schedule=SCHEDULE):
    """`wm_case(act, n)` stepped with schedule[i] RK4 steps in save interval i; the truth stays the uniform solve's"""
    b = wm_case(act, n)
    tot, terms, g, sol = oracle_under_schedule(schedule, lambda: O.loss_and_grad(b.cfg, b.p.x0, b.p.bcs, b.w, b.truth, WM_SC))
    return _freeze(SimpleNamespace(p=b.p, cfg=b.cfg, w=b.w, w_truth=b.w_truth, truth=b.truth, sc=b.sc, tot=float(tot), terms=terms, g=g, sol=sol,
                                   blocks=b.blocks, schedule=tuple(schedule)))


@functools.lru_cache(maxsize=None)
def fc_case(Nz, ca, seed=None, n=19):
    """free convection: 19 columns, 5 save points to t = 0.01, relu nets / 10 with biases 0.3 U(-1, 1); ca: ConvectiveAdjustmentNDE at 20 RK4 sub-steps"""
    seed = FC_SEED[(Nz, ca)] if seed is None else seed
    p = synthetic.free_convection_problem(n, Nz=Nz, n_save=FRAMES, substeps=20 if ca else SUBSTEPS, convective_adjustment=ca, t_end=0.01)
    return _reference(p, p.cfg, weights(p.cfg, seed, 10.0, 0.3), weights(p.cfg, seed + 100, 10.0, 0.3), O.default_loss_scalings(p.cfg), seed=seed)


@functools.lru_cache(maxsize=None)
def conv_case(Nz=32, c=3, seed=None, n=19):
    """the `--conv c` network on the same columns: `synthetic.free_convection_conv_problem`'s filter and its non-zero filter bias (0.05) in front of
    the dense layers of `weights(..., 10, 0.3)`; the oracle runs the equivalent Toeplitz network (tests/conv_cases.py) and folds its gradient back"""
    from tests import conv_cases as CC
    seed = FC_SEED["conv"] if seed is None else seed
    p = synthetic.free_convection_conv_problem(n, c, Nz=Nz, n_save=FRAMES, substeps=SUBSTEPS, t_end=0.01)
    tail = p.cfg.with_(layer_sizes=(Nz - c + 1, 4 * Nz, 4 * Nz, Nz - 1))

    def theta(front, s):
        return np.concatenate([front[:c + 1], weights(tail, s, 10.0, 0.3)]).astype(np.float32)
    w, w_truth = theta(p.weights, seed), theta(p.weights_truth, seed + 100)
    assert w[c] != 0 and w.shape == p.weights.shape
    dc = CC.dense_cfg(p.cfg, c)
    from colnde.free_convection import conv_to_dense
    truth = O.solve(dc, p.x0, p.bcs, conv_to_dense(w_truth.astype(np.float64), Nz, c)).astype(np.float32)
    tot, g, sol = CC.oracle_loss_grad(p.cfg, c, p.x0, p.bcs, w, truth)
    sc = O.default_loss_scalings(p.cfg)
    named = tuple((name, slice(a, b)) for name, a, b in CC.blocks(Nz, c))
    return _freeze(SimpleNamespace(p=p, cfg=p.cfg, w=w, w_truth=w_truth, truth=truth, sc=sc, tot=float(tot), terms=np.array([0, 0, tot, 0, 0, 0.0]), g=g, sol=sol,
                                   blocks=named, conv=c, dense_cfg=dc, seed=seed))


# every reference case tests/test_gpu_distinct_nets.py uses, by name (tests/test_distinct_nets_host.py checks each of them)
WM_CASES = {"%s/%d" % (a, n): functools.partial(wm_case, a, n) for n in (21, 70) for a in ACTS}
WM_CASES.update({"mish/1": functools.partial(wm_case, "mish", 1), "mish/21/rkc2": functools.partial(wm_case, "mish", 21, "rkc2"),
                 "mish/21/schedule": functools.partial(wm_schedule_case, "mish", 21),
                 "mish/8/member1": functools.partial(wm_case, "mish", 8, "rk4", 1), "mish/40/member1": functools.partial(wm_case, "mish", 40, "rk4", 1)})
FC_CASES = {"fc/32": functools.partial(fc_case, 32, False), "fc/64": functools.partial(fc_case, 64, False), "ca/32": functools.partial(fc_case, 32, True),
            "conv3/32": conv_case}
