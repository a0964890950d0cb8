"""Shared by tests/test_fc_pretrain_host.py (CPU) and tests/test_gpu_fc_pretrain.py (GPU): the samples, weights and float64 references of the ensemble
T -> wT pre-training (`colnde_ensemble_pretrain_flux_dev`; free_convection/train_free_convection_nde.jl:182-216), and a float32 restatement of the
whole per-sample chain — flux, loss with the causality penalty, gradient, Flux ADAM and Descent — from which the GPU tolerances are derived without
the kernel.  No GPU and no torch needed here.

The float64 reference of the plain network is `O.nn_pretrain_loss_and_grad` with gradient_scaling = 0; of the `--conv c` network the same oracle on
`conv_to_dense(theta)` (`conv_dense_layer_sizes`: the filter as a Toeplitz first layer), its gradient folded back by `conv_grad_from_dense`.  The penalty
and Descent are closed formulas: loss += c sum_{r<q} W1[r, q]^2, gradient[W1[r, q]] += 2 c W1[r, q]; theta -= eta g."""
import functools
from types import SimpleNamespace

import numpy as np

from colnde import synthetic
from colnde.free_convection import conv_dense_layer_sizes, conv_grad_from_dense, conv_n_params, conv_to_dense, pretrain_orders
from oracle import nde_oracle as O
from tests import pretrain_cases as PC

CONV_ACTS = ("relu", "relu", "relu", "identity")
SEQ_N = PC.SEQ_N                              # samples of the sequence and driver cases
SEQ_ORDER = PC.SEQ_ORDER                      # (3, 3, 0, 1, 1, 5, 7, 2): repeats, and not every sample
ETA_ADAM, ETA_DESCENT = 1e-3, 1e-2            # ADAM() and Descent(1e-2) of the driver


def handle_cfg(Nz):
    """What the handles of the GPU tests are created with: one column, n_save = 3."""
    return synthetic.free_convection_problem(1, Nz=Nz, n_save=3, substeps=2, t_end=0.01).cfg


def oracle_cfg(cfg, c):
    """The configuration the oracle evaluates: the plain one, or the four-layer dense equivalent of the conv chain."""
    return cfg if not c else cfg.with_(layer_sizes=conv_dense_layer_sizes(cfg.Nz, c), activations=CONV_ACTS)


def n_params(cfg, c):
    return conv_n_params(cfg.Nz, c) if c else cfg.n_params


def blocks(cfg, c):
    """[(name, slice)] of a model's vector: the plain network's W1, b1, ... or, behind a filter, w, b, then the three Dense layers (W1 4Nz x M)."""
    if not c:
        return PC.blocks(cfg)
    Nz, H, M = cfg.Nz, 4 * cfg.Nz, cfg.Nz - c + 1
    out, o = [("w", slice(0, c)), ("b", slice(c, c + 1))], c + 1
    for l, (ni, no) in enumerate(((M, H), (H, H), (H, Nz - 1))):
        out.append(("W%d" % (l + 1), slice(o, o + ni * no)))
        o += ni * no
        out.append(("b%d" % (l + 1), slice(o, o + no)))
        o += no
    assert o == conv_n_params(Nz, c)
    return out


def is_weight(name):
    return name[0] in "Ww"


def causal_mask(cfg, c):
    """bool [n_params]: the entries W1[r, q], r < q, of the first Dense weight (4Nz x Nz at 0, or 4Nz x M at c + 1; column-major)."""
    H, M = 4 * cfg.Nz, (cfg.Nz - c + 1) if c else cfg.Nz
    r, q = np.meshgrid(np.arange(H), np.arange(M), indexing="ij")
    mask = np.zeros(n_params(cfg, c), bool)
    mask[(c + 1 if c else 0) + (q * H + r)[r < q]] = True
    assert mask.sum() == M * (M - 1) // 2
    return mask


def block_errors(cfg, c, got, ref, extra=()):
    """{block: ||got - ref|| / ||ref||} per block of `blocks`, plus the index sets of `extra` = [(name, bool mask)]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    sel = list(blocks(cfg, c)) + list(extra)
    return {nm: float(np.linalg.norm(got[sl] - ref[sl]) / np.linalg.norm(ref[sl])) for nm, sl in sel}


def worst(errs, weights):
    return max(e for nm, e in errs.items() if is_weight(nm) == weights)


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------------------
def _dense(cfg, c, theta, dt):
    th = np.asarray(theta, dt)
    return O.unpack(conv_to_dense(th, cfg.Nz, c) if c else th, oracle_cfg(cfg, c).layer_sizes, 1)[0]


def loss_grad64(s, theta, i, coeff=0.0):
    """float64 loss and gradient (the model's own layout) of sample i at theta, the penalty with coefficient `coeff` included."""
    cfg, c = s.cfg, s.c
    th = np.asarray(theta, np.float64)
    loss, g = O.nn_pretrain_loss_and_grad(oracle_cfg(cfg, c), 2, s.X[i:i + 1].astype(np.float64), s.B[i:i + 1].astype(np.float64), _dense(cfg, c, th, np.float64),
                                          s.Y[i:i + 1].astype(np.float64), 0.0)
    loss, g = float(loss[0]), (conv_grad_from_dense(g[0], cfg.Nz, c) if c else g[0]).copy()
    if coeff:
        mask = causal_mask(cfg, c)
        loss += coeff * float((th[mask] ** 2).sum())
        g[mask] += 2.0 * coeff * th[mask]
    return loss, g


# ---- float32 restatement ------------------------------------------------------------------------------------------------------------------------------
def loss_grad32(s, theta, i, coeff=0.0):
    """The same with every array in float32: PC.f32_loss_grad on the (dense equivalent of the) network, the fold and the penalty in float32."""
    f = np.float32
    cfg, c = s.cfg, s.c
    th = np.asarray(theta, f)
    ns = SimpleNamespace(cfg=oracle_cfg(cfg, c), k=2, gs=0.0, X=s.X, B=s.B, Y=s.Y)
    loss, g = PC.f32_loss_grad(ns, conv_to_dense(th, cfg.Nz, c) if c else th, i)
    loss, g = f(loss), (conv_grad_from_dense(g, cfg.Nz, c) if c else g).astype(f)
    assert g.dtype == f
    if coeff:
        mask = causal_mask(cfg, c)
        loss = f(loss + f(coeff) * (th[mask] * th[mask]).sum(dtype=f))
        g[mask] += f(2.0) * f(coeff) * th[mask]
    return float(loss), g


def descent32(theta, g, eta):
    out = np.asarray(theta, np.float32) - np.float32(eta) * np.asarray(g, np.float32)
    assert out.dtype == np.float32
    return out


def run_pass(s, theta, order, kind, eta, coeff=0.0, state=None, beta=(0.9, 0.999), eps=1e-8, f32=False):
    """One `Flux.train!` pass from `theta` over `order`: (theta, (m, v, beta_t), [each sample's loss just before its own update]).  kind "adam" carries
    `state` = (m, v, beta_t) (None: a fresh ADAM's), "descent" passes it through untouched.  The library receives eta, beta and eps as floats."""
    dt = np.float32 if f32 else np.float64
    th = np.asarray(theta, dt).copy()
    b = (float(np.float32(beta[0])), float(np.float32(beta[1])))
    m, v, bt = state if state is not None else (np.zeros_like(th), np.zeros_like(th), (float(beta[0]), float(beta[1])))
    eta32 = float(np.float32(eta))
    losses = []
    for i in order:
        loss, g = (loss_grad32 if f32 else loss_grad64)(s, th, int(i), coeff)
        losses.append(loss)
        if kind == "adam":
            if f32:
                th, m, v, bt = PC.f32_adam_step(th, g, m, v, eta, b, eps, bt)
            else:
                th, m, v, bt = O.adam_step(th, g, m, v, eta32, b, float(np.float32(eps)), bt)
        else:
            th = descent32(th, g, eta) if f32 else th - eta32 * g
    return th, (m, v, bt), losses


# ---- samples and weights ------------------------------------------------------------------------------------------------------------------------------
def _min_kink(cfg, c, theta, X, B):
    return PC.min_kink_distance(oracle_cfg(cfg, c), 2, X.astype(np.float64), B.astype(np.float64), _dense(cfg, c, theta, np.float64))


@functools.lru_cache(maxsize=None)
def samples(Nz, c=0, n=1, K=3):
    """cfg, c, n samples X [n, Nz], B [n, 2], Y [n, Nz + 1] (float32; `tests.pretrain_cases.data` on `synthetic.free_convection_problem`, the wT flux) and
    K weight vectors W [K, n_params]: different in every model, non-zero biases, no relu pre-activation — the filter's included — within
    PC.KINK_MARGIN of a kink on any sample.  Shared among the tests: read-only."""
    p = synthetic.free_convection_problem(1, Nz=Nz, n_save=max(2, n), substeps=2, weight_divisor=1.0, t_end=0.005 * (max(2, n) - 1))
    cfg = p.cfg
    X, B, Y = PC.data(p, n)
    X, B, Y = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, B, Y[2]))
    base = synthetic.free_convection_conv_problem(1, c, Nz=Nz, n_save=2, substeps=2, weight_divisor=1.0).weights if c else p.weights
    W, seed = [], 0
    while len(W) < K:
        assert seed < 60, "no seed keeps the pre-activations away from the kinks"
        rng = np.random.default_rng(300 + seed)
        seed += 1
        # (the filter and the dense layers each on their own scale: the taps are O(1), the Glorot weights O(0.1))
        th = np.concatenate([synthetic.perturb_weights(rng, base[:c + 1], 0.25), synthetic.perturb_weights(rng, base[c + 1:], 0.25)]) if c else \
            synthetic.perturb_weights(rng, base, 0.25)
        if _min_kink(cfg, c, th, X, B) > PC.KINK_MARGIN:
            W.append(th)
    W = np.stack(W)
    for a in (X, B, Y, W):
        a.setflags(write=False)
    return SimpleNamespace(cfg=cfg, c=c, X=X, B=B, Y=Y, W=W, K=K, n=n)


# ---- the cases of the GPU tests: name -> (Nz, c, coefficients of the three models) ---------------------------------------------------------------------
GRAD_CASES = {"conv%d_Nz%d" % (c, Nz): (Nz, c, (0.0, 0.0, 0.0)) for c in (2, 3, 8) for Nz in (32, 64)}
GRAD_CASES["plain_penalty_Nz32"] = (32, 0, (0.0, 1.0, 0.3))
GRAD_CASES["plain_penalty_Nz64"] = (64, 0, (0.0, 1.0, 0.3))


def grad_extra(cfg, c, coeff):
    """Under a penalty the masked entries of W1 and the unmasked ones are judged separately."""
    if not coeff:
        return ()
    mask = causal_mask(cfg, c)
    w1 = np.zeros_like(mask)
    w1[dict(blocks(cfg, c))["W1"]] = True
    return (("W1[masked]", mask), ("W1[unmasked]", w1 & ~mask))


@functools.lru_cache(maxsize=None)
def grad_reference(case):
    """(samples, [(loss, gradient) in float64 of model k on the one sample])"""
    Nz, c, coeff = GRAD_CASES[case]
    s = samples(Nz, c, 1, 3)
    ref = [loss_grad64(s, s.W[k], 0, coeff[k]) for k in range(3)]
    for _, g in ref:
        g.setflags(write=False)
    return s, ref


# sequence: conv c = 3 with penalty, one ADAM pass then one Descent pass over per-model orders that differ
SEQ_NZ, SEQ_C = 32, 3
SEQ_COEFF = (1.0, 0.0, 0.3)
SEQ_ORDERS = np.array([SEQ_ORDER, SEQ_ORDER[::-1], (0, 5, 5, 2, 7, 4, 1, 6)], np.int32)


def sequence(f32=False):
    """Per model: ((theta, m, v, beta_t, losses) after the ADAM pass, (theta, losses) after the Descent pass that follows it)."""
    s = samples(SEQ_NZ, SEQ_C, SEQ_N, 3)
    out = []
    for k in range(3):
        th1, (m, v, bt), l1 = run_pass(s, s.W[k], SEQ_ORDERS[k], "adam", ETA_ADAM, SEQ_COEFF[k], f32=f32)
        th2, _, l2 = run_pass(s, th1, SEQ_ORDERS[k], "descent", ETA_DESCENT, SEQ_COEFF[k], f32=f32)
        out.append(((th1, m, v, bt, l1), (th2, l2)))
    return s, out


@functools.lru_cache(maxsize=None)
def sequence_reference():
    return sequence(False)


# driver: K = 2, 2 + 2 epochs, 8 samples, the driver's own permutations
DRV_NZ, DRV_C, DRV_K, DRV_EPOCHS, DRV_SEEDS = 32, 0, 2, 2, (11, 12)
DRV_COEFF = (0.0, 1.0)
DRV_OPTIMIZERS = (("adam", ETA_ADAM), ("descent", ETA_DESCENT))


def driver(f32=False):
    """The loop of `free_convection.train_neural_network_ensemble` per model: (samples, theta [K, P], history [passes, K])."""
    s = samples(DRV_NZ, DRV_C, SEQ_N, DRV_K)
    orders = pretrain_orders(DRV_SEEDS, SEQ_N, len(DRV_OPTIMIZERS) * DRV_EPOCHS)
    theta, hist = [], np.zeros((orders.shape[0], DRV_K))
    for k in range(DRV_K):
        th, p = s.W[k], 0
        for kind, eta in DRV_OPTIMIZERS:
            state = None
            for _ in range(DRV_EPOCHS):
                th, state, _ = run_pass(s, th, orders[p, k], kind, eta, DRV_COEFF[k], state=state if kind == "adam" else None, f32=f32)
                hist[p, k] = np.mean([(loss_grad32 if f32 else loss_grad64)(s, th, i, DRV_COEFF[k])[0] for i in range(SEQ_N)])
                p += 1
        theta.append(th)
    return s, np.stack(theta), hist


@functools.lru_cache(maxsize=None)
def driver_reference():
    return driver(False)


# ---- the error measures of the GPU tests, applied there to the kernel's results and in tests/test_fc_pretrain_host.py to the float32 restatement ------
def grad_errors(s, coeff, loss, g, ref):
    """(loss rel err, worst weight block, worst bias block) of one model's single-sample loss and gradient against ref = (loss, gradient) in float64;
    under a penalty the masked and unmasked entries of W1 count as weight blocks of their own."""
    errs = block_errors(s.cfg, s.c, g, ref[1], grad_extra(s.cfg, s.c, coeff))
    return abs(loss - ref[0]) / ref[0], worst(errs, True), worst(errs, False), errs


def pass_errors(s, theta0, theta, ref_theta, loss, ref_losses, m=None, ref_m=None, v=None, ref_v=None):
    """dict of a pass's errors, largest over the blocks: theta relative to |theta| and to the distance the pass moved the block, m, v, and the mean of
    the pre-update losses; `moved_least` = the least distance moved relative to |theta| over the blocks."""
    cfg, c = s.cfg, s.c
    moved = np.asarray(ref_theta, np.float64) - np.asarray(theta0, np.float64)
    d = np.asarray(theta, np.float64) - ref_theta
    bl = blocks(cfg, c)
    out = dict(theta=max(block_errors(cfg, c, theta, ref_theta).values()),
               moved=max(float(np.linalg.norm(d[sl]) / np.linalg.norm(moved[sl])) for _, sl in bl),
               moved_least=min(float(np.linalg.norm(moved[sl]) / np.linalg.norm(ref_theta[sl])) for _, sl in bl),
               loss=abs(loss - np.mean(ref_losses)) / np.mean(ref_losses))
    if m is not None:
        out["m"] = max(block_errors(cfg, c, m, ref_m).values())
        out["v"] = max(block_errors(cfg, c, v, ref_v).values())
    return out


# Descent: one sample, eta = 1e-2; (theta_0 - theta) / eta is the gradient the update used
DESCENT_CASES = {"plain_Nz32": (32, 0, (0.0, 1.0, 0.3)), "plain_Nz64": (64, 0, (0.0, 1.0, 0.3)), "conv3_Nz32": (32, 3, (0.3, 0.0, 1.0))}


@functools.lru_cache(maxsize=None)
def descent_reference(case):
    Nz, c, coeff = DESCENT_CASES[case]
    s = samples(Nz, c, 1, 3)
    ref = [loss_grad64(s, s.W[k], 0, coeff[k]) for k in range(3)]
    for _, g in ref:
        g.setflags(write=False)
    return s, ref


def descent_gradient(theta0, theta, eta):
    return (np.asarray(theta0, np.float64) - np.asarray(theta, np.float64)) / float(np.float32(eta))
