"""Shared by tests/test_wm_pretrain_host.py (CPU) and tests/test_gpu_wm_pretrain.py (GPU): the K = 3 constant sets, samples, per-chain orders and rates of the
ensemble flux pre-training of a wind-mixing sweep (`colnde_ensemble_pretrain_wm_flux_dev`: `train_NN`, wind_mixing/src/NN_training.jl:207-249, for all K x 3
networks in one launch), and its float64 references and float32 restatements.  Everything is built from tests/pretrain_cases.py: a chain (model k, net j) is
that module's sample with model k's five constants put into a copy of the config, so its oracle, its float32 restatement and its sequential loop apply
unchanged.  One column, the helper's 8-frame config, at most 8 samples, Nz = 32, 96-50-20-31 nets.  No GPU and no torch needed here."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

from colnde import synthetic
from colnde.free_convection import pretrain_orders
from colnde.nde import PHYSICS_KEYS
from oracle import nde_oracle as O
from tests import pretrain_cases as PC

NETS = ("uw", "vw", "wT")
K = 3
# (nu0, nu_minus, dRi, Ric, Pr) per model: every constant differs between the models; model 1 has the steep tanh of VARIANTS["dRi_small"], models 1 and 2 Pr != 1
PHYSICS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.1, 0.2, 1.2], [1e-3, 0.05, 1.3, 0.3, 2.0]], np.float32)
PHYSICS_ALT = np.array([2e-4, 0.09, 0.6, 0.15, 0.8], np.float32)      # what set_physics gives model 1 in the independence test
MPP_CONDS = ("mpp_zero_weights", "mpp_bc_faces")                        # the condition sets that read the constants: the three sets above
PLAIN_CONDS = ("conv_adj_branch", "raw")                                # ... and those that do not: physics = None
GS = 1e-2
N = PC.SEQ_N
# per-chain orders over the 8 samples, with repeats, different in every chain: rotations and reversals of PC.SEQ_ORDER
ORDERS = np.array([[np.roll(PC.SEQ_ORDER[::-1] if (k + j) % 2 else PC.SEQ_ORDER, ((0, 1, 2), (3, 4, 5), (6, 7, 1))[k][j]) for j in range(3)] for k in range(K)], np.int32)
ETAS = np.array([[1e-3, 2e-3, 5e-4], [2e-3, 5e-4, 1e-3], [5e-4, 1e-3, 2e-3]], np.float32)


def model_cfg(cfg, row):
    """cfg with one model's five constants (the floats the library receives)"""
    return dataclasses.replace(cfg, **{key: float(np.float32(x)) for key, x in zip(PHYSICS_KEYS, row)})


def physics_of(cond):
    return PHYSICS if cond in MPP_CONDS else None


@functools.lru_cache(maxsize=None)
def samples(cond, n=1, n_models=K):
    """One condition set's data as the ensemble call takes it (float32, read-only): cfg, X [n, 96], B [n, 6], Y [3, n, 33] (uw, vw, wT) and the weights
    W [n_models, P], different in every model and net (tests.pretrain_cases.sample per net: the same profiles and weights for the three)."""
    per_net = [PC.sample("%s-%s" % (cond, nm), n) for nm in NETS]
    s0 = per_net[0]
    for s in per_net[1:]:
        assert np.array_equal(s.X, s0.X) and np.array_equal(s.B, s0.B) and np.array_equal(s.theta, s0.theta)
    Y = np.stack([s.Y for s in per_net])
    W = np.stack([s0.theta] + [synthetic.perturb_weights(np.random.default_rng(500 + k), s0.theta, 0.1) for k in range(1, n_models)]).astype(np.float32)
    X, B = s0.X.copy(), s0.B.copy()
    for a in (X, B, Y, W):
        a.setflags(write=False)
    return SimpleNamespace(cond=cond, cfg=s0.cfg, X=X, B=B, Y=Y, W=W, n=n, K=n_models)


def chain(s, k, j, physics="own", theta=None):
    """Chain (model k, net j) as a sample of tests.pretrain_cases: the config carries model k's constants (physics: "own" = the condition set's,
    None = the config's, or an explicit [K, 5])."""
    ph = physics_of(s.cond) if isinstance(physics, str) else physics
    cfg = s.cfg if ph is None else model_cfg(s.cfg, ph[k])
    net = slice(j * cfg.net_size, (j + 1) * cfg.net_size)
    return SimpleNamespace(case="%s[%d]-%s" % (s.cond, k, NETS[j]), cfg=cfg, k=j, gs=GS, theta=s.W[k] if theta is None else theta, X=s.X, B=s.B, Y=s.Y[j], net=net)


def chains(s):
    return [(k, j, chain(s, k, j)) for k in range(s.K) for j in range(3)]


# ---- D: single-sample loss and gradient ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_reference(cond):
    """(samples, {(k, j): (loss, gradient)} in float64 on the one sample)"""
    s = samples(cond, 1)
    ref = {(k, j): PC.oracle_loss_grad(c, c.theta[c.net], 0) for k, j, c in chains(s)}
    for _, g in ref.values():
        g.setflags(write=False)
    return s, ref


def grad_errors(c, loss, g, ref):
    """(loss rel err, worst weight block, worst bias block, per-block errors)"""
    errs = PC.block_errors(c.cfg, g, ref[1])
    return abs(loss - ref[0]) / ref[0], PC.worst(errs, "W"), PC.worst(errs, "b"), errs


# ---- E: one ADAM pass over the per-chain orders ---------------------------------------------------------------------------------------------
SEQ_COND = "mpp_zero_weights"


def sequence(f32=False):
    """(samples, {(k, j): (theta_net, m, v, beta_t, pre-update losses)}) of one pass from zero moments at rate ETAS[k, j] over ORDERS[k, j]"""
    s = samples(SEQ_COND, N)
    return s, {(k, j): PC.sequential_pass(c, ORDERS[k, j], eta=float(ETAS[k, j]), f32=f32) for k, j, c in chains(s)}


@functools.lru_cache(maxsize=None)
def sequence_reference():
    return sequence(False)


def pass_errors(c, theta, m, v, loss, ref):
    """dict of a pass's errors on one chain, largest over the layer blocks: theta relative to |theta| and to the distance the pass moved the block, m, v,
    the mean of the pre-update losses; `moved_least` = the least distance moved relative to |theta| over the blocks."""
    th_ref, m_ref, v_ref, _, losses_ref = ref
    cfg = c.cfg
    moved = np.asarray(th_ref, np.float64) - c.theta[c.net]
    d = np.asarray(theta, np.float64) - th_ref
    bl = PC.blocks(cfg)
    return dict(theta=max(PC.block_errors(cfg, theta, th_ref).values()),
                moved=max(float(np.linalg.norm(d[sl]) / np.linalg.norm(moved[sl])) for _, sl in bl),
                moved_least=min(float(np.linalg.norm(moved[sl]) / np.linalg.norm(th_ref[sl])) for _, sl in bl),
                m=max(PC.block_errors(cfg, m, m_ref).values()), v=max(PC.block_errors(cfg, v, v_ref).values()),
                loss=abs(loss - np.mean(losses_ref)) / np.mean(losses_ref))


# ---- F: the driver: K = 2, two optimisers x 2 epochs, 8 samples, the driver's own permutations -----------------------------------------------
DRV_COND, DRV_K, DRV_EPOCHS = "mpp_zero_weights", 2, (2, 2)
DRV_RATES = (1e-3, 3e-4)
DRV_SEEDS = np.array([[11, 12, 13], [14, 15, 16]])
DRV_GS = 1e-4                                                          # train_NN's default gradient_scaling


def driver_orders():
    return pretrain_orders(DRV_SEEDS.reshape(-1), N, sum(DRV_EPOCHS)).reshape(sum(DRV_EPOCHS), DRV_K, 3, N)


def driver(f32=False):
    """The loop of `wind_mixing.train_NN_ensemble` chain by chain: (samples, theta [K, P], history [passes, K, 3]).  Moments and running powers start
    afresh with each optimiser and carry across its epochs; after each pass the mean loss over the training set at the weights it left."""
    s = samples(DRV_COND, N, DRV_K)
    orders = driver_orders()
    dt = np.float32 if f32 else np.float64
    theta, hist = np.array(s.W, dt), np.zeros((sum(DRV_EPOCHS), DRV_K, 3))
    loss_grad = PC.f32_loss_grad if f32 else PC.oracle_loss_grad
    beta = (float(np.float32(0.9)), float(np.float32(0.999)))
    for k in range(DRV_K):
        for j in range(3):
            c = chain(s, k, j, physics=PHYSICS)
            c.gs = DRV_GS
            th, p = theta[k, c.net].copy(), 0
            for eta, n_ep in zip(DRV_RATES, DRV_EPOCHS):
                m, v, bt = np.zeros_like(th), np.zeros_like(th), (0.9, 0.999)
                for _ in range(n_ep):
                    for i in orders[p, k, j]:
                        _, g = loss_grad(c, th, i)
                        if f32:
                            th, m, v, bt = PC.f32_adam_step(th, g, m, v, eta, beta, 1e-8, bt)
                        else:
                            th, m, v, bt = O.adam_step(th, g, m, v, float(np.float32(eta)), beta, float(np.float32(1e-8)), bt)
                    hist[p, k, j] = np.mean([loss_grad(c, th, i)[0] for i in range(N)])
                    p += 1
            theta[k, c.net] = th
    return s, theta, hist


@functools.lru_cache(maxsize=None)
def driver_reference():
    return driver(False)
