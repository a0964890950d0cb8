"""Shared by tests/test_pretrain.py (CPU) and tests/test_gpu_pretrain.py (GPU): the samples of flux-MLP pre-training (`train_NN`,
wind_mixing/src/NN_training.jl:207-249), the shapes the one-workgroup kernel is held to the float64 oracle at, and a float32 restatement of the
same loss, gradient and Flux-ADAM chain — what float32 alone costs for this arithmetic, from which the GPU tolerances are derived.
No GPU and no torch needed here."""
import functools
from types import SimpleNamespace

import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O
from tests.test_oracle import VARIANTS


def fluxes(p, X, B, seed=3):
    """the 'true' fluxes of the three nets for profiles X: those of a perturbed weight set, plus noise."""
    cfg = p.cfg
    nets = O.unpack(p.weights_truth.astype(np.float64), cfg.layer_sizes, cfg.n_nets)
    rng = np.random.default_rng(seed)
    return [O.predict_single_flux(cfg, k, X, B, nets[min(k, cfg.n_nets - 1)]) + 0.05 * rng.standard_normal((X.shape[0], cfg.Nz + 1)) for k in range(3)]


def data(p, n, seed=3):
    """(profile, BCs, flux) samples as 𝒟train holds them: states along a trajectory and 'true' fluxes from a perturbed weight set."""
    cfg = p.cfg
    sol = O.solve(cfg, p.x0, p.bcs, p.weights_truth)
    X = sol.reshape(-1, cfg.n_state)[:n]
    B = np.repeat(p.bcs, cfg.n_save, axis=0)[:n].astype(np.float64)
    return X, B, fluxes(p, X, B, seed)


UNSTABLE_FACES = (6, 7, 8, 9, 15, 22, 23, 24, 29)      # interior faces given dT/dz < 0 (of 1..31): runs, a single face, both sides of stable stretches
GT_MARGIN = 0.1                                         # least |dT/dz| (scaled units) on any interior face of such a profile


def destabilise(X, Nz):
    """The synthetic trajectories are stably stratified throughout (dT/dz > 0 on every face), so the convective-adjustment flux
    -cs kappa min(0, dT/dz) would be zero everywhere.  Give T a negative step across UNSTABLE_FACES (dT/dz = -0.32 ... -0.64, well away from the
    switch at 0) and keep its own, positive, steps elsewhere."""
    X = np.array(X, np.float64)
    T = X[:, 2 * Nz:]
    inc = np.diff(T, axis=1)                            # inc[:, f - 1] = T[f] - T[f - 1], the step across face f
    for j, f in enumerate(UNSTABLE_FACES):
        inc[:, f - 1] = -(0.01 + 0.01 * (j % 3) / 2) * 32.0 / Nz
    X[:, 2 * Nz:] = np.concatenate([T[:, :1], T[:, :1] + np.cumsum(inc, axis=1)], axis=1)
    return X


# ---- the single-sample cases: name -> (kind, problem keywords, flux_type, gradient_scaling) -----------------------------------------------
def _wm(k, gs=1e-2, **kw):
    return ("wm", kw, k, gs)


def _fc(gs=1e-2, **kw):
    return ("fc", kw, 2, gs)


CASES = {}
# the conditions of predict_uw / predict_vw / predict_wT at the default shape (Nz = 32, 96-50-20-31 mish)
for _c in ("mpp_zero_weights", "mpp_bc_faces", "raw", "conv_adj_branch"):
    for _k, _nm in enumerate(("uw", "vw", "wT")):
        CASES["%s-%s" % (_c, _nm)] = _wm(_k, **VARIANTS[_c])
# (conv_adj_branch-*: profiles with unstable faces, see destabilise: the closure -cs kappa min(0, dT/dz) is on at nine faces, in the wT flux only)
# T-only models (32-128-128-31 relu), without and with the gradient term
for _gs, _nm in ((0.0, "gs0"), (1e-2, "gs1e-2")):
    CASES["fc-%s" % _nm] = _fc(_gs)
    # (ConvectiveAdjustmentNDE: only the model-kind dispatch.  The flux of a T-only model is [bottom; NN(T); top] for both kinds — predict_single_flux and
    #  the kernel have no adjustment term there — so this is the arithmetic of fc-* again, not coverage of an adjustment flux.)
    CASES["fc_convadj-%s" % _nm] = _fc(_gs, convective_adjustment=True)
# Nz and the LDS carving ((ns + 3) & ~3, act_total + 4, nf + 3)
CASES["wm_Nz4"] = _wm(0, Nz=4)
CASES["wm_Nz5"] = _wm(1, Nz=5)
CASES["wm_Nz20"] = _wm(2, Nz=20)
CASES["wm_Nz64"] = _wm(0, Nz=64, substeps=8)
CASES["fc_Nz33"] = _fc(Nz=33)                 # ns = 33 is padded to 36; 34 faces
CASES["fc_Nz64"] = _fc(Nz=64)
# depth and width (wind mixing, Nz = 32); between them every activation on a hidden layer, tanh / leakyrelu / swish on the output layer
CASES["L1_identity"] = _wm(0, layer_sizes=(96, 31), activations=("identity",))
CASES["L1_tanh"] = _wm(2, layer_sizes=(96, 31), activations=("tanh",))
CASES["96-7-31_swish_leakyrelu"] = _wm(1, layer_sizes=(96, 7, 31), activations=("swish", "leakyrelu"))
CASES["96-600-31_relu"] = _wm(2, layer_sizes=(96, 600, 31), activations=("relu", "identity"))
CASES["96-50-20-13-31_mixed"] = _wm(0, layer_sizes=(96, 50, 20, 13, 31), activations=("mish", "tanh", "swish", "identity"))
CASES["96-400-400-31_swish"] = _wm(1, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
CASES["L8"] = _wm(2, layer_sizes=(96, 24, 21, 18, 16, 14, 12, 10, 31),
                  activations=("identity", "leakyrelu", "tanh", "mish", "relu", "swish", "tanh", "swish"))
# the largest dynamic LDS in the suite: 64 + 3 (7 * 800 + 64 + 4) + 3 * 68 + 64 floats = 69,344 B, above the 64 KB a kernel gets without asking
CASES["fc_Nz64_7x800_lds68k"] = _fc(Nz=64, layer_sizes=(64,) + (800,) * 7 + (63,), activations=("mish",) * 7 + ("identity",))

SEQ_CASE = "mpp_zero_weights-vw"          # the default shape, for the sequence tests
KINK_MARGIN = 1e-4


def problem(case, n_frames=2):
    kind, kw, k, gs = CASES[case]
    kw = dict(kw)
    if kind == "wm":
        p = synthetic.wind_mixing_problem(1, n_frames=n_frames, weight_divisor=1.0, **kw)
    else:
        Nz, ca = kw.get("Nz", 32), kw.get("convective_adjustment", False)
        # a short stable stretch (the convective-adjustment diffusion needs ~20 RK4 sub-steps per 0.0025 at Nz = 32)
        p = synthetic.free_convection_problem(1, n_save=n_frames, substeps=(40 * (Nz // 32) ** 2 if ca else 2), weight_divisor=1.0,
                                              t_end=0.005 * (n_frames - 1), **kw)
    return p, k, gs


def blocks(cfg):
    """[(name, slice)] of one net's packed parameters: W_1, b_1, W_2, b_2, ..."""
    out, o = [], 0
    s = cfg.layer_sizes
    for l in range(cfg.n_layers):
        out.append(("W%d" % (l + 1), slice(o, o + s[l] * s[l + 1])))
        o += s[l] * s[l + 1]
        out.append(("b%d" % (l + 1), slice(o, o + s[l + 1])))
        o += s[l + 1]
    assert o == cfg.net_size
    return out


def block_errors(cfg, got, ref):
    """{block: ||got - ref|| / ||ref||} per layer block (one norm over the net would let W_1 drown the rest)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return {nm: float(np.linalg.norm(got[sl] - ref[sl]) / np.linalg.norm(ref[sl])) for nm, sl in blocks(cfg)}


def worst(errs, kind):
    """largest error over the weight ('W') or bias ('b') blocks."""
    return max(e for nm, e in errs.items() if nm[0] == kind)


def min_kink_distance(cfg, k, x, bcs, layers):
    """least |pre-activation| over the relu / leakyrelu layers (inf: none), in float64."""
    _, tape = O.predict_single_flux(cfg, k, x, bcs, layers, True)
    d = [np.abs(z).min() for (a, z), nm in zip(tape, cfg.activations) if nm in ("relu", "leakyrelu")]
    return float(min(d)) if d else float("inf")


def _net(cfg, k):
    lo = k * cfg.net_size if cfg.n_nets == 3 else 0
    return slice(lo, lo + cfg.net_size)


def _weights(p, k, X, B):
    """float32 weights with non-zero biases, different in the three nets, and no relu / leakyrelu kink within KINK_MARGIN of any sample."""
    cfg = p.cfg
    for seed in range(20):
        theta = synthetic.perturb_weights(np.random.default_rng(100 + seed), p.weights, 0.25)
        layers = O.unpack(theta[_net(cfg, k)].astype(np.float64), cfg.layer_sizes, 1)[0]
        if min_kink_distance(cfg, k, X, B, layers) > KINK_MARGIN:
            return theta, seed
    raise AssertionError("no seed keeps the pre-activations away from the kinks")


@functools.lru_cache(maxsize=None)
def sample(case, n=1):
    """What one case hands the device (float32) and the oracle (the same numbers as float64): cfg, flux_type k, gradient_scaling gs, the
    full weight vector theta, X [n, n_state], B [n, n_bc], Y [n, Nz + 1], and `net` = the slice of theta being trained."""
    p, k, gs = problem(case, n_frames=max(2, n))
    cfg = p.cfg
    X, B, Y = data(p, n)
    if cfg.model == 0 and cfg.convective_adjustment:
        X = destabilise(X, cfg.Nz).astype(np.float32).astype(np.float64)
        Y = fluxes(p, X, B)
    X, B, Y = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, B, Y[k]))
    theta, seed = _weights(p, k, X.astype(np.float64), B.astype(np.float64))
    return SimpleNamespace(case=case, cfg=cfg, k=k, gs=gs, theta=theta, X=X, B=B, Y=Y, net=_net(cfg, k), seed=seed)


def oracle_loss_grad(s, theta_net, i):
    """float64 loss and packed gradient of sample i at the net's weights theta_net."""
    layers = O.unpack(np.asarray(theta_net, np.float64), s.cfg.layer_sizes, 1)[0]
    loss, g = O.nn_pretrain_loss_and_grad(s.cfg, s.k, s.X[i:i + 1].astype(np.float64), s.B[i:i + 1].astype(np.float64), layers,
                                          s.Y[i:i + 1].astype(np.float64), s.gs)
    return float(loss[0]), g[0]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(loss, gradient) of the case's one sample in float64: computed once, shared by the CPU and the GPU test."""
    s = sample(case)
    loss, g = oracle_loss_grad(s, s.theta[s.net], 0)
    g.setflags(write=False)
    return loss, g


# ---- float32 restatement ------------------------------------------------------------------------------------------------------------------
def f32_loss_grad(s, theta_net, i):
    """`NN_loss` and its gradient with every array in float32: predict_single_flux(dtype=float32), the cotangent of
    nn_pretrain_loss_and_grad and mlp_vjp on the float32 tape."""
    f = np.float32
    cfg, Nz, gs = s.cfg, s.cfg.Nz, s.gs
    layers = O.unpack(np.asarray(theta_net, f), cfg.layer_sizes, 1)[0]
    F, tape = O.predict_single_flux(cfg, s.k, s.X[i:i + 1], s.B[i:i + 1], layers, True, dtype=f)
    y = s.Y[i:i + 1]
    r = F - y
    dg = ((F[:, 1:] - F[:, :-1]) - (y[:, 1:] - y[:, :-1])) * f(Nz)
    loss = (r * r).mean(axis=1, dtype=f) + f(gs) * (dg * dg).mean(axis=1, dtype=f)
    Fb = f(2.0 / (Nz + 1)) * r
    Fb[:, 1:] += f(gs * 2.0) * dg
    Fb[:, :-1] -= f(gs * 2.0) * dg
    _, g = O.mlp_vjp(layers, tuple(cfg.activations), tape, Fb[:, 1:Nz])
    g = O.pack_grads([g])
    assert F.dtype == f and loss.dtype == f and g.dtype == f
    return float(loss[0]), g


def f32_adam_step(theta, g, m, v, eta, beta, eps, beta_t):
    """Flux ADAM with float32 state; the running powers travel as doubles (as the library's do)."""
    f = np.float32
    b1, b2 = f(beta[0]), f(beta[1])
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    c1, c2 = f(1.0 / (1.0 - beta_t[0])), f(1.0 / (1.0 - beta_t[1]))
    theta = theta - f(eta) * (m * c1) / (np.sqrt(v * c2) + f(eps))
    assert theta.dtype == f and m.dtype == f and v.dtype == f
    return theta, m, v, (beta_t[0] * float(b1), beta_t[1] * float(b2))


def sequential_pass(s, order, eta=1e-3, beta=(0.9, 0.999), eps=1e-8, f32=False):
    """One `Flux.train!` pass over `order` from zero moments: (theta_net, m, v, beta_t, [each sample's loss just before its update])."""
    dt = np.float32 if f32 else np.float64
    th = s.theta[s.net].astype(dt)
    b = (float(np.float32(beta[0])), float(np.float32(beta[1])))          # the library receives beta, eta and eps as floats
    m, v, bt, losses = np.zeros_like(th), np.zeros_like(th), (float(beta[0]), float(beta[1])), []     # (ADAM.beta_t starts from the doubles)
    for i in order:
        if f32:
            loss, g = f32_loss_grad(s, th, i)
            th, m, v, bt = f32_adam_step(th, g, m, v, eta, b, eps, bt)
        else:
            loss, g = oracle_loss_grad(s, th, i)
            th, m, v, bt = O.adam_step(th, g, m, v, float(np.float32(eta)), b, float(np.float32(eps)), bt)
        losses.append(loss)
    return th, m, v, bt, losses


SEQ_ORDER = (3, 3, 0, 1, 1, 5, 7, 2)          # repeats, and not every sample
SEQ_N = 8


@functools.lru_cache(maxsize=None)
def sequence_reference():
    """The float64 sequential loop over SEQ_ORDER and over 0..n-1 on the default shape: (samples, pass over SEQ_ORDER, pass over 0..n-1)."""
    s = sample(SEQ_CASE, SEQ_N)
    return s, sequential_pass(s, SEQ_ORDER), sequential_pass(s, range(SEQ_N))
