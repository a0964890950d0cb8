"""SURVEY §8f rank 2, second half: `train_NN` flux-MLP pre-training (wind_mixing/src/NN_training.jl:25-169, 207-249;
free_convection/train_free_convection_nde.jl:186-216).  CPU: the oracle's flux closures against the RHS they are pieces of, and its
per-sample gradient against finite differences.  GPU: the one-workgroup pre-training kernel against the oracle's sequential ADAM."""
import functools

import numpy as np
import pytest

import colnde
from colnde import synthetic
from colnde.flux_compat import ADAM
from oracle import nde_oracle as O
from tests import pretrain_cases as PC
from tests.pretrain_cases import data as _data
from tests.test_oracle import VARIANTS


@pytest.mark.parametrize("name", ["mpp_zero_weights", "mpp_bc_faces", "conv_adj_branch", "raw"])
def test_flux_closures_are_the_pieces_of_the_rhs(name):
    """predict_uw/vw/wT (NN_training.jl:25-169) and predict_flux (NDE_training.jl:94-147) restate the same arithmetic: assembling the
    three single-flux face vectors into tendencies (predict_NDE, :160-162) reproduces the oracle's RHS."""
    p = synthetic.wind_mixing_problem(3, n_frames=3, weight_divisor=10.0, **VARIANTS[name])
    cfg = p.cfg
    nets = O.unpack(p.weights.astype(np.float64), cfg.layer_sizes, 3)
    F = [O.predict_single_flux(cfg, k, p.x0, p.bcs, nets[k]) for k in range(3)]
    Nz, sg = cfg.Nz, cfg.sigma
    x = p.x0.astype(np.float64)
    A = [cfg.tau / cfg.H * sg[3 + k] / sg[k] * Nz for k in range(3)]
    du = -A[0] * (F[0][:, 1:] - F[0][:, :-1]) + cfg.f * cfg.tau / sg[0] * (sg[1] * x[:, Nz:2 * Nz] + cfg.mu[1])
    dv = -A[1] * (F[1][:, 1:] - F[1][:, :-1]) - cfg.f * cfg.tau / sg[1] * (sg[0] * x[:, :Nz] + cfg.mu[0])
    dT = -A[2] * (F[2][:, 1:] - F[2][:, :-1])
    np.testing.assert_allclose(np.concatenate([du, dv, dT], axis=1), O.rhs(cfg, p.x0, p.bcs, p.weights), rtol=1e-10, atol=1e-9)


def test_pretrain_gradient_matches_finite_differences():
    p = synthetic.wind_mixing_problem(2, n_frames=3, weight_divisor=10.0)
    cfg = p.cfg
    X, B, Y = _data(p, 4)
    th = p.weights[:cfg.net_size].astype(np.float64)
    loss, g = O.nn_pretrain_loss_and_grad(cfg, 2, X[:1], B[:1], O.unpack(th, cfg.layer_sizes, 1)[0], Y[2][:1], 1e-2)
    rng = np.random.default_rng(0)
    for _ in range(3):
        d = rng.standard_normal(th.shape)
        d /= np.linalg.norm(d)
        h = 1e-6
        f = lambda w: O.nn_pretrain_loss_and_grad(cfg, 2, X[:1], B[:1], O.unpack(w, cfg.layer_sizes, 1)[0], Y[2][:1], 1e-2)[0][0]
        assert np.isclose((f(th + h * d) - f(th - h * d)) / (2 * h), g[0] @ d, rtol=1e-5, atol=1e-12)


# ---- what float32 alone costs for the pre-training arithmetic: the yardstick of tests/test_gpu_pretrain.py, measured without the kernel ----------
# (the constants live in the GPU module, beside the kernel's own figures; it imports neither torch nor the library at module level)
@functools.lru_cache(maxsize=None)
def _f32_single_sample_errors(case):
    s = PC.sample(case)
    loss_ref, g_ref = PC.reference(case)
    loss, g = PC.f32_loss_grad(s, s.theta[s.net], 0)
    errs = PC.block_errors(s.cfg, g, g_ref)
    return abs(loss - loss_ref) / loss_ref, PC.worst(errs, "W"), PC.worst(errs, "b")


@pytest.mark.parametrize("case", list(PC.CASES))
def test_float32_restatement_of_the_single_sample_cases(case):
    """Loss and per-block gradient of every single-sample case in float32 numpy against the float64 oracle.  The GPU module's TOL_LOSS / TOL_W /
    TOL_B are 10x the largest figure printed here (run with -s), rounded up to two digits; this test and the next hold them to that."""
    from tests import test_gpu_pretrain as G
    s = PC.sample(case)
    loss_ref, g_ref = PC.reference(case)
    cfg = s.cfg
    assert all(np.linalg.norm(g_ref[sl]) > 1e-3 for _, sl in PC.blocks(cfg)) and loss_ref > 1e-3            # a non-trivial case
    layers = O.unpack(s.theta[s.net].astype(np.float64), cfg.layer_sizes, 1)[0]
    assert PC.min_kink_distance(cfg, s.k, s.X.astype(np.float64), s.B.astype(np.float64), layers) > PC.KINK_MARGIN
    e_loss, e_W, e_b = _f32_single_sample_errors(case)
    print("%s: float32 loss rel err %.2e, weight blocks %.2e, bias blocks %.2e" % (case, e_loss, e_W, e_b))
    assert 10 * e_loss <= G.TOL_LOSS and 10 * e_W <= G.TOL_W and 10 * e_b <= G.TOL_B


def test_single_sample_tolerances_are_not_looser_than_the_rule():
    """... and none of the three is more than 12x the largest measurement (a bound must not go stale on the loose side)."""
    from tests import test_gpu_pretrain as G
    worst = [max(e) for e in zip(*(_f32_single_sample_errors(c) for c in PC.CASES))]
    print("largest float32 errors over the cases: loss %.3e, weight blocks %.3e, bias blocks %.3e" % tuple(worst))
    assert G.TOL_LOSS <= 12 * worst[0] and G.TOL_W <= 12 * worst[1] and G.TOL_B <= 12 * worst[2]


@pytest.mark.parametrize("nm,k", [("uw", 0), ("vw", 1), ("wT", 2)])
def test_convective_adjustment_cases_have_the_closure_switched_on(nm, k):
    """The conv_adj_branch-* samples mix faces with dT/dz < 0 and > 0, every one a margin away from the switch (in the float32 the device gets), and the
    adjustment flux -cs kappa min(0, dT/dz) is then part of the wT flux and of nothing else (NN_training.jl:141-143)."""
    s = PC.sample("conv_adj_branch-%s" % nm)
    cfg, Nz = s.cfg, s.cfg.Nz
    assert cfg.convective_adjustment and not cfg.modified_pacanowski_philander and s.k == k
    gT = np.diff(s.X[0, 2 * Nz:]) * np.float32(Nz)                         # interior faces 1..Nz-1, float32
    assert sorted(np.nonzero(gT < 0)[0] + 1) == sorted(PC.UNSTABLE_FACES) and (gT > 0).sum() == Nz - 1 - len(PC.UNSTABLE_FACES)
    assert np.abs(gT).min() > PC.GT_MARGIN
    layers = O.unpack(s.theta[s.net].astype(np.float64), cfg.layer_sizes, 1)[0]
    X, B = s.X.astype(np.float64), s.B.astype(np.float64)
    F_ca = O.predict_single_flux(cfg, k, X, B, layers)
    F_raw = O.predict_single_flux(cfg.with_(convective_adjustment=False), k, X, B, layers)
    d = (F_ca - F_raw)[0]
    if k == 2:
        on = np.zeros(Nz + 1, bool)
        on[list(PC.UNSTABLE_FACES)] = True
        assert (d[on] > 0.1).all() and not d[~on].any()                     # an upward flux of order cs kappa |dT/dz| = 3.7 ... 7.5 on the unstable faces only
        loss_raw = O.nn_pretrain_loss_and_grad(cfg.with_(convective_adjustment=False), k, X, B, layers, s.Y.astype(np.float64), s.gs)[0][0]
        assert abs(loss_raw - PC.reference(s.case)[0]) > 0.1 * PC.reference(s.case)[0]          # a kernel without the branch misses the loss by far
    else:
        assert not d.any()


def test_float32_restatement_of_the_sequential_passes():
    """The passes of the GPU module's sequence tests (repeated order, 0..n-1, one sample) with float32 weights and moments against the float64
    loop: TOL_M / TOL_V / TOL_THETA / TOL_MOVED are 10x the largest block error printed here, rounded up to two digits, and none is more
    than 12x it."""
    from tests import test_gpu_pretrain as G
    s, ref_rep, ref_id = PC.sequence_reference()
    one = PC.sample(PC.SEQ_CASE)
    worst = dict(loss=0.0, m=0.0, v=0.0, theta=0.0, moved=0.0)
    for smp, order, ref in ((s, PC.SEQ_ORDER, ref_rep), (s, range(PC.SEQ_N), ref_id), (one, [0], PC.sequential_pass(one, [0]))):
        th, m, v, bt, losses = PC.sequential_pass(smp, order, f32=True)
        assert bt == ref[3]
        moved = ref[0] - smp.theta[smp.net]
        e = dict(loss=abs(np.mean(losses) - np.mean(ref[4])) / np.mean(ref[4]), m=max(PC.block_errors(s.cfg, m, ref[1]).values()),
                 v=max(PC.block_errors(s.cfg, v, ref[2]).values()), theta=max(PC.block_errors(s.cfg, th, ref[0]).values()),
                 moved=max(float(np.linalg.norm((th - ref[0])[sl]) / np.linalg.norm(moved[sl])) for _, sl in PC.blocks(s.cfg)))
        print("order %s: float32 " % (list(order),) + ", ".join("%s %.2e" % kv for kv in e.items()))
        worst = {q: max(worst[q], e[q]) for q in worst}
    assert 10 * worst["loss"] <= G.TOL_LOSS and 10 * worst["m"] <= G.TOL_M and 10 * worst["v"] <= G.TOL_V
    assert 10 * worst["theta"] <= G.TOL_THETA and 10 * worst["moved"] <= G.TOL_MOVED
    tol = dict(m=G.TOL_M, v=G.TOL_V, theta=G.TOL_THETA, moved=G.TOL_MOVED)
    assert all(tol[q] <= 12 * worst[q] for q in tol), (tol, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["uw_mpp", "vw_mpp_bc", "wT_mpp", "wT_ca", "fc"])
def test_device_pretraining_follows_the_sequential_adam_of_flux_train(case):
    from colnde.wind_mixing import train_NN
    if case == "fc":
        p = synthetic.free_convection_problem(3, Nz=32, n_save=9, substeps=2, t_end=0.05)
        k, gs = 2, 0.0
    else:
        kw = {"uw_mpp": {}, "vw_mpp_bc": VARIANTS["mpp_bc_faces"], "wT_mpp": {}, "wT_ca": VARIANTS["conv_adj_branch"]}[case]
        p = synthetic.wind_mixing_problem(3, n_frames=9, weight_divisor=10.0, **kw)
        k, gs = {"uw": 0, "vw": 1, "wT": 2}[case[:2]], 1e-2
    cfg = p.cfg
    n = 24
    X, B, Y = _data(p, n)
    order = np.random.default_rng(1).permutation(n)
    ns = cfg.net_size
    lo = k * ns if cfg.n_nets == 3 else 0
    ref, hist_ref = O.train_NN(cfg, k, p.weights[lo:lo + ns], X, B, Y[k], order, 1e-3, 2, gs)
    with colnde.ColumnNDE(cfg, 1) as eng:
        w, hist = train_NN(eng, ["uw", "vw", "wT"][k], p.weights, X, B, Y[k], [ADAM(1e-3)], [2], gradient_scaling=gs, order=order)
    assert hist_ref[1] < hist_ref[0]
    np.testing.assert_allclose(hist, hist_ref, rtol=2e-4)
    rel = np.linalg.norm(w[lo:lo + ns] - ref) / np.linalg.norm(ref)
    moved = np.linalg.norm(ref - p.weights[lo:lo + ns]) / np.linalg.norm(ref)
    assert rel < 2e-4 * max(1.0, moved / 1e-2) and moved > 1e-3          # 48 ADAM steps of float32 against float64
    other = np.ones(cfg.n_params, bool)
    other[lo:lo + ns] = False
    np.testing.assert_array_equal(w[other], p.weights[other])            # the other nets are untouched
