"""The inputs and bounds of tests/test_gpu_distinct_nets.py as checked facts, on the CPU (tests/distinct_nets.py holds the cases).

For every reference case the GPU file uses: the activations bend (wind mixing: a hidden pre-activation of 3 or more, above 1.5 in every net, both
signs in every hidden layer; free convection: both relu branches of every hidden layer), every layer block carries a measurable share of the
gradient, and a float32 restatement of the same arithmetic is within a TENTH of every bound the GPU file asserts — oracle.cref (the C port) where
it has the stepper; the float32 NumPy oracle for RKC2, the step schedule and the conv network's Toeplitz form, which the C port does not have.

And the checks see what they are for, on the float64 oracle's own arrays: exchanging two nets' parameters or zeroing the biases moves the solution
by more than 100 x its bound; a 1 % error in the smallest block passes the whole-vector norm and fails the per-block one; on the suite's usual
weights the nets are identical, the biases zero and the pre-activations below 0.1."""
import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as O
from tests import distinct_nets as D

WM = sorted(D.WM_CASES)
FC = sorted(D.FC_CASES)
ALL = WM + FC


def _case(name):
    return (D.WM_CASES[name] if name in D.WM_CASES else D.FC_CASES[name])()


def _bounds(name):
    """(solution, total rtol, gradient) of the GPU file for this case"""
    from tests.test_gpu_parity import FC_GRAD_REL, FC_LOSS_RTOL, FC_SOL_ATOL, GRAD_REL, LOSS_RTOL, SOL_ATOL
    return (SOL_ATOL, LOSS_RTOL, GRAD_REL) if name in D.WM_CASES else (FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL)


def _network(c):
    """(cfg, weights) the oracle evaluates: the conv case's is the equivalent Toeplitz network"""
    if hasattr(c, "conv"):
        from colnde.free_convection import conv_to_dense
        return c.dense_cfg, conv_to_dense(c.w.astype(np.float64), c.cfg.Nz, c.conv)
    return c.cfg, c.w


def _float32(name, c):
    """(total, terms, gradient, solution, which) of the float32 restatement"""
    if hasattr(c, "conv"):
        from tests import conv_cases as CC
        tot, g, sol = CC.oracle_loss_grad(c.cfg, c.conv, c.p.x0, c.p.bcs, c.w, c.truth, dtype=np.float32)
        return float(tot), np.array([0, 0, tot, 0, 0, 0.0]), g, sol, "numpy float32"
    if getattr(c.cfg, "stepper", "rk4") != "rk4" or hasattr(c, "schedule"):
        run = lambda: O.loss_and_grad(c.cfg, c.p.x0, c.p.bcs, c.w, c.truth, c.sc, dtype=np.float32)
        tot, terms, g, sol = D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run()
        return float(tot), terms, g, sol, "numpy float32"
    from oracle import cref
    tot, terms, g, sol = cref.loss_grad(c.cfg, c.p.x0, c.p.bcs, c.w, c.truth, c.sc, want_sol=True)
    return tot, terms, g, sol, "C port"


def _float32_errors(name, c):
    from tests.test_gpu_parity import _rel
    tot, terms, g, sol, which = _float32(name, c)
    blk, e = D.worst_block(g, c.g, c.blocks)
    return dict(sol_abs=float(np.abs(sol - c.sol).max()), loss_rel=abs(tot - c.tot) / abs(c.tot), grad_rel=float(_rel(g, c.g)), block_rel=e, block=blk,
                terms_abs=[float(v) for v in np.abs(np.asarray(terms, np.float64) - c.terms)], which=which)


def _terms_slack(c):
    """the GPU file's bound on each wind-mixing term: rtol = LOSS_RTOL, atol = 1e-3 LOSS_RTOL sum(terms)"""
    from tests.test_gpu_parity import LOSS_RTOL
    return LOSS_RTOL * np.abs(c.terms) + 1e-3 * LOSS_RTOL * float(np.sum(c.terms))


# ------------------------------------------------------------------------------------------------------------------ the helper itself
def test_blocks_come_from_the_oracles_packing_and_cover_the_vector():
    cfg = synthetic.wind_mixing_problem(1, n_frames=2).cfg
    bl = D.blocks(cfg)
    assert len(bl) == 18 and [b[:3] for b in bl[:3]] == [(0, 0, "W"), (0, 0, "b"), (0, 1, "W")]
    assert bl[0][3] == slice(0, 96 * 50) and bl[-1][3].stop == cfg.n_params
    assert all(a[3].stop == b[3].start for a, b in zip(bl, bl[1:]))
    assert [n for n, _ in D.named_blocks(cfg)][:2] == ["uw/W1", "uw/b1"] and D.named_blocks(cfg)[-1][0] == "wT/b3"
    fc = synthetic.free_convection_problem(1, n_save=2).cfg
    assert [n for n, _ in D.named_blocks(fc)] == ["W1", "b1", "W2", "b2", "W3", "b3"] and D.blocks(fc)[-1][3].stop == fc.n_params
    # the layout is unpack's: a gradient packed by pack_grads lands where blocks says
    nets = O.unpack(np.arange(cfg.n_params, dtype=np.float64), cfg.layer_sizes, 3)
    for k, l, kind, s in bl:
        a = nets[k][l][0 if kind == "W" else 1]
        assert np.array_equal(np.sort(a.reshape(-1)), np.arange(s.start, s.stop))


def test_weights_are_distinct_biased_and_reproducible():
    cfg = synthetic.wind_mixing_problem(1, n_frames=2).cfg
    w = D.weights(cfg, 3)
    assert w.dtype == np.float32 and np.array_equal(w, D.weights(cfg, 3)) and not np.array_equal(w, D.weights(cfg, 4))
    D.assert_distinct_and_biased(cfg, w)
    for k, l, kind, s in D.blocks(cfg):
        if kind == "b":
            assert np.abs(w[s]).max() <= 1 and np.abs(D.weights(cfg, 3, 10.0, 0.3)[s]).max() <= np.float32(0.3)
        else:
            assert np.allclose(D.weights(cfg, 3, 10.0)[s], w[s] / 10, rtol=1e-6, atol=0)
    usual = synthetic.wind_mixing_problem(1, n_frames=2, weight_divisor=1e2).weights
    with pytest.raises(AssertionError):
        D.assert_distinct_and_biased(cfg, usual)


def test_block_errors_names_the_block():
    cfg = synthetic.wind_mixing_problem(1, n_frames=2).cfg
    named = D.named_blocks(cfg)
    ref = np.random.default_rng(0).standard_normal(cfg.n_params)
    got = ref.copy()
    s = dict(named)["vw/b2"]
    got[s] *= 1.5
    errs = D.block_errors(got, ref, named)
    assert [n for n, e, _ in errs if e > 0] == ["vw/b2"] and D.worst_block(got, ref, named)[0] == "vw/b2"
    assert np.isclose(dict((n, e) for n, e, _ in errs)["vw/b2"], 0.5) and np.isclose(sum(sh * sh for _, _, sh in errs), 1.0)


def test_reference_cases_are_shared_and_read_only():
    c = _case("mish/21")
    assert _case("mish/21") is c
    for a in (c.w, c.truth, c.g, c.sol, c.terms, c.p.x0, c.p.bcs):
        assert not a.flags.writeable
    assert c.truth.dtype == np.float32 and c.sol.shape == (21, D.FRAMES, 96) and c.cfg.substeps == D.SUBSTEPS
    assert _case("mish/21/schedule").truth is c.truth and _case("mish/21/schedule").tot != c.tot


# ------------------------------------------------------------------------------------------------------------------ the activations bend
@pytest.mark.parametrize("name", WM)
def test_wind_mixing_preactivations_reach_where_the_activations_bend(name):
    c = _case(name)
    run = lambda: D.stage_inputs(c.cfg, c.p.x0, c.p.bcs, c.w)
    X = D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run()
    Z = D.preactivations(c.cfg, c.w, X)
    per_net = [max(float(np.abs(Z[(k, l)]).max()) for l in range(2)) for k in range(3)]
    above2 = [float((np.abs(Z[(k, 0)]).max(axis=0) > 2).mean()) for k in range(3)]
    print("distinct nets, %s: largest hidden pre-activation per net %s, share of layer-1 units above 2: %s, largest state %.2f" %
          (name, ["%.2f" % v for v in per_net], ["%.2f" % v for v in above2], np.abs(c.sol).max()))
    assert max(per_net) >= 3.0
    assert min(per_net) > 1.5
    for key, z in Z.items():
        assert (z > 0).any() and (z < 0).any(), key
    assert np.abs(c.sol).max() < 10                                     # the solve is stable at O(1) weights


@pytest.mark.parametrize("name", FC)
def test_free_convection_preactivations_take_both_relu_branches(name):
    """relu has no curve to reach: what a case must do is put hidden units on both sides of the kink, in every hidden layer (the conv case: the
    filter's relu included), and keep units changing side over the solve out of the float32 restatement's way (the C-port test below)"""
    c = _case(name)
    cfg, w = _network(c)
    Z = D.preactivations(cfg, w, D.stage_inputs(cfg, c.p.x0, c.p.bcs, w))
    assert len(Z) == len(cfg.layer_sizes) - 2
    for key, z in Z.items():
        frac = float((z > 0).mean())
        assert 0.05 < frac < 0.95, (key, frac)


@pytest.mark.parametrize("name", ALL)
def test_every_block_is_a_measurable_share_of_the_gradient(name):
    c = _case(name)
    shares = D.block_errors(c.g, c.g, c.blocks)
    print("distinct nets, %s: smallest block %s, %.2e of the gradient norm" % ((name,) + min(((n, s) for n, _, s in shares), key=lambda t: t[1])))
    assert min(s for _, _, s in shares) >= 1e-4
    assert len(shares) == (18 if name in D.WM_CASES else 8 if hasattr(c, "conv") else 6)


# ------------------------------------------------------------------------------------------------------------------ the float32 restatement
@pytest.mark.parametrize("name", ALL)
def test_float32_restatement_is_within_a_tenth_of_every_bound(name):
    c = _case(name)
    sol_b, loss_b, grad_b = _bounds(name)
    e = _float32_errors(name, c)
    print("distinct nets, %s (%s): %s" % (name, e["which"], {k: v for k, v in e.items() if k != "which"}))
    from tests.test_gpu_parity import _record                         # (with COLNDE_RECORD_ERRORS set: into the suite's error record)
    _record("distinct_nets_float32/" + name, sol_abs=e["sol_abs"], loss_rel=e["loss_rel"], grad_rel=e["grad_rel"], **{"block_rel:" + e["block"]: e["block_rel"]})
    assert e["which"] == ("numpy float32" if name in ("mish/21/rkc2", "mish/21/schedule", "conv3/32") else "C port")
    assert e["sol_abs"] <= sol_b / 10
    assert e["loss_rel"] <= loss_b / 10
    assert e["grad_rel"] <= grad_b / 10 and e["block_rel"] <= grad_b / 10, e["block"]
    if name in D.WM_CASES:
        assert (np.array(e["terms_abs"]) <= _terms_slack(c) / 10).all(), (e["terms_abs"], c.terms)


def test_free_convection_seeds_are_the_first_the_float32_restatement_passes_on():
    """relu kinks can flip between float32 and float64: a case takes the first of FC_SEEDS on which the restatement is within a tenth of the FC_* bounds"""
    for key, chosen in D.FC_SEED.items():
        name = {(32, False): "fc/32", (64, False): "fc/64", (32, True): "ca/32", "conv": "conv3/32"}[key]
        sol_b, loss_b, grad_b = _bounds(name)
        make = D.conv_case if key == "conv" else (lambda seed, key=key: D.fc_case(key[0], key[1], seed))
        first = None
        for seed in D.FC_SEEDS:
            e = _float32_errors(name, make(seed=seed) if key == "conv" else make(seed))
            if e["sol_abs"] <= sol_b / 10 and e["loss_rel"] <= loss_b / 10 and e["grad_rel"] <= grad_b / 10 and e["block_rel"] <= grad_b / 10:
                first = seed
                break
        assert first is not None, name
        assert chosen == first and _case(name).seed == first, (name, chosen, first)


# ------------------------------------------------------------------------------------------------------------------ the checks see what they are for
@pytest.mark.parametrize("name", WM)
def test_exchanging_two_nets_moves_the_solution(name):
    c = _case(name)
    sol_b = _bounds(name)[0]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        w = D.swap_nets(c.cfg, c.w, a, b)
        run = lambda: O.solve(c.cfg, c.p.x0, c.p.bcs, w)
        sol = D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run()
        assert np.abs(sol - c.sol).max() > 100 * sol_b, (a, b)


@pytest.mark.parametrize("name", ALL)
def test_zeroing_the_biases_moves_the_solution(name):
    c = _case(name)
    sol_b = _bounds(name)[0]
    if hasattr(c, "conv"):
        from colnde.free_convection import conv_to_dense
        w = c.w.astype(np.float64)
        w[c.conv + 1:] = D.zero_biases(c.cfg.with_(layer_sizes=(c.cfg.Nz - c.conv + 1,) + tuple(c.cfg.layer_sizes[1:])), w[c.conv + 1:])
        w[c.conv] = 0                                                   # the filter's bias with them
        cfg, w = c.dense_cfg, conv_to_dense(w, c.cfg.Nz, c.conv)
    else:
        cfg, w = c.cfg, D.zero_biases(c.cfg, c.w)
    run = lambda: O.solve(cfg, c.p.x0, c.p.bcs, w)
    sol = D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run()
    moved = float(np.abs(sol - c.sol).max())
    print("distinct nets, %s: zeroed biases move the solution by %.3e (bound %.1e)" % (name, moved, sol_b))
    assert moved > 100 * sol_b


@pytest.mark.parametrize("name", ALL)
def test_one_percent_in_the_smallest_block_passes_the_norm_and_fails_the_blocks(name):
    """the case the whole-vector norm cannot see"""
    from tests.test_gpu_parity import _rel
    c = _case(name)
    grad_b = _bounds(name)[2]
    smallest, _, share = min(D.block_errors(c.g, c.g, c.blocks), key=lambda t: t[2])
    g = np.array(c.g)
    g[dict(c.blocks)[smallest]] *= 1.01
    assert _rel(g, c.g) < grad_b / 2
    blk, e = D.worst_block(g, c.g, c.blocks)
    assert blk == smallest and e > grad_b and np.isclose(e, 0.01)


def test_the_usual_weights_show_none_of_this():
    """the setting of almost every parity test: the three nets are one draw, every bias is zero, no activation leaves its linear range"""
    p = synthetic.wind_mixing_problem(21, n_frames=9, weight_divisor=1e2)
    where = {(k, l, kind): s for k, l, kind, s in D.blocks(p.cfg)}
    for (k, l, kind), s in where.items():
        assert np.array_equal(p.weights[s], p.weights[where[(0, l, kind)]])
        if kind == "b":
            assert not p.weights[s].any()
    Z = D.preactivations(p.cfg, p.weights, D.stage_inputs(p.cfg, p.x0, p.bcs, p.weights))
    assert max(float(np.abs(z).max()) for z in Z.values()) < 0.1
    assert np.array_equal(O.solve(p.cfg, p.x0, p.bcs, D.swap_nets(p.cfg, p.weights, 0, 2)), O.solve(p.cfg, p.x0, p.bcs, p.weights))
    fc = synthetic.free_convection_problem(19, n_save=5, substeps=2, t_end=0.01)
    assert not any(fc.weights[s].any() for k, l, kind, s in D.blocks(fc.cfg) if kind == "b")
