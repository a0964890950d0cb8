"""The inputs and bounds of tests/test_gpu_activation_range.py as checked facts, on the CPU (tests/activation_range_cases.py holds the cases).

For every case the GPU file holds to the oracle — 96-50-20-31 at 21 and 70 columns for the five activations, its RKC2 and step-schedule variants, and
the wide shapes 96-400-31 and 96-400-400-31: the ladders put a unit of every net and of every hidden layer into each interval of the activation's
tails AT EVERY STAGE EVALUATION of the float64 solve (`A.REQUIRED`), a third of the units stay inside [-3, 3], and no relu or leakyrelu unit comes
closer to its kink than 1e-4; a float32 restatement (the C port, oracle.cref; the float32 NumPy oracle for RKC2 and the schedule, which the port does
not have) is within a TENTH of every bound the GPU file asserts; and the per-unit figure `A.PER_UNIT` is ten times the restatement's own worst
per-entry error of the hidden bias gradients on the shape that carries that check, 96-50-20-31.

And the inputs can tell a wrong kernel: five wrong activations swapped into the float64 oracle (`O.act` / `O.act_grad`) each miss a bound that the
GPU file asserts by a factor of ten or more (the unclamped float32 mish: it is not finite, which the GPU file asserts first).  The two wrong
derivatives pass the whole-gradient norm (a tenth of its bound) and fail the layer blocks by 500 and the per-unit check by 4e4 and more.

The forward-only families (embedding on the net-split shape and of any architecture, profile, flux pre-training) run the same ladders under
`A.forward_weights`; their float32 restatements are within a tenth of the tolerances of the families' own GPU tests.

How the relative class of the per-unit check is read here: at least a quarter of every hidden bias block is in it, for all five activations; for
tanh, whose 1 - t^2 is below 1e-3 from |z| = 4.2 on, the class is also held to contain nine in ten of the units that stay inside |z| < 3 (the
other factor of dL/db_j differs from unit to unit) and nothing beyond |z| = 9."""
import numpy as np
import pytest

from oracle import nde_oracle as O
from tests import activation_range_cases as A
from tests import distinct_nets as D

NAMES = sorted(A.WM_CASES)
VARIANTS = sorted(A.VARIANT_CASES)
WIDE = sorted(A.WIDE_CASES)
EVERY = NAMES + VARIANTS + WIDE
PER_UNIT_CASES = NAMES + VARIANTS                                  # the shape 96-50-20-31: the cases that carry the per-unit check


def _case(name):
    return next(d for d in (A.WM_CASES, A.VARIANT_CASES, A.WIDE_CASES) if name in d)[name]()


def _stage_preactivations(c):
    run = lambda: D.stage_inputs(c.cfg, c.p.x0, c.p.bcs, c.w)
    return D.preactivations(c.cfg, c.w, D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run())


def _bounds():
    """(solution, total, gradient, worst layer block) of tests/test_gpu_activation_range.py"""
    from tests.test_gpu_parity import GRAD_REL, LOSS_RTOL, SOL_ATOL
    return SOL_ATOL, LOSS_RTOL, GRAD_REL, 4 * GRAD_REL


def _errors(c, tot, g, sol):
    from tests.test_gpu_parity import _rel
    blk, e = D.worst_block(g, c.g, c.blocks)
    ub, ue = A.worst_per_unit(g, c.g, c)
    return dict(sol_abs=float(np.abs(sol - c.sol).max()), loss_rel=abs(tot - c.tot) / abs(c.tot), grad_rel=float(_rel(g, c.g)), block_rel=e, block=blk,
                unit=ue, unit_block=ub)


@pytest.fixture(scope="module")
def port():
    """the float32 restatement's errors on every case, computed once: the C port; the float32 NumPy oracle for RKC2 and the step schedule"""
    from oracle import cref
    out = {}
    for name in EVERY:
        c = _case(name)
        if name in A.VARIANT_CASES:
            run = lambda: O.loss_and_grad(c.cfg, c.p.x0, c.p.bcs, c.w, c.truth, c.sc, dtype=np.float32)
            tot, _, g, sol = D.oracle_under_schedule(c.schedule, run) if hasattr(c, "schedule") else run()
        else:
            tot, _, g, sol = cref.loss_grad(c.cfg, c.p.x0, c.p.bcs, c.w, c.truth, c.sc, want_sol=True)
        out[name] = _errors(c, float(tot), g, sol)
    return out


@pytest.fixture(scope="module")
def preacts():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _stage_preactivations(_case(name))
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------------------------ the cases themselves
def test_cases_are_shared_read_only_and_built_on_distinct_nets():
    c = A.wm_case("mish", 21)
    assert A.WM_CASES["mish/21"]() is c and not c.w.flags.writeable and not c.g.flags.writeable
    assert c.truth.dtype == np.float32 and c.sol.shape == (21, D.FRAMES, 96) and c.cfg.substeps == D.SUBSTEPS and c.blocks == D.named_blocks(c.cfg)
    assert [n for n, _ in A.hidden_bias_blocks(c)] == ["uw/b1", "uw/b2", "vw/b1", "vw/b2", "wT/b1", "wT/b2"]
    base = D.weights(c.cfg, A.SEED)
    for (k, l, kind, s), (name, _) in zip(D.blocks(c.cfg), c.blocks):
        if kind == "b" and l < 2:
            assert np.array_equal(c.w[s], A.ladder("mish", s.stop - s.start, k)[0].astype(np.float32)), name
        elif kind == "b":
            assert np.array_equal(c.w[s], base[s]), name                # the output bias is the draw's
        else:
            assert (np.abs(c.w[s]) <= np.abs(base[s])).all() and (c.w[s] != 0).all(), name
    assert np.array_equal(c.w_truth, D.weights(c.cfg, A.SEED + 1, divisor=1e2)) and c.tot > 0.1


@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("width", [20, 50, 400])
def test_a_ladder_has_its_rungs_and_a_third_of_ordinary_units(act, width):
    for net in range(3):
        z, s = A.ladder(act, width, net)
        assert z.shape == s.shape == (width,) and len(set(z.tolist())) == width and (z != 0).all()
        assert (s == 1).sum() >= width / 3 and (np.abs(z[s == 1]) <= 2.2).all()
        assert sorted(z[s != 1].tolist()) == sorted(v for v, _ in A.RUNGS[act])
    assert not np.array_equal(A.ladder(act, width, 0)[0], A.ladder(act, width, 1)[0])


# ------------------------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("name", EVERY)
def test_every_tail_interval_holds_a_unit_at_every_stage(name, preacts):
    c = _case(name)
    Z = preacts(name)
    assert sorted(Z) == [(k, l) for k in range(3) for l in range(len(c.cfg.layer_sizes) - 2)]
    for key, z in Z.items():
        lo, hi = z.min(axis=0), z.max(axis=0)
        for a, b, count in A.REQUIRED[c.act]:
            need = count if count >= 1 else int(np.ceil(count * z.shape[1]))
            inside = (lo >= a) & (hi <= b) if (a, b) == (-3.0, 3.0) else (lo > a) & (hi < b)
            assert inside.sum() >= need, (key, a, b, int(inside.sum()), need)
        if c.act in ("relu", "leakyrelu"):
            assert np.abs(z).min() >= 1e-4, (key, float(np.abs(z).min()))          # float32 cannot move a kink
    assert np.abs(c.sol).max() < 10 and c.tot > 0.1                     # the solve is stable and the loss is not near zero


def test_the_required_intervals_are_the_tails():
    """both sides of every clamp and of the overflow; both signs beyond 100 for all"""
    ln_flt_max = float(np.log(np.float64(np.finfo(np.float32).max)))
    assert 88.72 < ln_flt_max < 88.73
    for act in A.ACTS:
        iv = [(a, b) for a, b, _ in A.REQUIRED[act]]
        assert (-3.0, 3.0) in iv and (100.0, np.inf) in iv and (-np.inf, -100.0) in iv
    m, t, s, r = ([(a, b) for a, b, _ in A.REQUIRED[k]] for k in ("mish", "tanh", "swish", "relu"))
    assert (19.0, 20.0) in m and (20.0, 21.0) in m and (40.0, np.inf) in m and (-30.0, -10.0) in m and (-104.0, -87.4) in m
    assert {(14.0, 15.0), (15.0, 16.0), (-15.0, -14.0), (-16.0, -15.0), (5.0, 9.0), (-9.0, -5.0)} <= set(t)
    assert (-90.0, -88.73) in s and (-88.72, -87.0) in s and (30.0, np.inf) in s
    assert (1e-4, 1e-3) in r and (-1e-3, -1e-4) in r and A.REQUIRED["leakyrelu"] is A.REQUIRED["relu"]
    # exp(z) is a float32 subnormal on (-103.9, -87.4): below FLT_MIN, not yet rounded to 0; every rung placed in the interval is inside that
    assert np.exp(-87.4) < np.finfo(np.float32).tiny and np.float32(np.exp(-103.9)) > 0
    assert all(-103.9 < v < -87.4 for v, _ in A.RUNGS["mish"] if -104.0 < v < -87.4) and any(-104.0 < v < -87.4 for v, _ in A.RUNGS["mish"])


# ------------------------------------------------------------------------------------------------------------------ the float32 port
@pytest.mark.parametrize("name", EVERY)
def test_float32_restatement_is_within_a_tenth_of_every_bound(name, port):
    e = port[name]
    sol_b, loss_b, grad_b, block_b = _bounds()
    print("activation range, %s (%s): %s" % (name, "numpy float32" if name in A.VARIANT_CASES else "C port", e))
    from tests.test_gpu_parity import _record
    _record("activation_range_float32/" + name, sol_abs=e["sol_abs"], loss_rel=e["loss_rel"], grad_rel=e["grad_rel"], unit=e["unit"],
            **{"block_rel:" + e["block"]: e["block_rel"]})
    assert e["sol_abs"] <= sol_b / 10
    assert e["loss_rel"] <= loss_b / 10
    assert e["grad_rel"] <= grad_b / 10
    assert e["block_rel"] <= block_b / 10, e["block"]
    if name in PER_UNIT_CASES:
        assert e["unit"] <= A.PER_UNIT / 10, e["unit_block"]


def test_per_unit_figure_is_ten_times_the_ports_worst(port):
    """A.PER_UNIT is ten times the C port's worst per-entry error over the committed cases, rounded up by a quarter; the measured value is the one
    the cases module's docstring states"""
    name, e = max(((n, port[n]) for n in PER_UNIT_CASES), key=lambda t: t[1]["unit"])
    print("activation range: the C port's worst per-entry error of a hidden bias gradient is %.3e (%s, %s); PER_UNIT = %.1e" %
          (e["unit"], name, e["unit_block"], A.PER_UNIT))
    assert A.PER_UNIT / 20 <= e["unit"] <= A.PER_UNIT / 10
    assert abs(e["unit"] - A.PORT_WORST) <= 0.25 * A.PORT_WORST
    assert ("%.1e" % A.PORT_WORST) in A.__doc__ and ("PER_UNIT = %.1e" % A.PER_UNIT) in A.__doc__


@pytest.mark.parametrize("name", PER_UNIT_CASES)
def test_the_relative_class_of_the_per_unit_check_is_populated(name, preacts):
    c = _case(name)
    Z = preacts(name)
    for (blk, s), key in zip(A.hidden_bias_blocks(c), sorted(Z)):
        r = np.abs(c.g[s])
        big = r >= 1e-3 * r.max()
        assert big.sum() >= 0.25 * big.size, (blk, int(big.sum()))
        if c.act == "tanh":
            reach = np.abs(Z[key]).max(axis=0)
            assert big[reach < 3].sum() >= 0.9 * (reach < 3).sum() and not big[reach >= 9].any(), blk


# ------------------------------------------------------------------------------------------------------------------ the inputs can tell a wrong kernel
def _f32(f):
    return lambda z: f(np.asarray(z, np.float32)).astype(np.float64)


def _mish_unclamped_float32(z):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(z)
        n = e * (e + np.float32(2))
        return z * (n / (n + np.float32(2)))


MUTANTS = {
    # name: (activation, replacement of O.act or None, replacement of O.act_grad or None)
    "tanh clamped at 4": ("tanh", lambda z: np.tanh(np.clip(z, -4, 4)), lambda z: 1 - np.tanh(np.clip(z, -4, 4)) ** 2),
    "mish in float32 without the clamp": ("mish", _f32(_mish_unclamped_float32), None),
    "swish' without z s (1 - s)": ("swish", None, lambda z: O._sigmoid(z)),
    "mish' = tanh(softplus(z))": ("mish", None, lambda z: np.tanh(O._softplus(z))),
    "leakyrelu slope 0.02": ("leakyrelu", lambda z: np.maximum(0.02 * z, z), lambda z: np.where(z > 0, 1.0, 0.02)),
}


@pytest.mark.parametrize("n", [21, 70])
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_wrong_activation_misses_a_bound_by_ten(mutant, n, monkeypatch):
    act_name, f, df = MUTANTS[mutant]
    c = A.wm_case(act_name, n)
    act, act_grad = O.act, O.act_grad
    if f is not None:
        monkeypatch.setattr(O, "act", lambda name, z: f(z) if name == act_name else act(name, z))
    if df is not None:
        monkeypatch.setattr(O, "act_grad", lambda name, z: df(z) if name == act_name else act_grad(name, z))
    with np.errstate(all="ignore"):
        tot, _, g, sol = O.loss_and_grad(c.cfg, c.p.x0, c.p.bcs, c.w, c.truth, c.sc)
    monkeypatch.undo()
    if not (np.isfinite(sol).all() and np.isfinite(g).all() and np.isfinite(tot)):
        print("activation range, mutant %r at %d columns: not finite (the GPU tests assert finiteness first)" % (mutant, n))
        assert mutant == "mish in float32 without the clamp"
        return
    e = _errors(c, tot, g, sol)
    sol_b, loss_b, grad_b, block_b = _bounds()
    ratios = dict(sol=e["sol_abs"] / sol_b, total=e["loss_rel"] / loss_b, grad=e["grad_rel"] / grad_b, block=e["block_rel"] / block_b, unit=e["unit"] / A.PER_UNIT)
    print("activation range, mutant %r at %d columns: error / bound %s" % (mutant, n, {k: "%.3g" % v for k, v in ratios.items()}))
    assert max(ratios.values()) >= 10, ratios
    if f is None:                                                        # a wrong derivative leaves the solve alone: the gradient checks see it
        assert ratios["sol"] == 0 and max(ratios["grad"], ratios["block"], ratios["unit"]) >= 10


def test_the_oracle_hands_a_nan_on_for_every_activation():
    """what the NaN tests of the GPU file expect of the kernels is what the oracle (and Flux) does: act(NaN) = NaN for all five"""
    z = np.array([np.nan, 1.0])
    for a in A.ACTS:
        assert np.isnan(O.act(a, z)[0]) and np.isfinite(O.act(a, z)[1]), a


# ------------------------------------------------------------------------------------------------------------------ the forward-only families
def test_forward_weights_keep_a_saturated_unit_visible_in_the_output():
    cfg = A.wm_case("mish", 21).cfg
    a, b = A.forward_weights(cfg, "mish"), A.wm_case("mish", 21).w
    for (k, l, kind, s) in D.blocks(cfg):
        if (l, kind) == (2, "W"):
            assert np.allclose(a[s] * (A.OUT_SCALE / A.FORWARD_OUT_SCALE), b[s], rtol=1e-6, atol=0)
            assert 0.1 < 120 * np.abs(a[s]).max() < 10                  # a unit at 120 against an output bias of U(-1, 1)
        else:
            assert np.array_equal(a[s], b[s])


@pytest.mark.parametrize("act,sizes", [(a, (96, 50, 20, 31)) for a in A.EMBED_ACTS] + [(a, A.GENERIC_SHAPE) for a in A.GENERIC_ACTS + ("tanh",)])
def test_float32_forcings_are_within_a_tenth_of_their_bounds(act, sizes):
    """the embedding's float64 restatement run in float32 (tests/wm_embed_common.py), against DZ_BOUND of tests/test_gpu_wm_embed.py on the
    net-split shape and tests/wm_generic_cases.py's per net on 96-400-31"""
    from tests import wm_embed_common as W
    from tests import wm_generic_cases as C
    c = A.embed_case(act, sizes)
    d = C.rel_dist(W.dz_fluxes(c.p.cfg, c.w, c.u, c.v, c.T, c.top, W.LZ, np.float32), c.ref)
    print("activation range, float32 forcings %s %s: %s" % (act, sizes, ["%.2e" % v for v in d]))
    from tests.test_gpu_wm_embed import DZ_BOUND
    bound = [DZ_BOUND] * 3 if len(sizes) == 4 else [C.DZ_BOUND[k] for k in C.NETS]
    assert all(np.isfinite(r).all() for r in c.ref) and all(v <= b / 10 for v, b in zip(d, bound)), (d, bound)
    Z = D.preactivations(c.p.cfg, c.w, c.p.x0.astype(np.float64))       # the embedding's inputs are x0 in the ocean model's units
    for z in Z.values():
        assert (z.min(axis=0) > 100).any() and (z.max(axis=0) < -100).any() and ((np.abs(z).max(axis=0) <= 3).sum() >= z.shape[1] / 3)


@pytest.mark.parametrize("n", A.FORWARD_N)
def test_float32_profile_fluxes_are_within_a_tenth_of_their_bound(n):
    """FLUX_BOUND of tests/test_gpu_wm_profile.py"""
    from tests import wm_profile_restatement as R
    from tests.test_gpu_parity import _rel
    from tests.test_gpu_wm_profile import FLUX_BOUND
    c = A.profile_case(n)
    for k in range(2):
        cfg = R.member_cfg(c.cfg, c.rows[k])
        f64, f32 = R.fluxes(cfg, c.W[k], c.sol[k], c.p.bcs), R.fluxes(cfg, c.W[k], c.sol[k], c.p.bcs, dtype=np.float32)
        assert all(_rel(a[..., 1:32], b[..., 1:32]) <= FLUX_BOUND / 10 for a, b in zip(f32, f64))


@pytest.mark.parametrize("n", A.FORWARD_N)
@pytest.mark.parametrize("act", A.PRETRAIN_ACTS)
def test_float32_pretraining_is_within_a_tenth_of_its_bounds(act, n):
    """tests/pretrain_cases.py's float32 restatement against TOL_LOSS, TOL_W and TOL_B of tests/test_gpu_pretrain.py"""
    from tests import pretrain_cases as PC
    from tests.test_gpu_pretrain import TOL_B, TOL_LOSS, TOL_W
    s = A.pretrain_case(act, n)
    m, loss = A.pretrain_moment(s, PC.f32_loss_grad, np.float32)
    errs = PC.block_errors(s.cfg, m, s.m_ref)
    print("activation range, float32 pretraining %s n=%d: loss %.2e, blocks %s" % (act, n, abs(loss - s.loss_ref) / s.loss_ref, errs))
    assert abs(loss - s.loss_ref) / s.loss_ref <= TOL_LOSS / 10 and PC.worst(errs, "W") <= TOL_W / 10 and PC.worst(errs, "b") <= TOL_B / 10
    assert min(np.linalg.norm(s.m_ref[sl]) for _, sl in PC.blocks(s.cfg)) > 0
