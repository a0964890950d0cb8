"""Every hand-written form of the five activations held to float64 in its TAILS, and a NaN pre-activation held to reach the loss.

The cases (tests/activation_range_cases.py) are distinct, biased wind-mixing nets whose hidden bias blocks carry a ladder of pre-activations: both
sides of mish's clamp at 20 and of tanh's at +-15, both sides of ln FLT_MAX = 88.72 where swish's exp(-z) overflows, the range where exp(z) is a
float32 subnormal, |z| = 120, and 2e-4 ... 8e-4 on either side of the relu / leakyrelu kink.  tests/test_activation_range_host.py asserts on the CPU
that every interval is occupied at every stage evaluation, that a float32 restatement sits within a tenth of every bound used here, and that five
wrong activations each miss one of these bounds by ten or more.

Bounds: SOL_ATOL, LOSS_RTOL, GRAD_REL of tests/test_gpu_parity.py against the float64 oracle; 4 GRAD_REL for the worst layer block, as
tests/test_gpu_tile_ensemble.py has it; and, on the shape 96-50-20-31, the per-unit check of the hidden bias gradients at `A.PER_UNIT` (ten times the
float32 port's own worst, see the cases module).  Every case asserts the plan and that a second call returns the same bits (`_run` of
tests/test_gpu_distinct_nets.py).  COLNDE_RECORD_ERRORS=1 records what was measured.

NaN: tanh and relu clamp with minNum / maxNum, which answer the other operand to a NaN; the kernels hand the NaN on with one compare and select
(csrc/colnde_dev.h, csrc/regtile_dev.h).  Section 3 holds all five activations to it on the three engines, in both ensembles and in the
any-architecture embedding, and holds tanh(+-Inf) = +-1 and relu(-Inf) = 0 to what they were.  With the fminf / fmaxf forms the tanh and relu
cases of section 3 fail (12 engine cases, both ensembles, the embedding) and the mish, swish and leakyrelu ones pass."""
import numpy as np
import pytest

from tests import activation_range_cases as A
from tests import distinct_nets as D
from tests.test_gpu_distinct_nets import ENGINE_N, MAS, _assert_engine_plan, _run

pytestmark = pytest.mark.gpu


def _check(label, c, got, per_unit=True):
    """figures printed and recorded first; then every bound"""
    from tests.test_gpu_parity import GRAD_REL, LOSS_RTOL, SOL_ATOL, _record, _rel
    sol, (lt, lterms), (tot, terms, grad) = got
    assert np.isfinite(sol).all() and np.isfinite(grad).all() and np.isfinite(lterms).all() and np.isfinite(terms).all()
    blocks = D.block_errors(grad, c.g, c.blocks)
    blk, blk_e = D.worst_block(grad, c.g, c.blocks)
    errs = dict(sol_abs=float(np.abs(sol - c.sol).max()), loss_rel=abs(lt - c.tot) / abs(c.tot), loss_grad_total_rel=abs(tot - c.tot) / abs(c.tot),
                grad_rel=float(_rel(grad, c.g)))
    units = A.per_unit_errors(grad, c.g, c) if per_unit else []
    ub, ue = A.worst_per_unit(grad, c.g, c) if per_unit else ("-", 0.0)
    print("activation range, %s: %s, worst block %s %.3e, worst unit %s %.3e" % (label, {k: "%.3e" % v for k, v in errs.items()}, blk, blk_e, ub, ue))
    print("    blocks: " + " ".join("%s %.1e" % (n, e) for n, e, _ in blocks))
    print("    units (relative class, absolute class / floor, size of the relative class): " + " ".join("%s %.1e %.1e %d" % u for u in units))
    _record("activation_range/" + label, **errs, unit=ue, **{"block_rel:" + blk: blk_e})
    assert errs["sol_abs"] < SOL_ATOL
    assert np.isclose(lt, c.tot, rtol=LOSS_RTOL, atol=0) and np.isclose(tot, c.tot, rtol=LOSS_RTOL, atol=0)
    slack = 1e-3 * LOSS_RTOL * float(np.sum(c.terms))                     # the terms as tests/test_gpu_distinct_nets.py holds them
    np.testing.assert_allclose(lterms, c.terms, rtol=LOSS_RTOL, atol=slack)
    np.testing.assert_allclose(terms, c.terms, rtol=LOSS_RTOL, atol=slack)
    assert errs["grad_rel"] < GRAD_REL
    bad = [(n, e) for n, e, _ in blocks if not e < 4 * GRAD_REL]
    assert not bad, bad
    bad = [u for u in units if not (u[1] < A.PER_UNIT and u[2] < A.PER_UNIT)]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ 2a, 2b. engines x activations x arithmetics
@pytest.mark.parametrize("ma", MAS)
@pytest.mark.parametrize("act", A.ACTS)
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_engines_activations_arithmetics(engine, act, ma):
    """forward, loss and loss_grad on 96-50-20-31; the per-unit check of the six hidden bias blocks is part of `_check`"""
    import colnde
    n = ENGINE_N[engine]
    c = A.wm_case(act, n)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, n, engine=engine, matrix_arithmetic=ma))
    _assert_engine_plan(plan, engine, ma)
    if engine == 0:
        assert plan["split_rich_tape"] and plan["dw_taped"]
        assert plan["bf16x3_forward"] == plan["bf16x3_adjoint"] == (ma == "bf16x3_exact")
    if engine == 2:
        assert plan["z1_taped"] and plan["n_blocks"] == 1
    _check("engine%d/%s/%s/%d" % (engine, act, ma, n), c, got)


# ------------------------------------------------------------------------------------------------------------------ 2c. the other tile16 kernel forms
def _wide(act, shape):
    return A.WIDE_CASES["%s/%s/%d" % (act, shape, A.WIDE_N)]()


@pytest.mark.parametrize("act", A.WIDE_ACTS)
@pytest.mark.parametrize("shape", sorted(A.WIDE_SHAPES))
def test_tile16_rows_in_lds_and_in_global_memory(shape, act):
    """96-400-31: activation rows in LDS, weights streamed; 96-400-400-31: rows in global memory, bf16 planes.  The per-unit figure is measured on
    96-50-20-31 and is not applied to the 400-wide blocks."""
    import colnde
    c = _wide(act, shape)
    got, plan, text = _run(c, lambda: colnde.ColumnNDE(c.cfg, A.WIDE_N, engine=1, matrix_arithmetic="bf16x3_exact"))
    _assert_engine_plan(plan, 1, "bf16x3_exact")
    assert ("activation_rows=global_memory" in text) == (shape == "96-400-400-31"), text
    _check("tile16/%s/%s/%d" % (shape, act, A.WIDE_N), c, got, per_unit=False)


@pytest.mark.parametrize("act", A.WIDE_ACTS)
@pytest.mark.parametrize("shape", sorted(A.WIDE_SHAPES))
def test_tile_ensemble_rows_are_the_single_handles_bits(shape, act):
    """TileNDEEnsemble, 2 members on the same ladders (the second member: the next seed's draw): row k is the single tile16 handle's bits"""
    from tests import test_gpu_tile_ensemble as T
    c = _wide(act, shape)
    W = np.stack([c.w, A.weights(c.cfg, A.SEED + 5, act)])
    assert not np.array_equal(W[0], W[1])
    got = T._ensemble(c.p, c.truth, W, None, "bf16x3_exact")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and "models=2" in got[3] and "tile_ensemble" in got[3]
    T._assert_rows(c.p, c.truth, got, W, None, "bf16x3_exact", range(2))


# ------------------------------------------------------------------------------------------------------------------ 2d. net-split variants
def test_net_split_rkc2():
    import colnde
    c = A.VARIANT_CASES["swish/21/rkc2"]()
    assert colnde.rkc_stages(c.cfg) >= 2
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21))
    assert plan["split_forward"] and plan["split_adjoint"], plan
    _check("net_split_rkc2/swish/21", c, got)


def test_net_split_step_schedule():
    import colnde
    c = A.VARIANT_CASES["relu/21/schedule"]()

    def prepare(nde):
        nde.set_schedule(c.schedule)
        assert nde.schedule() == c.schedule and nde.n_steps == sum(c.schedule)
    got, plan, text = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21), prepare)
    assert plan["split_forward"] and plan["split_adjoint"] and "schedule=%d/%d intervals" % (sum(c.schedule), len(c.schedule)) in text, (plan, text)
    _check("net_split_schedule/relu/21", c, got)


def test_net_split_plain_tape(monkeypatch):
    """COLNDE_T16_SPLIT_RICH=0: the net-split adjoint recomputes the activation pairs from the pre-activation tape"""
    import colnde
    monkeypatch.setenv("COLNDE_T16_SPLIT_RICH", "0")
    c = A.wm_case("tanh", 21)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21))
    assert plan["split_forward"] and plan["split_adjoint"] and not plan["split_rich_tape"], plan
    _check("net_split_plain_tape/tanh/21", c, got)


def test_regtile_recomputed_layer1(monkeypatch):
    """COLNDE_RT_ZTAPE=0: rt_act_grad on a layer 1 recomputed from the stage tape instead of the taped Z1"""
    import colnde
    monkeypatch.setenv("COLNDE_RT_ZTAPE", "0")
    c = A.wm_case("leakyrelu", 70)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 70, engine=2))
    assert plan["engine"] == 2 and not plan["z1_taped"], plan
    _check("regtile_no_z1_tape/leakyrelu/70", c, got)


# ------------------------------------------------------------------------------------------------------------------ 2e. forward-only kernel families
# The same ladders under `A.forward_weights` (output layer / 30: nothing is integrated), against each family's float64 restatement at the
# tolerance of the family's own test; tests/test_activation_range_host.py holds the float32 restatements to a tenth of each.
@pytest.mark.parametrize("n", A.FORWARD_N)
@pytest.mark.parametrize("act", A.EMBED_ACTS)
def test_embedded_forcing_on_the_net_split_shape(act, n):
    """colnde_wm_infer_dz_flux; DZ_BOUND of tests/test_gpu_wm_embed.py::test_forcing_parity_host_and_device_twins"""
    import colnde
    from tests import wm_embed_common as W
    from tests.test_gpu_parity import _record
    from tests.test_gpu_wm_embed import DZ_BOUND, NETS, _dz_errors
    c = A.first_columns(A.embed_case(act), n)
    with colnde.ColumnNDE(c.p.cfg, 4) as nde:
        assert "wm_infer=f32" in nde.describe()
        got = nde.wm_infer_dz_flux(c.w, c.u, c.v, c.T, c.top, W.LZ)
        again = nde.wm_infer_dz_flux(c.w, c.u, c.v, c.T, c.top, W.LZ)
    errs = _dz_errors(got, c.ref)
    print("activation range, wm_infer %s n=%d: rel err uw %.3e vw %.3e wT %.3e" % ((act, n) + tuple(errs)))
    _record("activation_range/wm_infer/%s/%d" % (act, n), **dict(zip(NETS, errs)))
    assert all(np.isfinite(g).all() and np.array_equal(g, a) for g, a in zip(got, again))
    for nm, e in zip(NETS, errs):
        assert e <= DZ_BOUND, (nm, e)


def _generic(act):
    return A.embed_case(act, A.GENERIC_SHAPE)


@pytest.mark.parametrize("n", A.FORWARD_N)
@pytest.mark.parametrize("act", A.GENERIC_ACTS)
def test_embedded_forcing_of_any_architecture(act, n):
    """colnde_ensemble_wm_embedded with a single 96-400-31 handle as K = 1; DZ_BOUND of tests/wm_generic_cases.py, as
    tests/test_gpu_wm_generic.py::test_forcing holds it"""
    import colnde
    from tests import wm_generic_cases as C
    from tests.test_gpu_parity import _record
    from tests.test_gpu_wm_generic import DZ, _call, _same
    c = A.first_columns(_generic(act), n)
    with colnde.ColumnNDE(c.p.cfg, 4) as nde:
        assert "wm_embed=generic_f32" in nde.describe()
        got = _call(nde, c)
        _same(got, _call(nde, c), "two launches")
    errs = C.rel_dist([got[k] for k in DZ], c.ref)
    print("activation range, wm_generic %s n=%d: rel err uw %.3e vw %.3e wT %.3e" % ((act, n) + tuple(errs)))
    _record("activation_range/wm_generic/%s/%d" % (act, n), **dict(zip(C.NETS, errs)))
    for nm, e in zip(C.NETS, errs):
        assert e <= C.DZ_BOUND[nm], (nm, e)


@pytest.mark.parametrize("n", A.FORWARD_N)
def test_profile_of_the_networks_own_fluxes(n):
    """colnde_ensemble_profile, two members, the closure's constants at 0 for the call; FLUX_BOUND and BOUNDARY_ATOL of
    tests/test_gpu_wm_profile.py::test_networks_only_rows"""
    import colnde
    from tests import wm_profile_restatement as R
    from tests.test_gpu_parity import _record, _rel
    from tests.test_gpu_wm_profile import BOUNDARY_ATOL, FLUX_BOUND, NAMES
    c = A.profile_case(n)
    with colnde.ColumnNDEEnsemble(c.cfg, n, 2) as ens:
        ens.set_problem(c.p.x0, c.p.bcs, c.truth)
        assert "wm_profile=f32" in ens.describe()
        got = ens.profile(c.W, c.sol, physics=c.rows, Ri=False, losses=False)
    worst = 0.0
    for k in range(2):
        ref = R.fluxes(R.member_cfg(c.cfg, c.rows[k]), c.W[k], c.sol[k], c.p.bcs)
        for nm, r, g in zip(NAMES, ref, (got.uw[k], got.vw[k], got.wT[k])):
            assert g.shape == (n, c.cfg.n_save, 33) and np.isfinite(g).all()
            e = float(_rel(g[..., 1:32], r[..., 1:32]))
            print("activation range, wm_profile %s n=%d model %d %s: rel %.3g" % (A.PROFILE_ACT, n, k, nm, e))
            worst = max(worst, e)
            assert e < FLUX_BOUND, (k, nm, e)
            assert np.abs(g[..., [0, 32]] - r[..., [0, 32]]).max() <= BOUNDARY_ATOL, (k, nm)
    _record("activation_range/wm_profile/%s/%d" % (A.PROFILE_ACT, n), flux_rel=worst)


@pytest.mark.parametrize("n", A.FORWARD_N)
@pytest.mark.parametrize("act", A.PRETRAIN_ACTS)
def test_flux_pretraining_loss_and_gradient(act, n):
    """colnde_pretrain_flux_dev (dev_act and dev_act_grad in csrc/pretrain_sample.h): one call over n samples with zero moments, beta = (0.5, 0.5)
    and eta = 0, so that m = sum_i 2^-(n - i) g_i is linear in the samples' gradients and theta keeps its bits; TOL_LOSS, TOL_W and TOL_B of
    tests/test_gpu_pretrain.py::test_single_sample_loss_and_gradient"""
    import colnde
    from colnde.flux_compat import ADAM
    from tests import pretrain_cases as PC
    from tests.test_gpu_parity import _record
    from tests.test_gpu_pretrain import TOL_B, TOL_LOSS, TOL_W, _dev_sample, _moments, _np, _t
    s = A.pretrain_case(act, n)
    X, B, Y = _dev_sample(s)
    theta, m, v = _t(s.theta), _t(_moments(s)), _t(_moments(s))
    opt = ADAM(0.0, (0.5, 0.5))
    opt.beta_t = [0.5, 0.5]
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        loss = eng.pretrain_flux(s.k, theta, m, v, X, B, Y, None, s.gs, opt)
    theta, m = _np(theta), _np(m)
    errs = PC.block_errors(s.cfg, m[s.net], s.m_ref)
    e_loss = abs(loss - s.loss_ref) / s.loss_ref
    print("activation range, pretrain %s n=%d: loss %.6e rel err %.2e; blocks of m %s" % (act, n, loss, e_loss, " ".join("%s %.2e" % kv for kv in errs.items())))
    _record("activation_range/pretrain/%s/%d" % (act, n), loss_rel=e_loss, W=PC.worst(errs, "W"), b=PC.worst(errs, "b"))
    np.testing.assert_array_equal(theta, s.theta)
    assert np.isfinite(m[s.net]).all()
    assert e_loss < TOL_LOSS
    assert PC.worst(errs, "W") < TOL_W, errs
    assert PC.worst(errs, "b") < TOL_B, errs


# ------------------------------------------------------------------------------------------------------------------ 3. a NaN reaches the loss
def _nan_sites(cfg):
    """{name: index}: one layer-1 weight of net 1; one layer-2 bias of net 2"""
    where = {(k, l, kind): s for k, l, kind, s in D.blocks(cfg)}
    return {"vw/W1": where[(1, 0, "W")].start + 1234, "wT/b2": where[(2, 1, "b")].start + 9}


@pytest.mark.parametrize("engine,act,ma", [(e, a, "bf16x3_exact") for e in (0, 1, 2) for a in A.ACTS] +
                         [(e, a, "f32_mfma") for e in (0, 1, 2) for a in ("tanh", "relu")])
def test_a_nan_weight_reaches_the_loss(engine, act, ma):
    """NaN only: tanh(+-Inf) is legitimately finite, and the split turns an Inf into NaN by design"""
    import colnde
    n = ENGINE_N[engine]
    c = A.wm_case(act, n)
    with colnde.ColumnNDE(c.cfg, n, engine=engine, matrix_arithmetic=ma) as nde:
        nde.set_problem(c.p.x0, c.p.bcs, c.truth)
        clean = (nde.forward(c.w), nde.loss(c.w, c.sc), nde.loss_grad(c.w, c.sc))
        _assert_engine_plan(nde.plan(), engine, ma)
        assert np.isfinite(clean[0]).all() and np.isfinite(clean[2][2]).all()
        for name, i in _nan_sites(c.cfg).items():
            w = np.array(c.w)
            w[i] = np.nan
            sol = nde.forward(w)
            print("activation range, NaN in %s, engine %d, %s, %s: %d of %d solution entries are not finite" %
                  (name, engine, act, ma, int((~np.isfinite(sol)).sum()), sol.size))
            assert not np.isfinite(sol).all(), name
            with pytest.raises(colnde.ColndeError, match="not finite"):
                nde.loss(w, c.sc)
            with pytest.raises(colnde.ColndeError, match="not finite"):
                nde.loss_grad(w, c.sc)
            again = (nde.forward(c.w), nde.loss(c.w, c.sc), nde.loss_grad(c.w, c.sc))
            assert np.array_equal(again[0], clean[0]), name
            assert again[1][0] == clean[1][0] and np.array_equal(again[1][1], clean[1][1]), name
            assert again[2][0] == clean[2][0] and np.array_equal(again[2][1], clean[2][1]) and np.array_equal(again[2][2], clean[2][2]), name


def _assert_member_2_alone_is_not_finite(base, nanr, n_params):
    assert np.isfinite(base).all()
    assert not np.isfinite(nanr[2, n_params + 6])
    others = np.arange(base.shape[0]) != 2
    assert np.isfinite(nanr[others]).all() and np.array_equal(nanr[others], base[others])


def test_a_nan_hidden_weight_shows_in_its_tile_ensemble_row():
    """tanh 96-24-31, K = 5, the NaN in a layer-1 weight of member 2's net 1"""
    from tests import test_gpu_tile_ensemble as T
    from tests.test_gpu_ensemble import PHYS
    p, truth = T._problem("96-24-31_tanh", 8)
    W = T._weights(p.cfg, 5)
    Wn = W.copy()
    Wn[2, _nan_sites(p.cfg)["vw/W1"]] = np.nan
    base = T._ensemble(p, truth, W, PHYS, "bf16x3_exact")[1]
    _assert_member_2_alone_is_not_finite(base, T._ensemble(p, truth, Wn, PHYS, "bf16x3_exact")[1], p.cfg.n_params)


def test_a_nan_hidden_weight_shows_in_its_column_ensemble_row():
    """ColumnNDEEnsemble (net-split), tanh 96-50-20-31, K = 5, the NaN in a layer-2 bias of member 2's net 2"""
    from tests import test_gpu_ensemble as E
    p, truth = E._problem(8, activations=("tanh", "tanh", "identity"))
    W = E._weights(p.cfg, 5)
    Wn = W.copy()
    Wn[2, _nan_sites(p.cfg)["wT/b2"]] = np.nan
    base = E._ensemble(p, truth, W, E.PHYS, "bf16x3_exact")[1]
    _assert_member_2_alone_is_not_finite(base, E._ensemble(p, truth, Wn, E.PHYS, "bf16x3_exact")[1], p.cfg.n_params)


def test_a_nan_hidden_weight_shows_in_the_embedded_forcing_where_the_restatement_has_it():
    """the any-architecture embedding, tanh 96-400-31, a layer-1 weight of net 1: every dz_vw value is NaN, dz_uw and dz_wT keep their bits"""
    import colnde
    from tests import wm_embed_common as W
    from tests.test_gpu_wm_generic import DZ, _call
    c = A.first_columns(_generic("tanh"), 8)
    w = np.array(c.w)
    w[_nan_sites(c.p.cfg)["vw/W1"]] = np.nan
    with np.errstate(invalid="ignore"):
        ref = W.dz_fluxes(c.p.cfg, w, c.u, c.v, c.T, c.top, W.LZ)
    assert np.isnan(ref[1]).all() and np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    with colnde.ColumnNDE(c.p.cfg, 4) as nde:
        clean = _call(nde, c)
        c.w = w
        got = _call(nde, c)
    for k, r in zip(DZ, ref):
        assert np.array_equal(np.isnan(got[k]), np.isnan(r)), k
    assert np.array_equal(got["dz_uw"], clean["dz_uw"]) and np.array_equal(got["dz_wT"], clean["dz_wT"]) and np.isfinite(clean["dz_vw"]).all()


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_infinite_preactivations_keep_their_values(act):
    """what the NaN select must leave alone: tanh(+-Inf) = +-1 and relu(-Inf) = 0, through hidden biases of +-Inf in the any-architecture embedding
    (f32 MFMA throughout: no split turns the Inf into a NaN); held to the float64 restatement at tests/wm_generic_cases.py's DZ_BOUND"""
    import colnde
    from tests import wm_embed_common as W
    from tests import wm_generic_cases as C
    from tests.test_gpu_wm_generic import DZ, _call
    c = A.first_columns(_generic(act), 8)
    b1 = {k: s for k, l, kind, s in D.blocks(c.p.cfg) if kind == "b" and l == 0}
    w = np.array(c.w)
    w[b1[0].start + 200] = -np.inf                                    # ordinary units: the rungs sit in the first 26 places
    if act == "tanh":
        w[b1[2].start + 201] = np.inf
    ref = W.dz_fluxes(c.p.cfg, w, c.u, c.v, c.T, c.top, W.LZ)
    assert all(np.isfinite(r).all() for r in ref) and not np.array_equal(ref[0], c.ref[0]) and np.array_equal(ref[2], c.ref[2]) == (act == "relu")
    c.w = w
    with colnde.ColumnNDE(c.p.cfg, 4) as nde:
        got = _call(nde, c)
    errs = C.rel_dist([got[k] for k in DZ], ref)
    print("activation range, wm_generic %s with infinite hidden biases: rel err uw %.3e vw %.3e wT %.3e" % ((act,) + tuple(errs)))
    for nm, e in zip(C.NETS, errs):
        assert e <= C.DZ_BOUND[nm], (nm, e)
