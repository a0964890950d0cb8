"""The training engines held to the float64 oracle on three DIFFERENT, BIASED nets whose activations bend (tests/distinct_nets.py).

Every other parity test of forward / loss / loss_grad runs at `synthetic.make_weights(..., same_init=True)` / 1e2: three copies of one net, zero
biases, pre-activations below 0.05.  There a wrong per-net weight offset, a wrong wave-to-net mapping, a dropped bias add or an activation pair that
is wrong away from 0 computes the same numbers, and a gradient block four orders below the norm can be anything.  Here the nets are separate draws
at O(1), every bias is U(-1, 1), the hidden pre-activations reach 3.5 to 3.9, and the smallest of the 18 layer blocks is 2e-4 of the gradient's
norm; tests/test_distinct_nets_host.py asserts all of that on the CPU, and that a float32 restatement of the same arithmetic sits within a tenth of
every bound used here.

Bounds: the existing constants of tests/test_gpu_parity.py and nothing else — SOL_ATOL, LOSS_RTOL (terms: rtol = LOSS_RTOL, atol = 1e-3 LOSS_RTOL
sum(terms), as test_split_kernels_against_oracle_and_tile16 has it), GRAD_REL for the whole vector AND for every layer block on its own; free
convection: FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL the same way.  Every case asserts the plan (the kernel meant is the kernel run) and that a second
call returns the same bits.  5 frames and 2 sub-steps unless said otherwise.  COLNDE_RECORD_ERRORS=1 records what was measured
(profiles/distinct_nets_errors.json keeps the last measuring run, the float32 restatement's distances beside it)."""
import numpy as np
import pytest

from tests import distinct_nets as D

pytestmark = pytest.mark.gpu

MAS = ("bf16x3_exact", "f32_mfma")
ENGINE_N = {0: 21, 1: 21, 2: 70}          # net-split (AUTO): a full 16-column tile and a ragged one; tile16; regtile: two full 32-column tiles and six columns


def _run(c, make, prepare=None):
    """forward, loss and loss_grad twice on one handle: ((sol, (loss, terms), (total, terms, grad)), plan, describe()), the two calls' bits compared"""
    with make() as nde:
        if prepare is not None:
            prepare(nde)
        nde.set_problem(c.p.x0, c.p.bcs, c.truth)
        a, b = [(nde.forward(c.w), nde.loss(c.w, c.sc), nde.loss_grad(c.w, c.sc)) for _ in range(2)]
        plan, text = nde.plan(), nde.describe()
    assert a[0] is not b[0] and np.array_equal(a[0], b[0])
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1])
    assert a[2][0] == b[2][0] and np.array_equal(a[2][1], b[2][1]) and np.array_equal(a[2][2], b[2][2])
    return a, plan, text


def _check(label, c, got, fc=False):
    """figures printed and recorded first; then every bound"""
    from tests.test_gpu_parity import FC_GRAD_REL, FC_LOSS_RTOL, FC_SOL_ATOL, GRAD_REL, LOSS_RTOL, SOL_ATOL, _record, _rel
    sol_b, loss_b, grad_b = (FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL) if fc else (SOL_ATOL, LOSS_RTOL, GRAD_REL)
    sol, (lt, lterms), (tot, terms, grad) = got
    assert np.isfinite(sol).all() and np.isfinite(grad).all() and np.isfinite(lterms).all() and np.isfinite(terms).all()
    blocks = D.block_errors(grad, c.g, c.blocks)
    blk, blk_e = D.worst_block(grad, c.g, c.blocks)
    errs = dict(sol_abs=float(np.abs(sol - c.sol).max()), loss_rel=abs(lt - c.tot) / abs(c.tot), loss_grad_total_rel=abs(tot - c.tot) / abs(c.tot),
                grad_rel=float(_rel(grad, c.g)))
    print("distinct nets, %s: %s, worst block %s %.3e" % (label, {k: "%.3e" % v for k, v in errs.items()}, blk, blk_e))
    print("    blocks: " + " ".join("%s %.1e" % (n, e) for n, e, _ in blocks))
    _record("distinct_nets/" + label, **errs, **{"block_rel:" + blk: blk_e})
    assert errs["sol_abs"] < sol_b
    if not fc:
        slack = 1e-3 * LOSS_RTOL * float(np.sum(c.terms))
        np.testing.assert_allclose(lterms, c.terms, rtol=LOSS_RTOL, atol=slack)
        np.testing.assert_allclose(terms, c.terms, rtol=LOSS_RTOL, atol=slack)
    assert np.isclose(lt, c.tot, rtol=loss_b, atol=0) and np.isclose(tot, c.tot, rtol=loss_b, atol=0)
    assert errs["grad_rel"] < grad_b
    bad = [(n, e) for n, e, _ in blocks if not e < grad_b]
    assert not bad, bad


def _assert_engine_plan(plan, engine, ma):
    if engine == 0:
        assert plan["engine"] == 1 and plan["split_forward"] and plan["split_adjoint"], plan
    else:
        assert plan["engine"] == engine and not plan["split_forward"] and not plan["split_adjoint"], plan
    assert plan["matrix_arithmetic"] == ma


# ------------------------------------------------------------------------------------------------------------------ a. engines x activations x arithmetics
@pytest.mark.parametrize("ma", MAS)
@pytest.mark.parametrize("act", D.ACTS)
@pytest.mark.parametrize("engine", [0, 1, 2])
def test_engines_activations_arithmetics(engine, act, ma):
    import colnde
    n = ENGINE_N[engine]
    c = D.wm_case(act, n)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, n, engine=engine, matrix_arithmetic=ma))
    _assert_engine_plan(plan, engine, ma)
    if engine == 0:
        assert plan["split_rich_tape"] and plan["dw_taped"]
        assert plan["bf16x3_forward"] == plan["bf16x3_adjoint"] == (ma == "bf16x3_exact")
    if engine == 2:
        assert plan["z1_taped"] and plan["n_blocks"] == 1
    _check("engine%d/%s/%s/%d" % (engine, act, ma, n), c, got)


# ------------------------------------------------------------------------------------------------------------------ b. the other code forms, mish
def test_net_split_plain_tape(monkeypatch):
    """COLNDE_T16_SPLIT_RICH=0: the net-split adjoint recomputes the activation pairs from the pre-activation tape"""
    import colnde
    monkeypatch.setenv("COLNDE_T16_SPLIT_RICH", "0")
    c = D.wm_case("mish", 21)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21))
    assert plan["split_forward"] and plan["split_adjoint"] and not plan["split_rich_tape"], plan
    _check("net_split_plain_tape/mish/21", c, got)


def test_regtile_recomputed_layer1(monkeypatch):
    """COLNDE_RT_ZTAPE=0: rt_act_grad on a layer 1 recomputed from the stage tape instead of the taped Z1 (that adjoint runs f32 MFMA)"""
    import colnde
    monkeypatch.setenv("COLNDE_RT_ZTAPE", "0")
    c = D.wm_case("mish", 70)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 70, engine=2))
    assert plan["engine"] == 2 and not plan["z1_taped"], plan
    _check("regtile_no_z1_tape/mish/70", c, got)


@pytest.mark.parametrize("switch", ["COLNDE_T16_DWTAPE", "COLNDE_T16_ZTAPE"])
def test_tile16_without_its_tapes(switch, monkeypatch):
    """COLNDE_T16_DWTAPE=0: the in-register adjoint kernels; COLNDE_T16_ZTAPE=0: the taped adjoint recomputes the forward GEMMs"""
    import colnde
    monkeypatch.setenv(switch, "0")
    c = D.wm_case("mish", 21)
    got, plan, text = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21, engine=1))
    assert plan["engine"] == 1 and not plan["split_forward"] and not plan["split_adjoint"], plan
    assert plan["dw_taped"] == (switch == "COLNDE_T16_ZTAPE") and (switch + "=0") in text.split("| env")[1], (plan, text)
    _check("tile16/%s=0/mish/21" % switch, c, got)


def test_net_split_rkc2():
    """the Richardson closure is smooth: the discrete adjoint of the RKC2 recurrence is exact"""
    import colnde
    c = D.wm_case("mish", 21, "rkc2")
    assert colnde.rkc_stages(c.cfg) >= 2
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21))
    assert plan["split_forward"] and plan["split_adjoint"], plan
    _check("net_split_rkc2/mish/21", c, got)


def test_net_split_step_schedule():
    """save interval i stepped with (2, 3, 2, 4)[i] RK4 steps"""
    import colnde
    c = D.wm_schedule_case("mish", 21)

    def prepare(nde):
        nde.set_schedule(c.schedule)
        assert nde.schedule() == c.schedule and nde.n_steps == sum(c.schedule)
    got, plan, text = _run(c, lambda: colnde.ColumnNDE(c.cfg, 21), prepare)
    assert plan["split_forward"] and plan["split_adjoint"] and "schedule=%d/%d intervals" % (sum(c.schedule), len(c.schedule)) in text, (plan, text)
    _check("net_split_schedule/mish/21", c, got)


@pytest.mark.parametrize("engine", [0, 1, 2])
def test_one_column_alone(engine):
    import colnde
    c = D.wm_case("mish", 1)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 1, engine=engine))
    _assert_engine_plan(plan, engine, "bf16x3_exact")
    _check("one_column/engine%d/mish" % engine, c, got)


# ------------------------------------------------------------------------------------------------------------------ c. ensemble
@pytest.mark.parametrize("ma", MAS)
@pytest.mark.parametrize("n", [8, 40])
def test_ensemble_of_distinct_members(n, ma):
    """ColumnNDEEnsemble, K = 3, member k's weights of seed 20 + k under row k of tests/test_gpu_ensemble.py's PHYS: every row is the single handle's
    bits (with distinct nets a member or net index mix-up in the model-indexed launches changes them), and row 1 is held to the oracle per block"""
    from tests.test_gpu_ensemble import PHYS, _assert_rows_bit_identical, _ensemble
    c = D.wm_case("mish", n, "rk4", 1)
    p = c.p                                                          # (the plain configuration: the ensemble takes the constants as rows)
    W = np.stack([D.weights(p.cfg, 20 + k) for k in range(3)])
    assert np.array_equal(W[1], c.w)
    desc = _assert_rows_bit_identical(p, c.truth, W, PHYS[:3], ma, range(3))
    assert "models=3" in desc and "rich_tape=1" in desc, desc
    sol, res, loss8, desc2 = _ensemble(p, c.truth, W, PHYS[:3], ma)
    sol_b, res_b, loss8_b, _ = _ensemble(p, c.truth, W, PHYS[:3], ma)
    assert np.array_equal(sol, sol_b) and np.array_equal(res, res_b) and np.array_equal(loss8, loss8_b) and desc2 == desc
    P = p.cfg.n_params
    assert not np.array_equal(res[0], res[1]) and not np.array_equal(res[1], res[2])
    _check("ensemble/%d/%s/row1" % (n, ma), c, (sol[1], (loss8[1, 6], loss8[1, :6]), (res[1, P + 6], res[1, P:P + 6], res[1, :P])))


# ------------------------------------------------------------------------------------------------------------------ d. free convection with biases
@pytest.mark.parametrize("ma", MAS)
@pytest.mark.parametrize("Nz,ca", [(32, False), (64, False), (32, True)])
def test_fc32_with_biases(Nz, ca, ma):
    """fc32 (FreeConvectionNDE at 2 sub-steps; ConvectiveAdjustmentNDE at 20 under RK4), 19 columns: a ragged tile"""
    import colnde
    from colnde.nde import ENGINE_FC32
    c = D.fc_case(Nz, ca)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 19, engine=ENGINE_FC32, matrix_arithmetic=ma))
    assert plan["engine"] == ENGINE_FC32 and plan["dw_taped"] and plan["conv"] == 0 and plan["matrix_arithmetic"] == ma, plan
    assert plan["bf16x3_forward"] == plan["bf16x3_adjoint"] == (ma == "bf16x3_exact"), plan
    _check("fc32/%d/ca%d/%s" % (Nz, ca, ma), c, got, fc=True)


def test_tile16_free_convection_with_biases():
    import colnde
    from colnde.nde import ENGINE_TILE16
    c = D.fc_case(32, False)
    got, plan, _ = _run(c, lambda: colnde.ColumnNDE(c.cfg, 19, engine=ENGINE_TILE16))
    assert plan["engine"] == ENGINE_TILE16 and plan["dw_taped"], plan
    _check("tile16_fc/32", c, got, fc=True)


@pytest.mark.parametrize("ma", MAS)
def test_conv3_with_biases(ma):
    """the `--conv 3` network, its filter bias at the non-zero default, biased dense layers behind it"""
    import colnde
    from colnde.nde import ENGINE_FC32
    c = D.conv_case()
    got, plan, text = _run(c, lambda: colnde.ColumnNDE(c.cfg, 19, conv=c.conv, matrix_arithmetic=ma))
    assert plan["engine"] == ENGINE_FC32 and plan["conv"] == 3 and "conv=3" in text, (plan, text)
    assert plan["bf16x3_forward"] == plan["bf16x3_adjoint"] == (ma == "bf16x3_exact"), plan
    _check("conv3/32/%s" % ma, c, got, fc=True)
