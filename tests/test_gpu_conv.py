"""The free-convection driver's `--conv c` network (train_free_convection_nde.jl:110-122) on the fc32 kernels (colnde_create_conv): against the
float64 oracle run unchanged on the equivalent four-layer Toeplitz network (gradient folded onto the c + 1 filter entries), against tile16 running
that Toeplitz network (an independent kernel family), block by block, under both matrix arithmetics, RK4 and RKC2, time-segmented tapes,
bit-reproducible, through the device ADAM loop; and what a conv handle refuses."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde.flux_compat import ADAM
from colnde.free_convection import (FreeConvectionNDE, conv_grad_from_dense, conv_n_params, conv_to_dense, train_neural_differential_equation_device)
from colnde.nde import ENGINE_FC32, ENGINE_TILE16
from oracle import nde_oracle as O
from tests.conv_cases import CPU_CHECKED, FC_KW, blocks, dense_cfg, kw_items, oracle_loss_grad, reference
from tests.test_gpu_parity import _record, _rel, FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL

pytestmark = pytest.mark.gpu
SC = [0, 0, 1.0, 0, 0, 0]


def _conv_run(cfg, c, ncol, p, truth, arith):
    with colnde.ColumnNDE(cfg, ncol, conv=c, matrix_arithmetic=arith) as nde:
        assert nde.engine == ENGINE_FC32 and nde.n_params == conv_n_params(cfg.Nz, c)
        nde.set_problem(p.x0, p.bcs, truth)
        sol = nde.forward(p.weights)
        tot_l, _ = nde.loss(p.weights, SC)
        tot, _, grad = nde.loss_grad(p.weights, SC)
        tot2, _, grad2 = nde.loss_grad(p.weights, SC)
        plan, text = nde.plan(), nde.describe()
    assert tot2 == tot and np.array_equal(grad2, grad)                     # two calls: identical bits, total and gradient
    assert np.isclose(tot_l, tot, rtol=1e-5)
    split = arith == "bf16x3_exact"
    assert plan["conv"] == c and plan["bf16x3_forward"] == plan["bf16x3_adjoint"] == split
    assert "engine=fc32" in text and ("conv=%d" % c) in text and ("forward=%s" % ("bf16x3" if split else "f32")) in text
    return sol, tot, grad


def _toeplitz_run(cfg, c, ncol, p, truth):
    """tile16 on the four-layer Toeplitz network: what a user of the parent commit could run."""
    dc = dense_cfg(cfg, c)
    wd = conv_to_dense(p.weights, cfg.Nz, c).astype(np.float32)
    with colnde.ColumnNDE(dc, ncol, engine=ENGINE_TILE16) as nde:
        assert nde.engine == ENGINE_TILE16
        nde.set_problem(p.x0, p.bcs, truth)
        sol = nde.forward(wd)
        tot, _, g = nde.loss_grad(wd, SC)
    return sol, tot, conv_grad_from_dense(g.astype(np.float64), cfg.Nz, c)


def _check_against(label, Nz, c, got, ref, scale, floor=(0.0, 0.0, 0.0)):
    """sol within scale * FC_SOL_ATOL, loss within scale * FC_LOSS_RTOL, the whole gradient within scale * FC_GRAD_REL and every block on its own
    within twice that (+ the floors of a float32-vs-float64 yardstick, where one applies).  Figures are recorded and printed before the assertions."""
    (sol_g, tot_g, grad_g), (sol, tot, g) = got, ref
    errs = dict(sol_abs=np.abs(sol_g - sol).max(), loss_rel=abs(tot_g - tot) / abs(tot), grad_rel=_rel(grad_g, g))
    for name, a, b in blocks(Nz, c):
        errs["grad_rel_" + name] = _rel(grad_g[a:b], g[a:b])
    _record(label, **errs)
    print(label, {k: "%.3e" % v for k, v in errs.items()})
    assert errs["sol_abs"] < scale * FC_SOL_ATOL + floor[0]
    assert errs["loss_rel"] < scale * FC_LOSS_RTOL + floor[1]
    assert errs["grad_rel"] < scale * FC_GRAD_REL + floor[2]
    for name, a, b in blocks(Nz, c):
        assert errs["grad_rel_" + name] < 2 * (scale * FC_GRAD_REL + floor[2]), name
    return errs


@pytest.mark.parametrize("arith", ["bf16x3_exact", "f32_mfma"])
@pytest.mark.parametrize("Nz,c,ncol", [(32, 2, 1), (32, 3, 19), (32, 8, 33), (64, 2, 5), (64, 5, 17)])
def test_conv_free_convection_against_oracle_and_tile16_toeplitz(Nz, c, ncol, arith):
    """One lane group, a ragged tile, two tiles, the smallest and the largest filter."""
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(FC_KW))
    got = _conv_run(cfg, c, ncol, p, truth, arith)
    _check_against("conv/fc/%s/%d/%d/%d" % (arith, Nz, c, ncol), Nz, c, got, (sol, tot, g), 1.0)
    t16 = _toeplitz_run(cfg, c, ncol, p, truth)
    _check_against("conv/fc/%s/%d/%d/%d/vs_tile16_toeplitz" % (arith, Nz, c, ncol), Nz, c, got, t16, 0.25)
    _check_against("conv/fc/tile16_toeplitz_vs_oracle/%d/%d/%d" % (Nz, c, ncol), Nz, c, t16, (sol, tot, g), 1.0)


@pytest.mark.parametrize("arith", ["bf16x3_exact", "f32_mfma"])
@pytest.mark.parametrize("case,ncol", [("ca/32/c8", 19), ("ca/64/c2", 5)])
def test_conv_conv_adj_nde_rk4_against_oracle_and_tile16_toeplitz(case, ncol, arith):
    Nz, c, kw = CPU_CHECKED[case]
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(kw))
    got = _conv_run(cfg, c, ncol, p, truth, arith)
    _check_against("conv/ca_rk4/%s/%s/%d" % (arith, case, ncol), Nz, c, got, (sol, tot, g), 1.0)
    t16 = _toeplitz_run(cfg, c, ncol, p, truth)
    _check_against("conv/ca_rk4/%s/%s/%d/vs_tile16_toeplitz" % (arith, case, ncol), Nz, c, got, t16, 0.25)


@pytest.mark.parametrize("arith", ["bf16x3_exact", "f32_mfma"])
@pytest.mark.parametrize("case,ncol", [("ca/32/c8", 19), ("ca/64/c2", 5)])
def test_conv_conv_adj_nde_rkc2_against_oracle_and_tile16_toeplitz(case, ncol, arith):
    """RKC2, two steps per save interval, automatic stage count: held to the oracle's RKC2 (same recurrence, same one-switch-pattern pullback) the
    way the plain fc32 network is (tests/test_gpu_fc.py): five times the float32 oracle's own distance from float64, plus the fc32 floors."""
    Nz, c, kw = CPU_CHECKED[case]
    kw = dict(kw, substeps=2)
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(kw), stepper="rkc2")
    assert colnde.rkc_stages(cfg) >= 4
    tot32, g32, sol32 = oracle_loss_grad(cfg, c, p.x0, p.bcs, p.weights, truth, dtype=np.float32)
    e32 = (np.abs(sol32 - sol).max(), abs(tot32 - tot) / abs(tot), _rel(g32, g))
    got = _conv_run(cfg, c, ncol, p, truth, arith)
    t16 = _toeplitz_run(cfg, c, ncol, p, truth)
    _record("conv/ca_rkc2/%s/%s/oracle32_vs_64" % (arith, case), sol_abs=e32[0], loss_rel=e32[1], grad_rel=e32[2])
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    _check_against("conv/ca_rkc2/%s/%s/%d" % (arith, case, ncol), Nz, c, got, (sol, tot, g), 1.0, floor=(5 * e32[0] + FC_SOL_ATOL, 5 * e32[1], 5 * e32[2]))
    _check_against("conv/ca_rkc2/%s/%s/%d/vs_tile16_toeplitz" % (arith, case, ncol), Nz, c, got, t16, 0.25, floor=(5 * e32[0], 5 * e32[1], 5 * e32[2]))


@pytest.mark.parametrize("model,seg", [("fc", 2), ("fc", 3), ("ca_rkc2", 2)])
def test_conv_time_segmented_tapes(model, seg, monkeypatch):
    """COLNDE_FC_SEG forces at least two time segments of the tapes (the conv tape among them): the gradient keeps its bounds, the loss equals the
    unsegmented run's to 1e-5, and two segmented calls give the same bits."""
    Nz, c, ncol = 32, 3, 19
    kw = dict(FC_KW, n_save=6) if model == "fc" else dict(CPU_CHECKED["ca/32/c8"][2], n_save=6, substeps=2)
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(kw), stepper="rkc2" if model == "ca_rkc2" else "rk4")
    one = _conv_run(cfg, c, ncol, p, truth, "bf16x3_exact")
    monkeypatch.setenv("COLNDE_FC_SEG", str(seg))
    with colnde.ColumnNDE(cfg, ncol, conv=c) as nde:
        nde.set_problem(p.x0, p.bcs, truth)
        cut = nde.loss_grad(p.weights, SC)
        again = nde.loss_grad(p.weights, SC)
        plan = nde.plan()
    assert plan["time_segments"] == -(-5 // seg) >= 2 and plan["n_blocks"] == 1
    assert again[0] == cut[0] and np.array_equal(again[2], cut[2])
    _record("conv/segments/%s/%d" % (model, seg), loss_rel_vs_single=abs(cut[0] - one[1]) / abs(one[1]), grad_rel_vs_single=_rel(cut[2], one[2].astype(np.float64)))
    assert np.isclose(cut[0], one[1], rtol=1e-5)
    floor = (0.0, 0.0, 0.0)
    if model == "ca_rkc2":
        tot32, g32, sol32 = oracle_loss_grad(cfg, c, p.x0, p.bcs, p.weights, truth, dtype=np.float32)
        floor = (5 * np.abs(sol32 - sol).max() + FC_SOL_ATOL, 5 * abs(tot32 - tot) / abs(tot), 5 * _rel(g32, g))
    _check_against("conv/segments/%s/%d/vs_oracle" % (model, seg), Nz, c, (one[0], cut[0], cut[2]), (sol, tot, g), 1.0, floor=floor)


def test_conv_device_adam_follows_the_folded_oracle_gradient():
    """Five steps of train_neural_differential_equation_device with ADAM(1e-3) against a float64 loop on the folded oracle gradient: every step's
    loss within FC_LOSS_RTOL."""
    Nz, c, ncol = 32, 3, 19
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(FC_KW))
    nde = FreeConvectionNDE(cfg, p.x0, p.bcs, truth, conv=c)
    try:
        theta_g, hist = train_neural_differential_equation_device(nde, p.weights.copy(), ADAM(1e-3), 5)
        assert np.transpose(nde.solve_nde(theta_g), (0, 2, 1)).shape == truth.shape
        assert np.isclose(nde.nde_loss(theta_g), nde.nde_loss_and_grad(theta_g)[0], rtol=1e-5)
    finally:
        nde.close()
    theta, opt, ref_hist = p.weights.astype(np.float64), ADAM(1e-3), []
    for _ in range(5):
        t, gr, _ = oracle_loss_grad(cfg, c, p.x0, p.bcs, theta, truth)
        ref_hist.append(t)
        opt.update(theta, gr)
    print("device", hist, "oracle", ref_hist)
    _record("conv/adam5", **{"loss_rel_step%d" % i: abs(a - b) / abs(b) for i, (a, b) in enumerate(zip(hist, ref_hist))})
    assert len(hist) == 5 and theta_g.shape == (conv_n_params(Nz, c),)
    for a, b in zip(hist, ref_hist):
        assert np.isclose(a, b, rtol=FC_LOSS_RTOL), (hist, ref_hist)
    assert ref_hist[-1] < ref_hist[0]


def test_conv_handle_refuses_other_calls_by_name_and_leaves_plain_handles_alone():
    Nz, c, ncol = 32, 3, 19
    p, cfg, truth, tot, g, sol = reference(Nz, c, ncol, kw_items(FC_KW))
    plain = synthetic.free_convection_problem(ncol, Nz=Nz, **FC_KW)
    L = _lib.lib()
    with colnde.ColumnNDE(plain.cfg, ncol) as first:
        first.set_problem(plain.x0, plain.bcs, truth)
        with colnde.ColumnNDE(cfg, ncol, conv=c) as nde:
            nde.set_problem(p.x0, p.bcs, truth)
            assert L.colnde_conv_filter(nde._h) == c and L.colnde_conv_filter(first._h) == 0
            assert first.plan()["conv"] == 0 and "conv=" not in first.describe()
            w = p.weights
            T = p.x0[:4]
            top = np.zeros(4, np.float32)
            refused = {
                "colnde_rhs": lambda: nde.rhs(T, w, p.bcs[:4], 0.0),
                "colnde_flux": lambda: nde.flux(T, w, p.bcs[:4]),
                "colnde_error_estimate": lambda: nde.error_estimate(w),
                "colnde_choose_substeps": lambda: nde.choose_substeps(w, 1e-3),
                "colnde_infer_forcing": lambda: nde.infer_forcing(w, T, top, 100.0),
                "colnde_infer_dz_wT": lambda: nde.infer_dz_wT(w, T, top, 100.0),
                "colnde_fc_embedded_step": lambda: nde.fc_embedded_step(w, T, top, 100.0, 1.0, 10.0, None),
                "colnde_fc_diagnose_wT": lambda: nde.fc_diagnose_wT(w, T, top, 100.0, 10.0, None),
                "colnde_set_global_columns": lambda: nde.set_global_columns(64),
            }
            for name, call in refused.items():
                with pytest.raises(colnde.ColndeError, match=name):
                    call()
            # ... and straight through the C ABI: pre-training, the communicator result, the ensemble and closure families
            z = ctypes.c_void_p()
            f = ctypes.c_float()
            bt = (ctypes.c_double * 2)(0.9, 0.999)
            for name, call in (
                    ("colnde_pretrain_flux_dev", lambda: L.colnde_pretrain_flux_dev(nde._h, 2, z, z, z, z, z, z, z, 1, 1.0, 1e-3, 0.9, 0.999, 1e-8, bt, 0, ctypes.byref(f))),
                    ("colnde_allreduce_result_dev", lambda: L.colnde_allreduce_result_dev(nde._h, z, z)),
                    ("colnde_ensemble_", lambda: L.colnde_ensemble_forward_dev(nde._h, z, z)),
                    ("colnde_closure_", lambda: L.colnde_closure_forward_dev(nde._h, z, z))):
                rc = call()                                              # (the message is the last call's: read it before the next one)
                msg = L.colnde_last_error().decode()
                assert rc != 0 and name in msg and "conv" in msg, (name, msg)
            # the calls of the list still work after the refusals
            nde.set_substeps(2)
            assert nde.substeps == 2
            tot_c, _, grad_c = nde.loss_grad(p.weights, SC)
            assert np.isclose(tot_c, tot, rtol=FC_LOSS_RTOL)
            assert nde.loss_per_tstep(p.weights).shape == (ncol, 6, cfg.n_save)
            # a plain fc32 handle created next to the conv handle gives the bits a second plain handle gives
            sol_1 = first.forward(plain.weights)
            res_1 = first.loss_grad(plain.weights, SC)
    with colnde.ColumnNDE(plain.cfg, ncol) as second:
        second.set_problem(plain.x0, plain.bcs, truth)
        sol_2 = second.forward(plain.weights)
        res_2 = second.loss_grad(plain.weights, SC)
    assert np.array_equal(sol_1, sol_2) and res_1[0] == res_2[0] and np.array_equal(res_1[2], res_2[2])
