"""Records tests/golden/tape_plans.json: what the tape planners of the gradient paths (csrc/tape_plan.h, csrc/api_grad.hip, csrc/api_ensemble.hip) decide and
what the gradient then computes, on the cases of tests/test_gpu_tape_plans.py, from the build that is in the tree when this runs (one MI355X).

    python tests/golden/make_tape_plans.py    # rewrites tests/golden/tape_plans.json

tests/golden/dw_bits.json covers one-block plans only.  These cases are the plans with more than one column block or time segment and the optional tapes,
each on the smallest shape that reaches its path (the wind-mixing and fc32 problems are make_dw_bits.py's; 5 frames / save points unless said):
  tile16/*     ENGINE_TILE16, 21 columns (a full 16-column tile and a ragged one), COLNDE_T16_DWTAPE=1: the default plan, two blocks (COLNDE_T16_BLOCK=16, the
               second ragged), no pre-activation tape (COLNDE_T16_ZTAPE=0), and the in-register path (COLNDE_T16_DWTAPE=0)
  netsplit/*   engine AUTO, 21 columns: the rich tape (default), the plain pre-activation tape (COLNDE_T16_SPLIT_RICH=0), two blocks
  wide/ztape   3 x (96-400-400-31) at 16 columns, one save interval: activation rows in global memory, the Z tape required
  regtile/*    ENGINE_REGTILE, 40 columns: default, two blocks (COLNDE_RT_BLOCK=32), no Z1 tape (COLNDE_RT_ZTAPE=0)
  fc32/*       ENGINE_FC32, Nz = 32, substeps = 2: 19 columns whole, in four segments (COLNDE_FC_SEG=1) and in two, the last short (COLNDE_FC_SEG=3);
               40 columns in two blocks of the 32-column kernels (COLNDE_FC_CW=32 COLNDE_FC_BLOCK=32), alone and with COLNDE_FC_SEG=2;
               ConvectiveAdjustmentNDE (the switch tape; an inverted layer in two columns so that it is live; 20 sub-steps: its RK4 stability bound) in two segments
  conv/*       colnde_create_conv, c = 3 at 19 columns (tests/conv_cases.py's fc/32/c3 at 5 save points): whole and in two segments
  ens_wm/*     colnde_create_ensemble, K = 2 at 8 columns: rich tape, plain tape, and a step schedule set after creation (the re-plan path: the
               per-interval stability minimum, plus one step on the first interval)
  ens_fc/*     colnde_create_fc_ensemble, K = 2 at 8 columns: whole and in two segments
  ens_conv/seg2  colnde_create_conv_ensemble, K = 2, c = 3 at 8 columns, two segments
Recorded per case: the eight integers of colnde_plan after the first loss_grad, the colnde_describe string, SHA-256 of sol and of loss_grad's result.
Every case could be created on the parent of the change that added this file: none was dropped.

Run it on the PARENT of a change that must not move a plan or the bits, commit the file with the change, and the test holds the change to it."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import colnde                                                          # noqa: E402
from colnde import _lib, synthetic                                     # noqa: E402
from colnde.nde import ENGINE_AUTO, ENGINE_FC32, ENGINE_REGTILE, ENGINE_TILE16      # noqa: E402

WM_SCALINGS = (1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3)
FC_SCALINGS = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
WIDE = dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2]], np.float32)      # make_dw_bits.py's two models
CONV_KW = dict(weight_divisor=10.0, t_end=1.0, n_save=5, substeps=2)                        # tests/conv_cases.py's fc/32/c3 at 5 save points
PATH = os.path.join(HERE, "tape_plans.json")
# key -> (kind, columns, environment of the handle's whole life).  The part of the key before the slash is the engine group: one problem, one arithmetic.
CASES = {
    "tile16/default": ("tile16", 21, {"COLNDE_T16_DWTAPE": "1"}),
    "tile16/block16": ("tile16", 21, {"COLNDE_T16_DWTAPE": "1", "COLNDE_T16_BLOCK": "16"}),
    "tile16/ztape0": ("tile16", 21, {"COLNDE_T16_DWTAPE": "1", "COLNDE_T16_ZTAPE": "0"}),
    "tile16/inreg": ("tile16", 21, {"COLNDE_T16_DWTAPE": "0"}),
    "netsplit/rich": ("netsplit", 21, {}),
    "netsplit/plain": ("netsplit", 21, {"COLNDE_T16_SPLIT_RICH": "0"}),
    "netsplit/block16": ("netsplit", 21, {"COLNDE_T16_BLOCK": "16"}),
    "wide/ztape": ("wide", 16, {}),
    "regtile/default": ("regtile", 40, {}),
    "regtile/block32": ("regtile", 40, {"COLNDE_RT_BLOCK": "32"}),
    "regtile/ztape0": ("regtile", 40, {"COLNDE_RT_ZTAPE": "0"}),
    "fc32/whole": ("fc32", 19, {}),
    "fc32/seg1": ("fc32", 19, {"COLNDE_FC_SEG": "1"}),
    "fc32/seg3": ("fc32", 19, {"COLNDE_FC_SEG": "3"}),
    "fc32/block32": ("fc32", 40, {"COLNDE_FC_CW": "32", "COLNDE_FC_BLOCK": "32"}),
    "fc32/block32_seg2": ("fc32", 40, {"COLNDE_FC_CW": "32", "COLNDE_FC_BLOCK": "32", "COLNDE_FC_SEG": "2"}),
    "fc32/convadj_seg2": ("fc32_ca", 19, {"COLNDE_FC_SEG": "2"}),
    "conv/whole": ("conv", 19, {}),
    "conv/seg2": ("conv", 19, {"COLNDE_FC_SEG": "2"}),
    "ens_wm/rich": ("ens_wm", 8, {}),
    "ens_wm/plain": ("ens_wm", 8, {"COLNDE_T16_SPLIT_RICH": "0"}),
    "ens_wm/schedule": ("ens_wm_sched", 8, {}),
    "ens_fc/whole": ("ens_fc", 8, {}),
    "ens_fc/seg2": ("ens_fc", 8, {"COLNDE_FC_SEG": "2"}),
    "ens_conv/seg2": ("ens_conv", 8, {"COLNDE_FC_SEG": "2"}),
}
# groups whose cases share problem and arithmetic and differ in the plan alone: blocks and segments reorder the gradient's sums
PLAN_GROUPS = {"tile16": ["tile16/default", "tile16/block16", "tile16/ztape0", "tile16/inreg"],
               "netsplit": ["netsplit/rich", "netsplit/plain", "netsplit/block16"],
               "regtile": ["regtile/default", "regtile/block32", "regtile/ztape0"],
               "fc32/19": ["fc32/whole", "fc32/seg1", "fc32/seg3"],
               "fc32/40": ["fc32/block32", "fc32/block32_seg2"],
               "conv": ["conv/whole", "conv/seg2"],
               "ens_wm": ["ens_wm/rich", "ens_wm/plain"],
               "ens_fc": ["ens_fc/whole", "ens_fc/seg2"]}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def _plan_and_describe(nde):
    info = (ctypes.c_int * 8)()
    _lib.check(nde._L.colnde_plan(nde._h, info))
    return [int(v) for v in info], nde.describe()


def _single(p, n, engine, scalings, calls, conv=0):
    with colnde.ColumnNDE(p.cfg, n, engine=engine, conv=conv) as nde:
        assert engine == ENGINE_AUTO or nde.engine == engine
        nde.set_problem(p.x0, p.bcs)
        truth = nde.forward(p.weights_truth)
        nde.set_problem(p.x0, p.bcs, truth)
        sol = nde.forward(p.weights)
        res = []
        for _ in range(calls):
            tot, terms, g = nde.loss_grad(p.weights, scalings)
            res.append(np.concatenate([g, terms, [tot]]).astype(np.float32))
        plan, desc = _plan_and_describe(nde)
    return sol, res, plan, desc


def _ensemble(make, p, W, scalings, calls, conv=0, schedule=False):
    with colnde.ColumnNDE(p.cfg, p.x0.shape[0], conv=conv) as nde:
        nde.set_problem(p.x0, p.bcs)
        truth = nde.forward(p.weights_truth)
    with make() as e:
        if schedule:                                          # after creation: the tapes sized there are planned again (ens_replan_tapes)
            counts = list(colnde.nde.schedule_min(p.cfg))
            counts[0] += 1
            e.set_schedule(counts)
            assert e.schedule() == tuple(counts)
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        res = [np.array(e.loss_grad(W, scalings), np.float32) for _ in range(calls)]
        plan, desc = _plan_and_describe(e)
    assert res[0].shape == (2, e.n_params + 8)
    return sol, res, plan, desc


def _fc_problem(n, ca=False):
    if not ca:
        return synthetic.free_convection_problem(n, Nz=32, n_save=5, substeps=2, t_end=0.01)
    p = synthetic.free_convection_problem(n, Nz=32, n_save=5, substeps=20, convective_adjustment=True, t_end=0.01)
    x0 = p.x0.copy()
    x0[:2, 16:22] = x0[:2, 16:22][:, ::-1]                    # an inverted layer in two columns: the adjustment switches (tests/test_gpu_fc_ensemble.py)
    return synthetic.ColumnProblem(p.cfg, x0, p.bcs, p.weights, p.weights_truth)


def _run(kind, n, calls):
    if kind in ("tile16", "netsplit", "regtile"):
        engine = {"tile16": ENGINE_TILE16, "netsplit": ENGINE_AUTO, "regtile": ENGINE_REGTILE}[kind]
        return _single(synthetic.wind_mixing_problem(n, n_frames=5, weight_divisor=1e2), n, engine, WM_SCALINGS, calls)
    if kind == "wide":
        return _single(synthetic.wind_mixing_problem(n, n_frames=2, weight_divisor=1e2, **WIDE), n, ENGINE_TILE16, WM_SCALINGS, calls)
    if kind in ("fc32", "fc32_ca"):
        return _single(_fc_problem(n, ca=kind == "fc32_ca"), n, ENGINE_FC32, FC_SCALINGS, calls)
    if kind == "conv":
        return _single(synthetic.free_convection_conv_problem(n, 3, Nz=32, **CONV_KW), n, ENGINE_AUTO, FC_SCALINGS, calls, conv=3)
    if kind in ("ens_wm", "ens_wm_sched"):
        p = synthetic.wind_mixing_problem(n, n_frames=5, weight_divisor=1e2)
        W = np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 1e2) for k in range(2)]).astype(np.float32)
        return _ensemble(lambda: colnde.ColumnNDEEnsemble(p.cfg, n, 2, physics=PHYS), p, W, WM_SCALINGS, calls, schedule=kind == "ens_wm_sched")
    if kind == "ens_fc":
        p = _fc_problem(n)
        W = np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 1e2) for k in range(2)]).astype(np.float32)
        return _ensemble(lambda: colnde.FreeConvectionEnsemble(p.cfg, n, 2), p, W, FC_SCALINGS, calls)
    assert kind == "ens_conv", kind
    p = synthetic.free_convection_conv_problem(n, 3, Nz=32, **CONV_KW)
    W = np.stack([p.weights, p.weights * (1.0 + 0.05 * synthetic._rng(21, 1).standard_normal(p.weights.shape))]).astype(np.float32)
    return _ensemble(lambda: colnde.FreeConvectionEnsemble(p.cfg, n, 2, conv=3), p, W, FC_SCALINGS, calls, conv=3)


def run(name, calls=1):
    """(sol, [result of each of `calls` loss_grad calls on one handle], the eight integers of colnde_plan, colnde_describe's string).  A single
    handle's result is [gradient; terms(6); total], an ensemble's the K rows [gradient; terms(6); total; 0].  The switches are read when the handle
    plans its tapes and when it launches, and colnde_describe lists every one that is set: all COLNDE_* variables but the library's path are taken
    out of the environment for the handle's whole life, the case's own set, and everything is put back."""
    kind, n, env = CASES[name]
    before = {k: v for k, v in os.environ.items() if k.startswith("COLNDE_") and k != "COLNDE_LIB"}
    for k in before:
        del os.environ[k]
    os.environ.update(env)
    try:
        return _run(kind, n, calls)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(before)


def record(sol, res, plan, desc):
    return {"plan": plan, "describe": desc, "sol_sha256": sha(sol), "result_sha256": sha(res)}


if __name__ == "__main__":
    fixture = {}
    for name in CASES:
        sol, (res,), plan, desc = run(name)
        assert np.isfinite(sol).all() and np.isfinite(res).all(), name
        fixture[name] = record(sol, res, plan, desc)
        print(name, json.dumps(fixture[name]), flush=True)
    with open(PATH, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
