"""Records tests/golden/dw_bits.json: SHA-256 digests of what loss_grad returns on the cases of tests/test_gpu_dw_bits.py — one per way through
the taped weight-gradient GEMM (csrc/engine_dwgemm.hip) and its plan (csrc/dw_plan.h) — from the build that is in the tree when this runs (one MI355X).

    python tests/golden/make_dw_bits.py    # rewrites tests/golden/dw_bits.json

Each case is the smallest configuration of the existing test that covers its path:
  tile16/*    tests/test_gpu_parity.py::test_tile16_taped_weight_gradients[wind_mixing]: 21 columns = a full 16-column tile and a ragged one, 5 frames;
              the LDS-staged f32 kernel, the L2-streaming one (COLNDE_T16_DWLDS=0) and the bf16 split kernel
  fc32/*      tests/test_gpu_fc.py::test_fc32_against_oracle_and_tile16[32-19-32]: Nz = 32, 19 columns in one 32-column tile, both arithmetics
  wide/*      tests/test_gpu_wide_nets.py's 3 x (96-400-400-31) at 16 columns and one save interval: 325 KB records do not fit the LDS, so the 400 x 400
              matrices are cut into chunks of output blocks (split kernel) or stream from L2 (f32 kernel)
  ensemble/*  tests/test_gpu_ensemble.py's K-model handle at K = 2 and 8 columns, 5 frames, both arithmetics

Run it on the PARENT of a change that must not move the bits, commit the file with the change, and the test holds the change to it.
Run it again only with a change that is meant to alter the arithmetic (and say so in that commit)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import colnde                                                # noqa: E402
from colnde import synthetic                                 # noqa: E402
from colnde.nde import ENGINE_FC32, ENGINE_TILE16            # noqa: E402

ARITHMETICS = ("bf16x3_exact", "f32_mfma")
WM_SCALINGS = (1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3)
FC_SCALINGS = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0)                 # free convection: the T term alone (oracle.default_loss_scalings)
WIDE = dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
# (nu0, nu_minus, dRi, Ric, Pr) of the two models: tests/test_gpu_ensemble.py's first two constant sets
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2]], np.float32)
PATH = os.path.join(HERE, "dw_bits.json")
# key -> (kind, matrix arithmetic, environment of the handle's whole life)
CASES = {
    "tile16/lds": ("tile16", "f32_mfma", {"COLNDE_T16_DWTAPE": "1"}),
    "tile16/l2stream": ("tile16", "f32_mfma", {"COLNDE_T16_DWTAPE": "1", "COLNDE_T16_DWLDS": "0"}),
    "tile16/split": ("tile16", "bf16x3_exact", {"COLNDE_T16_DWTAPE": "1"}),
    "fc32/bf16x3_exact": ("fc32", "bf16x3_exact", {"COLNDE_FC_CW": "32"}),
    "fc32/f32_mfma": ("fc32", "f32_mfma", {"COLNDE_FC_CW": "32"}),
    "wide/bf16x3_exact": ("wide", "bf16x3_exact", {}),
    "wide/f32_mfma": ("wide", "f32_mfma", {}),
    "ensemble/bf16x3_exact": ("ensemble", "bf16x3_exact", {}),
    "ensemble/f32_mfma": ("ensemble", "f32_mfma", {}),
}
SWITCHES = ("COLNDE_T16_DWTAPE", "COLNDE_T16_DWLDS", "COLNDE_FC_CW", "COLNDE_DW_SPLIT", "COLNDE_T16_BLOCK", "COLNDE_FC_BLOCK", "COLNDE_FC_SEG",
            "COLNDE_T16_SPLIT_RICH")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def _single(p, engine, ma, scalings, calls):
    with colnde.ColumnNDE(p.cfg, p.n_columns, engine=engine, matrix_arithmetic=ma) as nde:
        assert nde.engine == engine and nde.matrix_arithmetic == ma
        nde.set_problem(p.x0, p.bcs)
        truth = nde.forward(p.weights_truth)
        nde.set_problem(p.x0, p.bcs, truth)
        sol = nde.forward(p.weights)
        res = []
        for _ in range(calls):
            tot, terms, g = nde.loss_grad(p.weights, scalings)
            res.append(np.concatenate([g, terms, [tot]]).astype(np.float32))
        plan = nde.plan()
    assert plan["dw_taped"] and plan["dw_slices"] >= 1 and plan["n_blocks"] == 1 and plan["bf16x3_dw"] == (ma == "bf16x3_exact"), plan
    return sol, res


def _ensemble(p, ma, calls):
    with colnde.ColumnNDE(p.cfg, p.n_columns, matrix_arithmetic=ma) as nde:
        nde.set_problem(p.x0, p.bcs)
        truth = nde.forward(p.weights_truth)
    W = np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 1e2) for k in range(2)]).astype(np.float32)
    with colnde.ColumnNDEEnsemble(p.cfg, p.n_columns, 2, physics=PHYS, matrix_arithmetic=ma) as e:
        e.set_problem(p.x0, p.bcs, truth)
        sol = e.forward(W)
        res = [np.array(e.loss_grad(W, WM_SCALINGS), np.float32) for _ in range(calls)]
    assert res[0].shape == (2, p.cfg.n_params + 8)
    return sol, res


def run(name, calls=1):
    """(sol, [result of each of `calls` loss_grad calls on one handle]).  A single handle's result is [gradient; terms(6); total], an ensemble's
    the K rows [gradient; terms(6); total; 0].  The switches are read when the handle plans its tapes and when it launches, so they are set
    around the handle's whole life and put back."""
    kind, ma, env = CASES[name]
    before = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        if kind == "tile16":
            return _single(synthetic.wind_mixing_problem(21, n_frames=5, weight_divisor=1e2), ENGINE_TILE16, ma, WM_SCALINGS, calls)
        if kind == "fc32":
            return _single(synthetic.free_convection_problem(19, Nz=32, n_save=5, substeps=2, t_end=0.01), ENGINE_FC32, ma, FC_SCALINGS, calls)
        if kind == "wide":
            return _single(synthetic.wind_mixing_problem(16, n_frames=2, weight_divisor=1e2, **WIDE), ENGINE_TILE16, ma, WM_SCALINGS, calls)
        return _ensemble(synthetic.wind_mixing_problem(8, n_frames=5, weight_divisor=1e2), ma, calls)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record(sol, res):
    n = res.shape[-1] - (7 if res.ndim == 1 else 8)
    return {"sol_sha256": sha(sol), "result_sha256": sha(res), "loss_total": float(res[..., n + 6].sum()),
            "gradient_norm": float(np.linalg.norm(res[..., :n].astype(np.float64)))}


if __name__ == "__main__":
    fixture = {}
    for name in CASES:
        sol, (res,) = run(name)
        assert np.isfinite(sol).all() and np.isfinite(res).all(), name
        fixture[name] = record(sol, res)
    with open(PATH, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(fixture, indent=1, sort_keys=True))
