"""ms per loss_grad, and per kernel, of the `--conv 3` free-convection network on the two 8-simulation shapes of bench.py --full (32 and 64 levels,
129 save points x 4 RK4 sub-steps), in the manner of tools/fc_small.py:
  (a) the conv handle (colnde_create_conv: the filter inside the fc32 16-column kernels)
  (b) the plain fc32 handle of the same build (the three-Dense network)
  (c) tile16 on the four-layer Toeplitz network (free_convection.conv_to_dense): what a `--conv` user could run before the conv handle
Each timing is the mean of `--reps` iterations after a warm-up, repeated `--rounds` times; the spread is (max - min) over the rounds.
    python tools/fc_conv_rate.py [--out profiles/fc_conv_rate.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import colnde
from colnde import synthetic
from colnde.free_convection import conv_dense_layer_sizes, conv_to_dense
from colnde.nde import ENGINE_TILE16

SC = [0, 0, 1, 0, 0, 0]
KERNELS = ("forward", "adjoint", "dw1", "reduce")


def measure(make, x0, bcs, w, w_truth, reps, rounds):
    with make() as nde:
        nde.set_problem(x0, bcs)
        truth = nde.forward(w_truth)
        nde.set_problem(x0, bcs, truth)
        nde.loss_grad(w, SC)                                   # plans the tapes
        nde.loss_grad(w, SC)
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            for _ in range(reps):
                nde.loss_grad(w, SC)
            ms.append((time.perf_counter() - t0) / reps * 1e3)
        nde.set_profiling(True)
        nde.reset_kernel_times()
        for _ in range(reps):
            nde.loss_grad(w, SC)
        kt = {k: round(nde.kernel_time(k)[0] / reps, 3) for k in KERNELS}
        return dict(ms=round(float(np.mean(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), spread_ms=round(max(ms) - min(ms), 3),
                    kernel_ms_per_iteration=kt, describe=nde.describe().split(" | env")[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conv", type=int, default=3)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for Nz in (32, 64):
        c, n = a.conv, a.columns
        pc = synthetic.free_convection_conv_problem(n, c, Nz=Nz)
        pp = synthetic.free_convection_problem(n, Nz=Nz)
        dcfg = pc.cfg.with_(layer_sizes=conv_dense_layer_sizes(Nz, c), activations=("relu", "relu", "relu", "identity"))
        wd, wdt = (conv_to_dense(t, Nz, c).astype(np.float32) for t in (pc.weights, pc.weights_truth))
        res = {
            "conv_handle": measure(lambda: colnde.ColumnNDE(pc.cfg, n, conv=c), pc.x0, pc.bcs, pc.weights, pc.weights_truth, a.reps, a.rounds),
            "plain_fc32": measure(lambda: colnde.ColumnNDE(pp.cfg, n), pp.x0, pp.bcs, pp.weights, pp.weights_truth, a.reps, a.rounds),
            "tile16_toeplitz": measure(lambda: colnde.ColumnNDE(dcfg, n, engine=ENGINE_TILE16), pc.x0, pc.bcs, wd, wdt, a.reps, a.rounds),
        }
        row = dict(Nz=Nz, conv=c, columns=n, n_save=pc.cfg.n_save, substeps=pc.cfg.substeps, reps=a.reps, rounds=a.rounds, **res)
        row["conv_over_plain"] = round(res["conv_handle"]["ms"] / res["plain_fc32"]["ms"], 3)
        row["toeplitz_over_conv"] = round(res["tile16_toeplitz"]["ms"] / res["conv_handle"]["ms"], 3)
        row["gap_ms_toeplitz_minus_conv"] = round(res["tile16_toeplitz"]["ms_min"] - res["conv_handle"]["ms_max"], 3)
        row["largest_spread_ms"] = max(r["spread_ms"] for r in res.values())
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
