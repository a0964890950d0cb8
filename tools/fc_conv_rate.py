"""ms per loss_grad, and per kernel, of the `--conv 3` free-convection network on the two 8-simulation shapes of bench.py --full (32 and 64 levels,
129 save points x 4 RK4 sub-steps), in the manner of tools/fc_small.py:
  (a) the conv handle (colnde_create_conv: the filter inside the fc32 16-column kernels)
  (b) the plain fc32 handle of the same build (the three-Dense network)
  (c) tile16 on the four-layer Toeplitz network (free_convection.conv_to_dense): what a `--conv` user could run before the conv handle
Each timing is the mean of `--reps` iterations after a warm-up, repeated `--rounds` times; the spread is (max - min) over the rounds.
    python tools/fc_conv_rate.py [--out profiles/fc_conv_rate.jsonl]

--ensemble: the K sweep of the conv ENSEMBLE (colnde_create_conv_ensemble) on the reference's training shape — 9 simulations, Nz = 32 and 64, c = 3,
FreeConvectionNDE (RK4) and ConvectiveAdjustmentNDE under RKC2, 129 save points x 4 sub-steps: ms per training iteration (loss_grad + ADAM on device
tensors) of K networks in one handle, K = 1, 4, 16, 64, against what a user has without it — a single conv handle run K times one after another, each
with its own weights and ADAM state (the single handle's kernels are the parent commit's, instruction for instruction: tools/asm_same.py).  Both sides
are warmed up and timed in the same process, ensemble and baseline in turn per K, ending in a device synchronise; the per-kernel slots come from a
separate profiled pass.
    python tools/fc_conv_rate.py --ensemble [--out profiles/fc_conv_ens_rate.json]"""
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


ENS_KERNELS = ("forward", "adjoint", "dw1", "reduce", "adam")          # dw1: the dW GEMM and the filter-gradient kernel; reduce: reduction and fold


def ensemble_sweep(a):
    import torch
    dev = torch.device("cuda", 0)
    c, n = a.conv, 9
    rows = []

    def timed(step, warmup, iters):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters

    for model in ("fc_rk4", "ca_rkc2"):
        for Nz in (32, 64):
            pc = synthetic.free_convection_conv_problem(n, c, Nz=Nz, convective_adjustment=model == "ca_rkc2")
            cfg = pc.cfg.with_(stepper="rkc2") if model == "ca_rkc2" else pc.cfg
            P = c + 1 + cfg.n_params - 4 * Nz * (c - 1)
            try:
                single = colnde.ColumnNDE(cfg, n, conv=c)
            except colnde.ColndeError as err:
                rows.append(dict(model=model, Nz=Nz, conv=c, columns=n, refused=str(err)))
                print(json.dumps(rows[-1]), flush=True)
                continue
            with single:
                single.set_problem(pc.x0, pc.bcs)
                truth = single.forward(pc.weights_truth)
                x0, bcs, tr = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (pc.x0, pc.bcs, truth))
                single.set_problem(x0, bcs, tr)
                rng = np.random.default_rng(1)
                Wall = (pc.weights[None, :] * (1 + 0.05 * rng.standard_normal((64, P)))).astype(np.float32)
                for K in (1, 4, 16, 64):
                    iters, warmup = (a.reps, 2) if K < 16 else (max(2, a.reps // 2), 1)
                    W = torch.from_numpy(Wall[:K].copy()).to(dev)
                    out = torch.empty((K, P + 8), device=dev)
                    m, v = torch.zeros((K, P), device=dev), torch.zeros((K, P), device=dev)
                    etas = torch.full((K,), 1e-4, device=dev)
                    row = dict(model=model, Nz=Nz, conv=c, columns=n, n_save=cfg.n_save, substeps=cfg.substeps, K=K, iterations=iters, warmup=warmup)
                    try:
                        ens = colnde.FreeConvectionEnsemble(cfg, n, K, conv=c)
                    except colnde.ColndeError as err:
                        row["refused"] = str(err)
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        continue
                    with ens:
                        ens.set_problem(x0, bcs, tr)

                        def ens_step():
                            ens.loss_grad(W, SC, out=out)
                            ens.adam_step(W, out, m, v, etas, beta_t=(0.9, 0.999))

                        # the baseline: the single handle K times in turn, member k on its own weights and moments
                        Wb, mb, vb = W.clone(), torch.zeros((K, P), device=dev), torch.zeros((K, P), device=dev)

                        def base_step():
                            for k in range(K):
                                single.loss_grad(Wb[k], SC, out=out[k])
                                single.adam_step(Wb[k], out[k], mb[k], vb[k], 1e-4, beta_t=(0.9, 0.999))

                        ms_e, ms_b = [], []
                        for _ in range(a.rounds):                              # in turn: the machine's drift falls on both
                            ms_e.append(timed(ens_step, warmup, iters))
                            ms_b.append(timed(base_step, warmup, iters))
                        ens.set_profiling(True)
                        ens.reset_kernel_times()
                        for _ in range(2):
                            ens_step()
                        torch.cuda.synchronize()
                        kt = {k: round(ens.kernel_time(k)[0] / 2, 3) for k in ENS_KERNELS}
                        desc = ens.describe().split(" | env")[0]
                    e, b = float(np.median(ms_e)), float(np.median(ms_b))
                    row.update(ensemble_ms_per_iteration=round(e, 3), ensemble_ms_rounds=[round(x, 3) for x in ms_e],
                               one_after_another_ms_per_iteration=round(b, 3), one_after_another_ms_rounds=[round(x, 3) for x in ms_b],
                               ensemble_model_iterations_per_s=round(K * 1e3 / e, 2), one_after_another_model_iterations_per_s=round(K * 1e3 / b, 2),
                               speedup=round(b / e, 3), ensemble_kernel_ms_per_iteration=kt, finite=bool(torch.isfinite(out[:, P + 6]).all().item()),
                               bytes_per_model=int(desc.split("tape_bytes_per_model=")[1].split()[0]), describe=desc)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del W, out, m, v, Wb, mb, vb
                    torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", action="store_true")
    ap.add_argument("--conv", type=int, default=3)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ensemble:
        return ensemble_sweep(a)
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
