#!/usr/bin/env python
"""What a step schedule buys on an uneven time axis: `loss_grad` under the minimal schedule against one global sub-step count, same build, same problem.

18 simulations (the reference's largest training set) on the axis of save intervals 1, 1, 1, 1, 4, 8 (units of 1/256) repeated to 97 save points.
Handle A steps by the per-interval stability minima rounded up to powers of two (2, 2, 2, 2, 8, 16, ...: `colnde.schedule_min`); handle B by
`substeps = U`, the count `choose_substeps` settles on at reltol = 1e-3 (the longest interval dictates it).  Per handle: kernel milliseconds of one
`loss_grad` (forward with tapes + adjoint + dW GEMM + reduction) from the library's HIP events (`colnde_kernel_time`), `--repeats` calls after
`--warmup`, the two handles alternating; median, min and max.  Writes one JSON object (stdout and --out).

    python tools/schedule_rate.py --out profiles/schedule_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("forward", "adjoint", "dw1", "reduce")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=18)
    ap.add_argument("--periods", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--reltol", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    units = np.concatenate([[0], np.cumsum(np.tile([1, 1, 1, 1, 4, 8], a.periods))])
    p = synthetic.wind_mixing_problem(a.columns, n_frames=4, n_frames_total=257, weight_divisor=1e2)
    cfg = p.cfg.with_(save_times=tuple((units / 256.0).tolist()))
    dev = torch.device("cuda", 0)
    x0, bcs, w, wt = (torch.as_tensor(v).to(dev) for v in (p.x0, p.bcs, p.weights, p.weights_truth))
    sc = [1, 1, 1, 5e-3, 5e-3, 5e-3]
    S = []
    for v in colnde.schedule_min(cfg):
        c = 1
        while c < v:
            c *= 2
        S.append(c)
    with colnde.ColumnNDE(cfg, a.columns) as probe:
        probe.set_problem(x0, bcs)
        U, est_u = probe.choose_substeps(p.weights, a.reltol)
        truth = probe.forward(wt)
        probe.set_schedule(S)
        est_s = probe.error_estimate(p.weights)
    out = torch.empty(cfg.n_params + 8, dtype=torch.float32, device=dev)
    with colnde.ColumnNDE(cfg, a.columns) as hs, colnde.ColumnNDE(cfg, a.columns) as hu:
        hs.set_schedule(S)
        hu.set_substeps(U)
        ms = {}
        for h in (hs, hu):
            h.set_problem(x0, bcs, truth)
            h.set_profiling(True)
            for _ in range(a.warmup):
                h.loss_grad(w, sc, out=out)
            ms[h] = {k: [] for k in KERNELS + ("total",)}
        torch.cuda.synchronize()
        for r in range(a.repeats):
            for h in ((hs, hu) if r % 2 == 0 else (hu, hs)):
                h.reset_kernel_times()
                h.loss_grad(w, sc, out=out)
                torch.cuda.synchronize()
                t = {k: h.kernel_time(k)[0] for k in KERNELS}
                for k in KERNELS:
                    ms[h][k].append(t[k])
                ms[h]["total"].append(sum(t.values()))

        def stats(h):
            return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in ms[h].items()}
        res = dict(columns=a.columns, n_save=cfg.n_save, axis="(1,1,1,1,4,8)/256 x %d" % a.periods, reltol=a.reltol, repeats=a.repeats, device=torch.cuda.get_device_name(0),
                   schedule=dict(counts_per_period=S[:6], total_steps=hs.n_steps, estimate=est_s, ms=stats(hs), describe=hs.describe()),
                   substeps=dict(U=U, total_steps=hu.n_steps, estimate=est_u, ms=stats(hu), describe=hu.describe()))
        res["steps_ratio"] = hu.n_steps / hs.n_steps
        res["ms_ratio"] = res["substeps"]["ms"]["total"]["median"] / res["schedule"]["ms"]["total"]["median"]
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
