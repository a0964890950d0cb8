#!/usr/bin/env python
"""Rate of the wind-mixing flux diagnosis and the decision between one launch and two for `colnde_wm_embedded_step_flux`.

One process, HIP-event time through `colnde_kernel_time`, `--warmup` launches, then the median and the spread (max − min) over `--groups`
groups of `--reps` launches (mean per launch within a group), at each column count:
    diagnosis   colnde_wm_diagnose_flux_dev alone (slot 10)
    step        colnde_wm_embedded_step_dev, the existing kernel: the yardstick (slot 4)
    step_flux   colnde_wm_embedded_step_flux_dev, one launch (slot 10)
    baseline    colnde_mpp_diagnose_flux_dev (slot 10)
and step + diagnosis, the two launches the one replaces.  Rule (fixed before measuring): the one launch stays only if it beats
step + diagnosis by more than the spread at 9,216 and at 65,536 columns.  Writes one JSON document.

    python tools/wm_diag_rate.py --out profiles/wm_diag_rate.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MPP = (1e-4, 1e-1, 1.0, 0.25, 1.0, 1.67e-4, 9.81)
RULE_SIZES = (9216, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[9216, 65536, 1048576])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    base = synthetic.wind_mixing_problem(4096, n_frames=3, weight_divisor=1.0)
    mu, sg = base.cfg.mu, base.cfg.sigma
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, groups=a.groups, reps=a.reps, results=[],
               rule="one launch stays only if step_flux < step + diagnosis by more than the spread at 9,216 and 65,536 columns")
    with colnde.ColumnNDE(base.cfg, 4) as nde:
        doc["describe"] = nde.describe()
        w = torch.from_numpy(base.weights_truth).to(dev)
        for n in a.columns:
            rep = (n + 4095) // 4096
            x0 = torch.from_numpy(base.x0).to(dev).repeat(rep, 1)[:n]
            u, v, T = ((sg[f] * x0[:, 32 * f:32 * f + 32] + mu[f]).contiguous() for f in range(3))
            bcs = torch.from_numpy(base.bcs.astype(np.float32)).to(dev).repeat(rep, 1)[:n]
            top = torch.stack([sg[3 + k] * bcs[:, 1 + 2 * k] + mu[3 + k] for k in range(3)]).contiguous()
            hb = torch.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] - 0.01]).contiguous()
            ht = torch.stack([u[:, -1] + 2e-3, v[:, -1] - 1e-3, T[:, -1] + 0.01]).contiguous()
            dz = tuple(torch.empty_like(T) for _ in range(3))
            out = tuple(torch.empty_like(T) for _ in range(3))
            faces = tuple(torch.empty((n, 33), dtype=T.dtype, device=dev) for _ in range(3))
            calls = {
                "diagnosis": ("flux_diag", lambda: nde.wm_diagnose_flux(w, u, v, T, top, 256.0, MPP, True, (hb, ht), faces_out=faces)),
                "step": ("infer", lambda: nde.wm_embedded_step(w, u, v, T, top, 256.0, 60.0, MPP, True, hb, dz_out=dz, out=out)),
                "step_flux": ("flux_diag", lambda: nde.wm_embedded_step_flux(w, u, v, T, top, 256.0, 60.0, MPP, True, (hb, ht), dz_out=dz, out=out,
                                                                             faces_out=faces)),
                "baseline": ("flux_diag", lambda: nde.mpp_diagnose_flux(u, v, T, top, 8.0, MPP, True, hb, faces_out=faces)),
            }
            row = dict(columns=n)
            for name, (slot, fn) in calls.items():
                nde.set_profiling(False)
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.groups):
                    nde.reset_kernel_times()
                    nde.set_profiling(True)
                    for _ in range(a.reps):
                        fn()
                    torch.cuda.synchronize()
                    t, launches = nde.kernel_time(slot)
                    assert launches == a.reps, (name, launches)
                    ms.append(t / launches)
                    nde.set_profiling(False)
                row[name] = dict(ms_median=statistics.median(ms), ms_spread=max(ms) - min(ms), ms_groups=ms)
            assert all(bool(torch.isfinite(t).all()) for t in dz + out + faces)
            two = row["step"]["ms_median"] + row["diagnosis"]["ms_median"]
            spread = max(row["step_flux"]["ms_spread"], row["step"]["ms_spread"] + row["diagnosis"]["ms_spread"])
            row["step_plus_diagnosis_ms"] = two
            row["spread_ms"] = spread
            row["one_launch_wins"] = bool(two - row["step_flux"]["ms_median"] > spread)
            doc["results"].append(row)
            print(json.dumps(row), flush=True)
    sizes = {r["columns"]: r["one_launch_wins"] for r in doc["results"]}
    if all(n in sizes for n in RULE_SIZES):
        doc["outcome"] = "one launch" if all(sizes[n] for n in RULE_SIZES) else "two launches"
        print("outcome:", doc["outcome"], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
