#!/usr/bin/env python
"""Rate of the wind-mixing embedded inference: `colnde_wm_infer_dz_flux_dev` (forcing only), `colnde_wm_embedded_step_dev` (fused with the
implicit diffusion step) and, in the same process, the unchanged `colnde_implicit_diffusion_dev`.

HIP-event time of each kernel through `colnde_kernel_time` (warm; `--reps` launches, mean per launch) and the achieved GB/s on the
algorithmic bytes per column: forcing 384 in + 384 out, fused 384 in + 768 out, diffusion 384 in + 384 out.  The yardstick of the fused
call is the sum of the other two from the same run.  Writes one JSON document.

    python tools/wm_infer_rate.py --out profiles/wm_infer_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"forcing": 768, "fused": 1152, "implicit_diffusion": 768}
MPP = (1e-4, 1e-1, 1.0, 0.25, 1.0, 1.67e-4, 9.81)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    base = synthetic.wind_mixing_problem(4096, n_frames=3, weight_divisor=1.0)
    mu, sg = base.cfg.mu, base.cfg.sigma
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, bytes_per_column=BYTES, results=[])
    with colnde.ColumnNDE(base.cfg, 4) as nde:
        doc["describe"] = nde.describe()
        w = torch.from_numpy(base.weights_truth).to(dev)
        for n in a.columns:
            rep = (n + 4095) // 4096
            x0 = torch.from_numpy(base.x0).to(dev).repeat(rep, 1)[:n]
            u, v, T = ((sg[f] * x0[:, 32 * f:32 * f + 32] + mu[f]).contiguous() for f in range(3))
            bcs = torch.from_numpy(base.bcs.astype(np.float32)).to(dev).repeat(rep, 1)[:n]
            top = torch.stack([sg[3 + k] * bcs[:, 1 + 2 * k] + mu[3 + k] for k in range(3)]).contiguous()
            dz = tuple(torch.empty_like(T) for _ in range(3))
            out = tuple(torch.empty_like(T) for _ in range(3))
            calls = {
                "forcing": ("infer", lambda: nde.wm_infer_dz_flux(w, u, v, T, top, 256.0, dz_out=dz)),
                "fused": ("infer", lambda: nde.wm_embedded_step(w, u, v, T, top, 256.0, 60.0, MPP, True, dz_out=dz, out=out)),
                "implicit_diffusion": ("impldiff", lambda: nde.implicit_diffusion(u, v, T, 60.0, 8.0, MPP, True, out=out)),
            }
            row = dict(columns=n)
            for name, (slot, fn) in calls.items():
                nde.set_profiling(False)
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                nde.reset_kernel_times()
                nde.set_profiling(True)
                for _ in range(a.reps):
                    fn()
                torch.cuda.synchronize()
                ms, launches = nde.kernel_time(slot)
                assert launches == a.reps, (name, launches)
                row[name] = dict(ms=ms / launches, gb_per_s=BYTES[name] * n / (ms / launches) * 1e-6)
            nde.set_profiling(False)
            assert all(bool(torch.isfinite(t).all()) for t in dz + out)
            row["forcing_plus_diffusion_ms"] = row["forcing"]["ms"] + row["implicit_diffusion"]["ms"]
            row["fused_below_sum"] = row["fused"]["ms"] < row["forcing_plus_diffusion_ms"]
            doc["results"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
