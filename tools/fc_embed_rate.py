#!/usr/bin/env python
"""Rate of the free-convection embedded step: the fused `colnde_fc_embedded_step_dev`, the diagnosis-only `colnde_fc_diagnose_wT_dev` and, in
the same process, the existing pair `colnde_infer_dz_wT_dev` + `colnde_convective_adjustment_dev`, for Nz = 32 and 64 at 9,216 (96 x 96),
65,536 and 1,048,576 columns.

HIP-event time through `colnde_kernel_time`: `--warmup` launches, then `--groups` groups of `--reps` launches; per group the mean per launch,
reported as the median over the groups with their spread (max − min) beside it.  The fused call is KEPT where its median is below the pair's
median by more than the larger of the two spreads.  Writes one JSON document.

    python tools/fc_embed_rate.py --out profiles/fc_embed_rate.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LZ, DT, K = 1000.0, 600.0, 10.0


def _git(*args):
    try:
        return subprocess.check_output(("git", "-C", ROOT) + args, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[9216, 65536, 1048576])
    ap.add_argument("--levels", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    lib = colnde.LIB_PATH
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, groups=a.groups, reps=a.reps, Lz=LZ, dt=DT, K=K,
               build=dict(library=os.path.basename(lib), library_bytes=os.path.getsize(lib), library_mtime=int(os.path.getmtime(lib)),
                          flags="-O3 --offload-arch=gfx950 (csrc/Makefile)", commit=_git("rev-parse", "HEAD"),
                          tree_dirty=bool(_git("status", "--porcelain")) if _git("rev-parse", "HEAD") else None),
               method="hipEvent pairs around each launch (colnde_kernel_time); per group mean per launch; median and spread (max - min) over the groups",
               results=[])
    for Nz in a.levels:
        cfg, T0, _, w0 = synthetic.inference_problem(64, 64, Nz=Nz)
        with colnde.ColumnNDE(cfg, 4) as nde:
            doc.setdefault("describe", {})[str(Nz)] = nde.describe()
            w = torch.from_numpy(w0).to(dev)
            base = torch.from_numpy(T0).to(dev)
            for n in a.columns:
                T = base.repeat((n + 4095) // 4096, 1)[:n].contiguous()
                top = torch.full((n,), 1e-5, device=dev)
                dz, To = torch.empty_like(T), torch.empty_like(T)
                faces = torch.empty((n, Nz + 1), device=dev)
                calls = {
                    "fused": (("fc_embed",), lambda: nde.fc_embedded_step(w, T, top, LZ, DT, K, dz_out=dz, T_out=To)),
                    "fused_with_diagnosis": (("fc_embed",), lambda: nde.fc_embedded_step(w, T, top, LZ, DT, K, dz_out=dz, T_out=To, faces_out=faces)),
                    "diagnose_only": (("fc_embed",), lambda: nde.fc_diagnose_wT(w, T, top, LZ, K, faces_out=faces)),
                    "two_launches": (("infer", "convadj"), lambda: (nde.infer_dz_wT(w, T, top, LZ), nde.convective_adjustment(T, DT, LZ / Nz, K, out=To))),
                }
                row = dict(Nz=Nz, columns=n, tile_width=16 if n <= 4096 else 32)
                for name, (slots, fn) in calls.items():
                    os.environ["COLNDE_FC_EMBED_FUSED"] = "1" if name == "fused" else "0"      # the entry point itself issues two launches
                    nde.set_profiling(False)
                    for _ in range(a.warmup):
                        fn()
                    torch.cuda.synchronize()
                    per = []
                    for _ in range(a.groups):
                        nde.reset_kernel_times()
                        nde.set_profiling(True)
                        for _ in range(a.reps):
                            fn()
                        torch.cuda.synchronize()
                        nde.set_profiling(False)
                        ms = 0.0
                        for s in slots:
                            t, launches = nde.kernel_time(s)
                            assert launches == a.reps, (name, s, launches)
                            ms += t
                        per.append(ms / a.reps)
                    row[name] = dict(ms_median=statistics.median(per), ms_spread=max(per) - min(per), ms_groups=per)
                assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(To).all()) and bool(torch.isfinite(faces).all())
                gain = row["two_launches"]["ms_median"] - row["fused"]["ms_median"]
                row["fused_gain_ms"] = gain
                row["fused_wins_beyond_spread"] = gain > max(row["two_launches"]["ms_spread"], row["fused"]["ms_spread"])
                doc["results"].append(row)
                print(json.dumps({k: (v if not isinstance(v, dict) else {"ms_median": v["ms_median"], "ms_spread": v["ms_spread"]}) for k, v in row.items()}),
                      flush=True)
    doc["keep_fused"] = all(r["fused_wins_beyond_spread"] for r in doc["results"] if r["columns"] in (9216, 65536))
    print(json.dumps(dict(keep_fused=doc["keep_fused"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
