#!/usr/bin/env python
"""One ensemble launch against K single-model launches for one embedded iteration (step + flux) of K wind-mixing models.

One process, warm, HIP-event time through `colnde_kernel_time` (slot 10), mean of `--reps` iterations:
    ensemble   colnde_ensemble_wm_embedded_dev on one ensemble handle, all output groups: ms per call
    singles    colnde_wm_embedded_step_flux_dev once per model on K single-model handles (the code of the parent commit): the sum of the K launches' ms
Both are also timed on the host clock around the synchronised loop (`wall_ms`: what an embedding that waits for the state sees, launch gaps included).
No ratio is fixed in advance; where the one launch loses, the K launches are dispatched behind the same ABI from that size on.

    python tools/wm_ens_embed_rate.py --out profiles/wm_ens_embed_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MPP = (1e-4, 1e-1, 1.0, 0.25, 1.0, 1.67e-4, 9.81)
SIZES = ((8, 8), (8, 18), (8, 4096), (64, 8), (64, 18), (64, 4096), (512, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, nargs="+", default=["%dx%d" % s for s in SIZES], help="KxN_COL")
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
    x0 = torch.from_numpy(base.x0).to(dev)
    bcs = torch.from_numpy(base.bcs.astype(np.float32)).to(dev)
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, results=[],
               metric="ms per embedded iteration of all K models (step + flux), HIP events, mean of reps; singles = sum over the K launches")
    rng = np.random.default_rng(0)
    singles = []
    try:
        for size in a.sizes:
            K, n = (int(x) for x in size.split("x"))
            while len(singles) < K:
                singles.append(colnde.ColumnNDE(base.cfg, 4))
            w = torch.from_numpy(np.stack([synthetic.perturb_weights(rng, base.weights_truth, 0.05) for _ in range(K)])).to(dev)
            off = torch.arange(1, K + 1, device=dev, dtype=torch.float32).view(K, 1, 1)
            u, v, T = ((sg[f] * x0[:n, 32 * f:32 * f + 32] + mu[f]).unsqueeze(0) + c * off for f, c in zip(range(3), (0.003, -0.002, 0.05)))
            u, v, T = u.contiguous(), v.contiguous(), T.contiguous()
            top = torch.stack([sg[3 + k] * bcs[:n, 1 + 2 * k] + mu[3 + k] for k in range(3)]).contiguous()
            hb = torch.stack([u[:, :, 0] - 1e-3, v[:, :, 0] + 2e-3, T[:, :, 0] - 0.01], dim=1).contiguous()
            ht = torch.stack([u[:, :, -1] + 2e-3, v[:, :, -1] - 1e-3, T[:, :, -1] + 0.01], dim=1).contiguous()
            params = np.tile(np.float32(MPP), (K, 1)) * np.float32(1 + 0.001 * np.arange(K))[:, None]
            # the single-model arguments: model k's own 16-byte-aligned arrays (a slice of the faces [K][n][33] is not aligned for every n)
            per = [dict(w=w[k], u=u[k], v=v[k], T=T[k], hb=hb[k].contiguous(), ht=ht[k].contiguous(), pr=tuple(float(x) for x in params[k]),
                        dz=tuple(torch.empty_like(T[k]) for _ in range(3)), out=tuple(torch.empty_like(T[k]) for _ in range(3)),
                        faces=tuple(torch.empty((n, 33), device=dev) for _ in range(3))) for k in range(K)]

            def run_singles():
                for k in range(K):
                    q = per[k]
                    singles[k].wm_embedded_step_flux(q["w"], q["u"], q["v"], q["T"], top, 256.0, 60.0, q["pr"], True, (q["hb"], q["ht"]), dz_out=q["dz"],
                                                     out=q["out"], faces_out=q["faces"])

            row = dict(models=K, columns=n)
            with colnde.ColumnNDEEnsemble(base.cfg, 8, K) as ens:
                run_ens = lambda: ens.wm_embedded(w, u, v, T, top, 256.0, 60.0, params, True, hb, ht)
                timed = {"ensemble": (run_ens, [ens]), "singles": (run_singles, singles[:K])}
                for name, (fn, handles) in timed.items():
                    for h in handles:
                        h.set_profiling(False)
                    for _ in range(a.warmup):
                        r = fn()
                    torch.cuda.synchronize()
                    for h in handles:
                        h.reset_kernel_times()
                        h.set_profiling(True)
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        r = fn()
                    torch.cuda.synchronize()
                    wall = (time.perf_counter() - t0) * 1e3 / a.reps
                    ms, launches = 0.0, 0
                    for h in handles:
                        t, l = h.kernel_time("flux_diag")
                        ms += t
                        launches += l
                        h.set_profiling(False)
                    assert launches == a.reps * len(handles), (name, launches)
                    row[name] = dict(ms=ms / a.reps, wall_ms=wall, launches_per_iteration=len(handles))
                    if name == "ensemble":
                        r_ens = r
                # the same bits, while both results are at hand
                for k in (0, K - 1):
                    for x, y in zip(r_ens.dz + r_ens.state + r_ens.faces, per[k]["dz"] + per[k]["out"] + per[k]["faces"]):
                        assert torch.equal(x[k], y), (K, n, k)
            row["singles_over_ensemble"] = row["singles"]["ms"] / row["ensemble"]["ms"]
            row["one_launch_wins"] = bool(row["ensemble"]["ms"] < row["singles"]["ms"])
            doc["results"].append(row)
            print(json.dumps(row), flush=True)
    finally:
        for h in singles:
            h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
