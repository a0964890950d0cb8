#!/usr/bin/env python
"""One ensemble launch against K single-model launches for one embedded iteration (step + faces) of K free-convection networks.

One process, warm, HIP-event time through `colnde_kernel_time` (slot 9: the embedded kernel alone), mean of `--reps` iterations:
    ensemble        colnde_ensemble_fc_embedded_dev on one ensemble handle with weights given (the K images are packed every call): ms per call
    ensemble_reuse  the same with weights = NULL (the images of the previous call)
    singles         colnde_fc_embedded_step_dev with faces once per member on K single-model handles (the code of the parent commit): the sum of
                    the K launches' ms.  Plain members only: no single-model call runs a --conv network.
Slot 9 does not contain the pack (neither here nor in the single-model call), so all three are also timed on the host clock around the
synchronised loop (`wall_ms`: what an embedding that waits for the state sees — packs and launch gaps included).  The pack's share is
`ensemble.wall_ms - ensemble_reuse.wall_ms`.  No ratio is fixed in advance.

    python tools/fc_ens_embed_rate.py --out profiles/fc_ens_embed_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS, COLUMNS, LEVELS, CONVS = (8, 64, 512), (9, 4096), (32, 64), (0, 3)       # 9: the reference's 9 simulations
LZ, DT, K_CA = 1000.0, 600.0, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, nargs="+", default=list(MODELS))
    ap.add_argument("--columns", type=int, nargs="+", default=list(COLUMNS))
    ap.add_argument("--levels", type=int, nargs="+", default=list(LEVELS))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    from colnde.free_convection import conv_n_params
    dev = torch.device("cuda", 0)
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, results=[],
               metric="ms per embedded iteration of all K members (step + faces); ms: HIP events around the embedded kernel(s), mean of reps, singles = sum "
                      "over the K launches; wall_ms: host clock around the synchronised loop, packs included")
    rng = np.random.default_rng(0)

    def timed(fn, handles, n_launches):
        for h in handles:
            h.set_profiling(False)
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        for h in handles:
            h.reset_kernel_times()
            h.set_profiling(True)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / a.reps
        ms, launches = 0.0, 0
        for h in handles:
            t, l = h.kernel_time("fc_embed")
            ms += t
            launches += l
            h.set_profiling(False)
        assert launches == a.reps * n_launches, (launches, n_launches)
        return dict(ms=ms / a.reps, wall_ms=wall, launches_per_iteration=n_launches)

    for Nz in a.levels:
        cfg = synthetic.free_convection_problem(4, Nz=Nz, n_save=3, substeps=2, t_end=0.01).cfg
        singles = []
        try:
            for K in a.models:
                for n in a.columns:
                    T = (torch.linspace(5.0, 25.0, Nz, device=dev).view(1, 1, Nz) + 0.5 * torch.randn((K, n, Nz), device=dev)).contiguous()
                    top = (1e-5 * torch.randn(n, device=dev)).contiguous()
                    hb, ht = (T[:, :, 0] - 0.1).contiguous(), (T[:, :, -1] + 0.1).contiguous()
                    dz, To = torch.empty_like(T), torch.empty_like(T)
                    for c in CONVS:
                        P = conv_n_params(Nz, c) if c else cfg.n_params
                        w = torch.from_numpy((rng.standard_normal((K, P)) * 0.05).astype(np.float32)).to(dev)
                        row = dict(levels=Nz, models=K, columns=n, conv=c)
                        with colnde.FreeConvectionEnsemble(cfg, 4, K, conv=c) as ens:
                            row["ensemble"] = timed(lambda: ens.fc_embedded(w, T, top, LZ, K_CA, DT, (hb, ht), dz_out=dz, T_out=To), [ens], 1)
                            r_ens = ens.fc_embedded(w, T, top, LZ, K_CA, DT, (hb, ht))
                            row["ensemble_reuse"] = timed(lambda: ens.fc_embedded(None, T, top, LZ, K_CA, DT, (hb, ht), dz_out=dz, T_out=To), [ens], 1)
                            row["pack_wall_ms"] = row["ensemble"]["wall_ms"] - row["ensemble_reuse"]["wall_ms"]
                            if not c:
                                while len(singles) < K:
                                    singles.append(colnde.ColumnNDE(cfg, 4))
                                # the single-model arguments: member k's own 16-byte-aligned arrays (a slice of the faces [K][n][Nz+1] is not aligned for every n)
                                per = [dict(w=w[k], T=T[k], hb=hb[k].contiguous(), ht=ht[k].contiguous(), dz=torch.empty_like(T[k]), To=torch.empty_like(T[k]),
                                            f=torch.empty((n, Nz + 1), device=dev)) for k in range(K)]

                                def run_singles():
                                    for k in range(K):
                                        q = per[k]
                                        singles[k].fc_embedded_step(q["w"], q["T"], top, LZ, DT, K_CA, (q["hb"], q["ht"]), dz_out=q["dz"], T_out=q["To"],
                                                                    faces_out=q["f"])
                                row["singles"] = timed(run_singles, singles[:K], K)
                                for k in (0, K - 1):                              # the same bits, while both results are at hand
                                    assert torch.equal(r_ens.dz_wT[k], per[k]["dz"]) and torch.equal(r_ens.T_new[k], per[k]["To"])
                                    assert torch.equal(r_ens.faces[k], per[k]["f"]), (Nz, K, n, k)
                                del per
                                row["singles_over_ensemble"] = row["singles"]["ms"] / row["ensemble"]["ms"]
                                row["singles_over_ensemble_wall"] = row["singles"]["wall_ms"] / row["ensemble"]["wall_ms"]
                                row["one_launch_wins"] = bool(row["ensemble"]["ms"] < row["singles"]["ms"] and row["ensemble"]["wall_ms"] < row["singles"]["wall_ms"])
                            del r_ens
                        doc["results"].append(row)
                        print(json.dumps(row), flush=True)
                    del T, dz, To
                    torch.cuda.empty_cache()
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
