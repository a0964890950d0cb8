#!/usr/bin/env python
"""Rate of judging a wind-mixing sweep: ONE `colnde_ensemble_profile_dev` call (fluxes and Ri of all K x simulations x frames states in one launch of
wm_profile_ens_kernel) against the path available before it: K x n_save `colnde_flux_dev` calls on K single handles.  The shape is the reference's
judging of a sweep, 64 members x 18 simulations x 129 frames, and the same with 1 member.

HIP-event time through `colnde_kernel_time` (slot `wm_profile`; slot `rhs` summed over the K handles), warm: `--warmup` passes, then `--groups` groups
of `--reps` passes; per group the mean per pass, reported as the median over the groups with their spread (max - min).  A pass of the old path is
K x n_save launches, so its groups hold `--old-reps` passes.  The host clock around the same passes (ending in a synchronise) is reported beside it:
the old path's launches are small, and what a user waits for is the wall time.  The matrix-pipe bound of the new launch: ceil(tiles / (4 CUs'
SIMDs)) x 345 v_mfma_f32_32x32x2_f32 x 64 cycles at `--ghz`.  Writes one JSON document.

    python tools/wm_profile_rate.py --out profiles/wm_profile_rate.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _git(*args):
    try:
        return subprocess.check_output(("git", "-C", ROOT) + args, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def _groups(fn, read_ms, engines, warmup, groups, reps, sync):
    """-> (event ms per pass, wall ms per pass), each [groups]"""
    for _ in range(warmup):
        fn()
    sync()
    ev, wall = [], []
    for _ in range(groups):
        for e in engines:
            e.reset_kernel_times()
            e.set_profiling(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        wall.append((time.perf_counter() - t0) * 1e3 / reps)
        for e in engines:
            e.set_profiling(False)
        ev.append(read_ms(reps) / reps)
    return ev, wall


def _stat(per):
    return dict(ms_median=statistics.median(per), ms_spread=max(per) - min(per), ms_groups=per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--simulations", type=int, default=18)
    ap.add_argument("--frames", type=int, default=129)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--old-reps", type=int, default=2)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lib = colnde.LIB_PATH
    doc = dict(device=torch.cuda.get_device_name(0), compute_units=n_cu, warmup=a.warmup, groups=a.groups, reps=a.reps, old_reps=a.old_reps,
               build=dict(library=os.path.basename(lib), library_bytes=os.path.getsize(lib), flags="-O3 --offload-arch=gfx950 (csrc/Makefile)",
                          commit=_git("rev-parse", "HEAD"), tree_dirty=bool(_git("status", "--porcelain")) if _git("rev-parse", "HEAD") else None),
               method="hipEvent pairs around each launch (colnde_kernel_time), per group mean per pass, median and spread (max - min) over the groups; "
                      "wall: host clock around the same passes, ending in a synchronise",
               results=[])
    n, ns = a.simulations, a.frames
    p = synthetic.wind_mixing_problem(n, n_frames=ns, weight_divisor=10, diurnal=True)
    times = [float(np.float32(t)) for t in p.cfg.save_times]
    sync = torch.cuda.synchronize
    for K in a.members:
        W = np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 10) for k in range(K)]).astype(np.float32)
        rng = np.random.default_rng(3)
        # states to diagnose: the initial profiles, smoothly perturbed per member and frame (the call solves nothing; the time does not depend on the values)
        sol = (p.x0[None, :, None, :] + 0.05 * rng.standard_normal((K, n, ns, 1)).astype(np.float32) * np.sin(np.linspace(0, 3, 96, dtype=np.float32))).astype(np.float32)
        Wd, sd, bd = torch.from_numpy(W).to(dev), torch.from_numpy(np.ascontiguousarray(sol)).to(dev), torch.from_numpy(p.bcs).to(dev)
        row = dict(members=K, simulations=n, frames=ns, states=K * n * ns)
        with colnde.ColumnNDEEnsemble(p.cfg, n, K) as ens:
            doc["describe"] = ens.describe()
            ens.set_problem(p.x0, p.bcs)
            new = lambda: ens.profile(Wd, sd, losses=False)
            got = new()

            def read_new(reps):
                ms, launches = ens.kernel_time("wm_profile")
                assert launches == reps, launches
                return ms
            ev, wall = _groups(new, read_new, [ens], a.warmup, a.groups, a.reps, sync)
            row["profile_launch"], row["profile_wall"] = _stat(ev), _stat(wall)
        singles = [colnde.ColumnNDE(p.cfg, n) for _ in range(K)]
        try:
            frames = [[sd[k, :, f].contiguous() for f in range(ns)] for k in range(K)]

            def old():
                for k, h in enumerate(singles):
                    for f in range(ns):
                        h.flux(frames[k][f], Wd[k], bd, times[f])

            def read_old(reps):
                tot = 0.0
                for h in singles:
                    ms, launches = h.kernel_time("rhs")
                    assert launches == reps * ns, launches
                    tot += ms
                return tot
            ev, wall = _groups(old, read_old, singles, 1, a.groups, a.old_reps, sync)
            row["flux_calls"], row["flux_calls_wall"] = _stat(ev), _stat(wall)
            ref = torch.stack([singles[0].flux(frames[0][f], Wd[0], bd, times[f]) for f in range(ns)], dim=1)          # [n, ns, 3, 33]
            row["max_abs_difference_member0"] = float(max((ref[:, :, q] - g[0]).abs().max() for q, g in enumerate((got.uw, got.vw, got.wT))))
        finally:
            for h in singles:
                h.close()
        tiles = K * ((n * ns + 31) // 32)
        bound_ms = -(-tiles // (4 * n_cu)) * 345 * 64 / (a.ghz * 1e6)
        row["matrix_pipe_bound_ms"] = bound_ms
        row["fraction_of_matrix_pipe_bound"] = bound_ms / row["profile_launch"]["ms_median"]
        row["speedup_events"] = row["flux_calls"]["ms_median"] / row["profile_launch"]["ms_median"]
        row["speedup_wall"] = row["flux_calls_wall"]["ms_median"] / row["profile_wall"]["ms_median"]
        gain = row["flux_calls"]["ms_median"] - row["profile_launch"]["ms_median"]
        row["faster_beyond_spread"] = gain > max(row["flux_calls"]["ms_spread"], row["profile_launch"]["ms_spread"])
        doc["results"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {"ms_median": v["ms_median"], "ms_spread": v["ms_spread"]}) for k, v in row.items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
