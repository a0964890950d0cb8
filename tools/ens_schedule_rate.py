#!/usr/bin/env python
"""What the ensemble forms of the error estimate and of the schedule choice cost against what the single-model calls offer for the same information.

The reference's shape: 8 simulations on the axis of save intervals 1, 1, 1, 1, 4, 8 (units of 1/256) repeated to 97 save points, K = 1, 16, 64 members
with their own Pacanowski-Philander constants and weights.  Per K, wall time (time.perf_counter around the call; every call synchronises) of

  ensemble    ColumnNDEEnsemble.ensemble_error_estimate / .choose_ensemble_schedule: every solve one launch for all K members
  sequential  K single handles (created and given the problem beforehand), each calling error_estimate / choose_schedule, one after another

the two alternating, `--repeats` times after one untimed call each; every repeat is recorded, the median reported, and the ratio
sequential / ensemble stated.  Also recorded: the largest relative distance between the estimate kernel and the NumPy norm of the two solutions it
compares (twin ensemble at twice the sub-steps; the tests' bound is 1e-3), and, on the tests' K = 3 problem (8 columns, 7 save points), the total of
the chosen schedule against 6 x U, U the largest `choose_substeps` of the members' single twins.  Writes one JSON object (stdout and --out).

    python tools/ens_schedule_rate.py --out profiles/ens_schedule_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHYS_KEYS = ("nu0", "nu_minus", "dRi", "Ric", "Pr")
PHYS_K3 = np.array([[1e-4, 0.13, 1.0, 0.25, 1.0], [5e-4, 0.12, 0.8, 0.2, 1.0], [1e-3, 0.05, 1.3, 0.3, 1.2]], np.float32)    # tests/ens_schedule_cases.py


def norm(a, b, factor, floor=1e-3):
    """[K, n_save]: max over columns of rms_i((a_i - b_i) / (floor + |b_i|)), times Richardson's factor"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = (a - b) / (floor + np.abs(b))
    return factor * np.sqrt((q * q).mean(axis=-1)).max(axis=1)


def physics(K, rng):
    """K constant sets around the reference's defaults: nu_minus 0.05 .. 0.13 (it sets the stability bound: 16 steps cover the longest interval up to 0.132), the rest within their sweep ranges"""
    return np.stack([[10 ** rng.uniform(-4, -3), rng.uniform(0.05, 0.13), rng.uniform(0.6, 1.3), rng.uniform(0.15, 0.35), rng.uniform(1.0, 2.0)] for _ in range(K)]).astype(np.float32)


def attempt(fn):
    """fn's result, or the library's message when it refuses"""
    from colnde import ColndeError
    try:
        return fn()
    except ColndeError as ex:
        return str(ex)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--periods", type=int, default=16)
    ap.add_argument("--members", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reltol", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    units = np.concatenate([[0], np.cumsum(np.tile([1, 1, 1, 1, 4, 8], a.periods))])
    p = synthetic.wind_mixing_problem(a.columns, n_frames=4, n_frames_total=257, weight_divisor=1e2)
    cfg = p.cfg.with_(save_times=tuple((units / 256.0).tolist()), substeps=16)          # one count on this axis: the longest interval needs 13
    res = dict(columns=a.columns, n_save=cfg.n_save, axis="(1,1,1,1,4,8)/256 x %d" % a.periods, substeps=cfg.substeps, reltol=a.reltol, repeats=a.repeats,
               device=torch.cuda.get_device_name(0), members={})
    worst = 0.0
    for K in a.members:
        rng = np.random.default_rng(K)
        ph = physics(K, rng)
        W = np.stack([synthetic.make_weights(synthetic._rng(11, k), cfg, 1e2) for k in range(K)]).astype(np.float32)
        singles = [colnde.ColumnNDE(cfg.with_(**dict(zip(PHYS_KEYS, [float(v) for v in ph[k]]))), a.columns) for k in range(K)]
        try:
            with colnde.ColumnNDEEnsemble(cfg, a.columns, K, physics=ph) as e:
                for h in singles + [e]:
                    h.set_problem(p.x0, p.bcs, None)
                ens_est = lambda: e.ensemble_error_estimate(W)
                seq_est = lambda: np.array([h.error_estimate(W[k]) for k, h in enumerate(singles)])
                # a choice may end in one of the rule's failures (the estimate falling by less than a fifth in a round reads as the float32 floor): that is
                # a result too — recorded with its message, the time being the time to it
                ens_choose = lambda: attempt(lambda: e.choose_ensemble_schedule(W, a.reltol))
                seq_choose = lambda: [attempt(lambda: h.choose_schedule(W[k], a.reltol)) for k, h in enumerate(singles)]
                rec = {}
                # the estimates first, on handles without a schedule (a choice leaves one behind)
                dist = None
                if K <= 16:                                                         # (a twin's tapes are sized for twice the steps: not at K = 64)
                    with colnde.ColumnNDEEnsemble(cfg.with_(substeps=2 * cfg.substeps), a.columns, K, physics=ph) as twin:
                        twin.set_problem(p.x0, p.bcs, None)
                        dist = float(np.max(np.abs(ens_est()[:, 1:] / norm(e.forward(W), twin.forward(W), 16.0 / 15.0)[:, 1:] - 1.0)))
                    worst = max(worst, dist)
                for name, ens, seq in (("error_estimate", ens_est, seq_est), ("choose_schedule", ens_choose, seq_choose)):
                    ens(), seq()                                                    # untimed: first-use allocations, the kernels' code objects
                    t = dict(ensemble=[], sequential=[])
                    for r in range(a.repeats):
                        for which in (("ensemble", "sequential") if r % 2 == 0 else ("sequential", "ensemble")):
                            dt, out = timed(ens if which == "ensemble" else seq)
                            t[which].append(dt)
                            if which == "ensemble":
                                got_e = out
                            else:
                                got_s = out
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    rec[name] = dict(seconds=t, median=med, sequential_over_ensemble=med["sequential"] / med["ensemble"])
                    if name == "error_estimate":
                        rec[name]["largest_member_distance"] = float(np.max(np.abs(got_e.max(axis=1) / got_s - 1.0)))
                    else:
                        failed = [(k, r) for k, r in enumerate(got_s) if isinstance(r, str)]
                        rec[name]["sequential_failures"] = [dict(member=k, message=r) for k, r in failed]
                        if isinstance(got_e, str):
                            rec[name]["ensemble_failure"] = got_e
                        else:
                            rec[name].update(ensemble_total=int(sum(got_e[0])), ensemble_counts_first_period=list(got_e[0][:6]), ensemble_estimate=float(got_e[1].max()),
                                             driving_member=int(np.argmax(got_e[1])))
                        if not failed:
                            merged = tuple(int(v) for v in np.max([s for s, _ in got_s], axis=0))   # the merge by hand: the largest count per interval
                            rec[name].update(merged_single_total=int(sum(merged)), merged_equals_ensemble=bool(not isinstance(got_e, str) and merged == got_e[0]))
                rec["kernel_vs_numpy_norm"] = dist
                res["members"][str(K)] = rec
        finally:
            for h in singles:
                h.close()
    res["kernel_vs_numpy_norm_largest"] = worst
    # the tests' K = 3 problem: the chosen schedule against one count for all
    q = synthetic.wind_mixing_problem(8, n_frames=4, n_frames_total=257, weight_divisor=1e2)
    c3 = q.cfg.with_(save_times=tuple(k / 256.0 for k in (0, 1, 2, 3, 4, 8, 16)), substeps=16)
    W3 = np.stack([synthetic.make_weights(synthetic._rng(11, k), c3, 1e2) for k in range(3)]).astype(np.float32)
    with colnde.ColumnNDEEnsemble(c3, 8, 3, physics=PHYS_K3) as e:
        e.set_problem(q.x0, q.bcs, None)
        counts, est = e.choose_ensemble_schedule(W3, a.reltol)
    U = 0
    for k in range(3):
        with colnde.ColumnNDE(c3.with_(**dict(zip(PHYS_KEYS, [float(v) for v in PHYS_K3[k]]))), 8) as h:
            h.set_problem(q.x0, q.bcs, None)
            U = max(U, h.choose_substeps(W3[k], a.reltol)[0])
    res["k3"] = dict(counts=list(counts), total=int(sum(counts)), estimates=[float(v) for v in est], U=int(U), six_U=int(6 * U))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
