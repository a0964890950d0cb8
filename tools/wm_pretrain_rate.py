"""Seconds per pass of `train_NN` (wind_mixing/src/NN_training.jl:207-249: one ADAM update per sample) for the K x 3 flux networks of a wind-mixing sweep, on
the README's training shape — n = 2,312 samples (8 simulations x 289 frames), one ADAM pass, Nz = 32, 96-50-20-31 nets, synthetic samples:
  (a) the sweep's work before the ensemble call: `colnde_pretrain_flux_dev` on single handles, one call per (model, net) one after another, each with its
      own weights and moments.  --calls of them are timed (default 48 = 16 models x 3 nets) and the 3 K calls of a sweep are that time scaled: the calls
      are serial and each synchronises, so their time is linear in their number;
  (b) ONE `colnde_ensemble_pretrain_wm_flux_dev` call for K in {1, 16, 64, 85, 86, 256} (85: 255 workgroups, one per CU with one to spare; 86: 258, the
      first count above the 256 CUs), in each candidate form of the kernel (theta, m, v in global memory / LDS-resident) and block size (128 / 256 / 512).
      The shipped library is the candidate lds_512; the other five are experimental builds of csrc/engine_wm_pretrain.hip beside it, loaded into the same
      process (as tools/ab_bench.py does), each made by
          make -C climateparameterizations.jl_amd/csrc variant STEM=engine_wm_pretrain NAME=wmp_<form>_<block> DEFS="-DWMP_IN_LDS=<0|1> -DWMP_BLOCK=<block>"
      for <form> = global (0) | lds (1).  A candidate whose library is missing is an error; --shipped-only times lds_512 alone.
Every call synchronises its stream, so wall-clock time around a call is the time of its launch.  Each candidate gets a warm-up call (64 samples) and
--repeats timed passes (default 3), the candidates alternating inside each repeat; the least and the median are recorded.  The candidates' theta, m and v
after the pass must agree to the bit at every K (the row-bits contract), or the tool fails.
    python tools/wm_pretrain_rate.py [--out profiles/wm_pretrain_ens_rate.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import colnde
from colnde import _lib, synthetic
from colnde.flux_compat import ADAM

SHIPPED = "lds_512"
CANDIDATES = ("global_128", "global_256", "global_512", "lds_128", "lds_256", SHIPPED)
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2], [1e-3, 0.05, 1.3, 0.3, 1.0], [2e-4, 0.09, 0.6, 0.15, 2.0]], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/wm_pretrain_ens_rate.json")
    ap.add_argument("--n", type=int, default=8 * 289)
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 16, 64, 85, 86, 256])
    ap.add_argument("--shipped-only", action="store_true")
    a = ap.parse_args()
    shipped_path = _lib.LIB_PATH
    cands = (SHIPPED,) if a.shipped_only else CANDIDATES
    paths = {c: shipped_path if c == SHIPPED else os.path.join(os.path.dirname(shipped_path), "libcolnde_wmp_%s.so" % c) for c in cands}
    missing = [p for p in paths.values() if not os.path.exists(p)]
    if missing:
        raise SystemExit("missing candidate builds (see this tool's docstring for the make command): %s" % ", ".join(missing))
    import torch
    dev = torch.device("cuda", 0)
    t = lambda x, dt=np.float32: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    p = synthetic.wind_mixing_problem(1, n_frames=3, weight_divisor=1.0)
    cfg, n, Nz = p.cfg, a.n, p.cfg.Nz
    P = cfg.n_params
    rng = np.random.default_rng(32)
    k = np.arange(Nz)
    shear = np.tanh((k - 0.75 * Nz) / (Nz / 8.0))[None, :]
    X = t(np.concatenate([rng.uniform(0.2, 1.0, (n, 1)) * shear + 0.05 * rng.standard_normal((n, Nz)), rng.uniform(0.2, 1.0, (n, 1)) * shear +
                          0.05 * rng.standard_normal((n, Nz)), np.linspace(-1.5, 1.5, Nz)[None, :] + 0.05 * rng.standard_normal((n, Nz))], axis=1))
    B = t(np.tile(p.bcs[:1], (n, 1)) * rng.uniform(0.5, 1.5, (n, 6)))
    Y = t(0.3 * rng.standard_normal((3, n, Nz + 1)))

    def weights(K):
        return np.stack([synthetic.perturb_weights(np.random.default_rng(1000 + q), p.weights, 0.05) for q in range(K)])

    out = dict(n_samples=n, Nz=Nz, layer_sizes=list(cfg.layer_sizes), repeats=a.repeats, rows=[])
    # (a) one (model, net) after another on single handles with the models' constants
    Kb = (a.calls + 2) // 3
    W = weights(Kb)
    od = t(rng.permutation(n), np.int32)
    secs, finite = [], True
    engines = [colnde.ColumnNDE(cfg.with_(**dict(zip(colnde.nde.PHYSICS_KEYS, [float(x) for x in PHYS[q % 4]]))), 1) for q in range(min(Kb, 4))]
    try:
        z = lambda: torch.zeros(P, device=dev)
        engines[0].pretrain_flux(0, t(W[0]), z(), z(), X[:64], B[:64], Y[0, :64], None, 1e-4, ADAM(1e-3))
        for _ in range(a.repeats):
            th, m, v = t(W), torch.zeros((Kb, P), device=dev), torch.zeros((Kb, P), device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = [engines[q % len(engines)].pretrain_flux(j, th[q], m[q], v[q], X, B, Y[j], od, 1e-4, ADAM(1e-3)) for q in range(Kb) for j in range(3)]
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
            finite = finite and bool(np.isfinite(losses).all())
    finally:
        for e in engines:
            e.close()
    per_call = min(secs) / (3 * Kb)
    out["single_handle"] = dict(calls=3 * Kb, s_min=round(min(secs), 4), s_median=round(statistics.median(secs), 4), s_per_call=round(per_call, 5),
                                us_per_update=round(per_call / n * 1e6, 3), finite=finite)
    print(json.dumps(out["single_handle"]), flush=True)

    # (b) one ensemble call per K, every candidate
    for K in a.K:
        Wk = weights(K)
        orders = t(np.stack([np.random.default_rng(7000 + c).permutation(n) for c in range(3 * K)]).reshape(K, 3, n), np.int32)
        etas = torch.full((K, 3), 1e-3, device=dev)
        times = {c: [] for c in cands}
        first, same, finite = None, True, True
        ens = {}
        try:
            for c in cands:                                  # one handle per build, each bound to its own library
                _lib._lib, _lib.LIB_PATH = None, paths[c]
                ens[c] = colnde.ColumnNDEEnsemble(cfg, 1, K, physics=PHYS[np.arange(K) % 4])
            z = lambda: torch.zeros((K, P), device=dev)

            def run(c, th, m, v, nn):
                return ens[c].pretrain_fluxes(th, m, v, X[:nn], B[:nn], Y[:, :nn].contiguous(), None if nn < n else orders, 1e-4, etas)

            for c in cands:
                run(c, t(Wk), z(), z(), 64)
            for _ in range(a.repeats):
                for c in cands:
                    th, m, v = t(Wk), z(), z()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    loss = run(c, th, m, v, n)
                    torch.cuda.synchronize()
                    times[c].append(time.perf_counter() - t0)
                    finite = finite and bool(np.isfinite(loss).all() and torch.isfinite(th).all())
                    if first is None:
                        first = (th.clone(), m.clone(), v.clone())
                    same = same and all(torch.equal(x, y) for x, y in zip(first, (th, m, v)))
        finally:
            for e in ens.values():
                e.close()
            _lib._lib, _lib.LIB_PATH = None, shipped_path
        best = min(cands, key=lambda c: min(times[c]))
        t_ship = min(times[SHIPPED])
        row = dict(K=K, workgroups=3 * K, candidates={c: dict(s_min=round(min(times[c]), 4), s_median=round(statistics.median(times[c]), 4)) for c in cands},
                   best=best, shipped=SHIPPED, shipped_s=round(t_ship, 4), single_handle_3K_calls_s=round(per_call * 3 * K, 3),
                   ratio=round(per_call * 3 * K / t_ship, 2), ideal=min(3 * K, 256), all_candidates_same_bits=same, finite=finite)
        row["ratio_over_ideal"] = round(row["ratio"] / row["ideal"], 3)
        print(json.dumps(row), flush=True)
        out["rows"].append(row)
        if not same:
            raise SystemExit("the candidates' theta, m, v differ at K = %d" % K)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
