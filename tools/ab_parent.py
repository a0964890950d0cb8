"""Unchanged behaviour of the single handle, measured against ANOTHER BUILD of the library loaded in the same process (the parent commit's, built
beside the shipped one: `git worktree` + make, copied to libcolnde_parent.so): colnde_loss_grad_dev on the two 8-simulation free-convection shapes
(16-column kernels) and on the configs[3] shard (16,384 columns x 64 levels: the 32-column kernels), the builds alternating round by round.
Reports per shape the per-round ms of each build, the medians, the parent's own spread (max - min over its rounds) and whether the results are
bit-identical.  The yardstick is the other build, never this one.  One JSON object per line on stdout (and to the .jsonl given).
usage: python tools/ab_parent.py libcolnde_parent.so [libcolnde.so] [out.jsonl] [--rounds N] [--no-shard]"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import colnde
from colnde import _lib, synthetic

PKG = os.path.dirname(_lib.LIB_PATH)
libs = [a for a in sys.argv[1:] if a.endswith(".so")]
if len(libs) == 1:
    libs.append("libcolnde.so")
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 6
OUT = next((a for a in sys.argv[1:] if a.endswith(".jsonl")), None)
SC = [0, 0, 1, 0, 0, 0]
dev = torch.device("cuda", 0)
ALL_SYMBOLS = list(_lib.SYMBOLS)
lines = []


def use(path):
    """Point the binding at one build (an older build lacks the newer symbols: bind what it exports)."""
    full = os.path.join(PKG, path)
    probe = ctypes.CDLL(full)
    _lib.SYMBOLS[:] = [s for s in ALL_SYMBOLS if hasattr(probe, s[0])]
    _lib._lib = None
    _lib.LIB_PATH = full


def emit(r):
    print(json.dumps(r), flush=True)
    lines.append(r)


def report(name, ms, outs):
    a, b = libs
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms[a]) - min(ms[a])
    emit({"shape": name, "rounds": ROUNDS, "ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
          "median_difference_ms": round(med[b] - med[a], 4), "parent_spread_ms": round(spread, 4), "inside_parent_spread": abs(med[b] - med[a]) <= spread,
          "bit_identical": bool(torch.equal(outs[a], outs[b]))})


# the two 8-simulation shapes: both builds' handles alive, alternating
for Nz in (32, 64):
    p = synthetic.free_convection_problem(8, Nz=Nz)
    P = p.cfg.n_params
    x0, bcs, w, wt = (torch.from_numpy(a).to(dev) for a in (p.x0, p.bcs, p.weights, p.weights_truth))
    hs, outs = {}, {}
    for path in libs:
        use(path)
        h = colnde.ColumnNDE(p.cfg, 8)
        h.set_problem(x0, bcs)
        truth = h.forward(wt)
        h.set_problem(x0, bcs, truth)
        outs[path] = torch.empty(P + 8, device=dev)
        for _ in range(3):
            h.loss_grad(w, SC, out=outs[path])
        hs[path] = h
    torch.cuda.synchronize()
    ms = {path: [] for path in libs}
    for rnd in range(ROUNDS):
        for path in (libs if rnd % 2 == 0 else libs[::-1]):
            h = hs[path]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                h.loss_grad(w, SC, out=outs[path])
            torch.cuda.synchronize()
            ms[path].append((time.perf_counter() - t0) * 1e3 / 10)
    report("free_convection_8_simulations_%d_levels" % Nz, ms, outs)
    for h in hs.values():
        h.close()

# the configs[3] shard: one handle at a time (its tapes take most of the memory)
if "--no-shard" not in sys.argv:
    p = synthetic.free_convection_problem(16384, Nz=64)
    P = p.cfg.n_params
    x0, bcs, w, wt = (torch.from_numpy(a).to(dev) for a in (p.x0, p.bcs, p.weights, p.weights_truth))
    ms, outs, truth = {path: [] for path in libs}, {}, None
    for rnd in range(ROUNDS):
        for path in (libs if rnd % 2 == 0 else libs[::-1]):
            use(path)
            h = colnde.ColumnNDE(p.cfg, 16384)
            h.set_problem(x0, bcs)
            if truth is None:
                truth = h.forward(wt)
            h.set_problem(x0, bcs, truth)
            out = torch.empty(P + 8, device=dev)
            h.loss_grad(w, SC, out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.loss_grad(w, SC, out=out)
            torch.cuda.synchronize()
            ms[path].append((time.perf_counter() - t0) * 1e3)
            outs[path] = out
            h.close()
            del h
            torch.cuda.empty_cache()
    report("config4_shard_16384x64", ms, outs)

if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
