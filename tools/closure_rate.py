#!/usr/bin/env python
"""Rate of the closure-only engine (colnde_create_closure) at the reference's calibration shape: 8 simulations x 289 frames x 2 sub-steps.

Milliseconds per `loss_grad` (forward solve with tape + adjoint + reduction, one launch each for all K sets) for K in 1, 16, 64, 256, 1024, the
aggregate set-iterations/s relative to K = 1, and the K = 1 forward solve against `ColumnNDE.forward` with theta = 0 on the same 8 columns (that path
evaluates three MLPs per stage on top of the same closure, so the closure solve must not be slower).  One JSON line per measurement on stdout and,
with --out, appended to a file.  Timing: torch.cuda events around `--iters` back-to-back calls after `--warmup` calls, median of `--repeats`.

    python tools/closure_rate.py --out profiles/closure_rate.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, iters, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--frames", type=int, default=289)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    p = synthetic.wind_mixing_problem(a.columns, n_frames=a.frames, substeps=2)
    dev = torch.device("cuda", 0)
    x0, bcs = torch.as_tensor(p.x0).to(dev), torch.as_tensor(p.bcs).to(dev)
    base = np.array([p.cfg.nu0, p.cfg.nu_minus, p.cfg.dRi, p.cfg.Ric, p.cfg.Pr], np.float32)
    sc = [1, 1, 1, 5e-3, 5e-3, 5e-3]
    lines = []

    def emit(**kw):
        kw.update(columns=a.columns, frames=a.frames, substeps=p.cfg.substeps, device=torch.cuda.get_device_name(0))
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    with colnde.ClosureColumns(p.cfg, a.columns, 1) as one:          # truth: the solve of a set 30 % away
        one.set_problem(x0, bcs)
        truth = one.forward(torch.as_tensor(base[None] * np.float32(1.3)).to(dev))[0].contiguous()
    with colnde.ColumnNDE(p.cfg, a.columns) as nde:
        nde.set_problem(x0, bcs, truth)
        w0 = torch.zeros(p.cfg.n_params, dtype=torch.float32, device=dev)
        sol = torch.empty((a.columns, p.cfg.n_save, p.cfg.n_state), dtype=torch.float32, device=dev)
        med, lo, hi = timed(lambda: nde.forward(w0, out=sol), a.warmup, a.iters, a.repeats)
        emit(what="network_engine_forward_theta0", ms=med, ms_min=lo, ms_max=hi, describe=nde.describe())
    ms1 = None
    rng = np.random.default_rng(0)
    for K in a.sets:
        prm = torch.as_tensor((base[None] * rng.uniform(0.8, 1.0, size=(K, 5))).astype(np.float32)).to(dev).contiguous()
        with colnde.ClosureColumns(p.cfg, a.columns, K) as eng:
            eng.set_problem(x0, bcs, truth)
            out = torch.empty((K, 13), dtype=torch.float32, device=dev)
            sol = torch.empty((K, a.columns, p.cfg.n_save, p.cfg.n_state), dtype=torch.float32, device=dev)
            f_med, f_lo, f_hi = timed(lambda: eng.forward(prm, out=sol), a.warmup, a.iters, a.repeats)
            med, lo, hi = timed(lambda: eng.loss_grad(prm, sc, out=out), a.warmup, a.iters, a.repeats)
            assert bool(torch.isfinite(out).all())
            if ms1 is None:
                ms1 = med / K
            emit(what="closure", sets=K, forward_ms=f_med, forward_ms_min=f_lo, forward_ms_max=f_hi, loss_grad_ms=med, loss_grad_ms_min=lo,
                 loss_grad_ms_max=hi, set_iterations_per_s=1e3 * K / med, ratio_to_first=ms1 / (med / K), describe=eng.describe())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
