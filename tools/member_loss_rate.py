#!/usr/bin/env python
"""What the member loss costs: one `loss_grad` of an ensemble under a member loss against the shared-scalings call, same build, same handle.

Wind mixing: K = 64 members on 8 simulations x 289 frames (the sweep shape of tools/ensemble_rate.py).  Free convection (fc32): K = 64 networks on the
reference's nine simulations, 32 and 64 levels.  Per case one ensemble handle; the member loss is interleaved 0/1 masks (member k trains on the
simulations c with (c + k) % 3 != 0) and per-member scalings.  Kernel milliseconds of one call (forward with tapes + adjoint + dW GEMM + reduction) from
the library's HIP events (`colnde_kernel_time`), `--repeats` calls after `--warmup`, the two calls alternating; median, min and max.  Writes one JSON
object (stdout and --out).

    python tools/member_loss_rate.py --out profiles/member_loss_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("forward", "adjoint", "dw1", "reduce")


def measure(ens, W, shared_sc, scalings, cw, warmup, repeats):
    import torch
    K, P = W.shape
    out = torch.empty((K, P + 8), dtype=torch.float32, device=W.device)
    ens.set_member_loss(scalings, cw)
    ens.set_profiling(True)
    calls = dict(shared=lambda: ens.loss_grad(W, shared_sc, out=out), member=lambda: ens.member_loss_grad(W, out=out))
    for _ in range(warmup):
        for c in calls.values():
            c()
    torch.cuda.synchronize()
    ms = {n: {k: [] for k in KERNELS + ("total",)} for n in calls}
    for r in range(repeats):
        for n in (("shared", "member") if r % 2 == 0 else ("member", "shared")):
            ens.reset_kernel_times()
            calls[n]()
            torch.cuda.synchronize()
            t = {k: ens.kernel_time(k)[0] for k in KERNELS}
            for k in KERNELS:
                ms[n][k].append(t[k])
            ms[n]["total"].append(sum(t.values()))
    st = {n: {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in d.items()} for n, d in ms.items()}
    st["member_over_shared"] = {k: st["member"][k]["median"] / st["shared"][k]["median"] for k in ("adjoint", "total")}
    st["describe"] = ens.describe()
    return st


def masks(K, n):
    cw = np.array([[0.0 if (c + k) % 3 == 0 else 1.0 for c in range(n)] for k in range(K)], np.float32)
    return cw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=64)
    ap.add_argument("--frames", type=int, default=289)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    K = a.models
    res = dict(models=K, repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0))
    rng = np.random.default_rng(0)
    # ---- wind mixing: 8 simulations x 289 frames
    n = 8
    p = synthetic.wind_mixing_problem(n, n_frames=a.frames, weight_divisor=1e2)
    W = torch.as_tensor(np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 1e2) for k in range(K)]).astype(np.float32)).to(dev)
    sc = np.tile(np.array([1, 1, 1, 5e-3, 5e-3, 5e-3], np.float32), (K, 1)) * rng.uniform(0.5, 2.0, (K, 6)).astype(np.float32)
    with colnde.ColumnNDEEnsemble(p.cfg, n, K) as ens:
        x0, bcs, wt = (torch.as_tensor(v).to(dev) for v in (p.x0, p.bcs, p.weights_truth))
        ens.set_problem(x0, bcs)
        truth = ens.forward(wt[None].repeat(K, 1))[0].contiguous()
        ens.set_problem(x0, bcs, truth)
        res["wind_mixing"] = dict(simulations=n, frames=a.frames, **measure(ens, W, [1, 1, 1, 5e-3, 5e-3, 5e-3], sc, masks(K, n), a.warmup, a.repeats))
    # ---- free convection: the reference's nine simulations, 32 and 64 levels
    n = 9
    for Nz in (32, 64):
        p = synthetic.free_convection_problem(n, Nz=Nz, n_save=a.frames, substeps=2, t_end=0.01 * (a.frames - 1) / 4)
        W = torch.as_tensor(np.stack([synthetic.make_weights(synthetic._rng(11, k), p.cfg, 1e2) for k in range(K)]).astype(np.float32)).to(dev)
        sc = np.zeros((K, 6), np.float32)
        sc[:, 2] = rng.uniform(0.5, 2.0, K)
        with colnde.FreeConvectionEnsemble(p.cfg, n, K) as ens:
            x0, bcs, wt = (torch.as_tensor(v).to(dev) for v in (p.x0, p.bcs, p.weights_truth))
            ens.set_problem(x0, bcs)
            truth = ens.forward(wt[None].repeat(K, 1))[0].contiguous()
            ens.set_problem(x0, bcs, truth)
            res["free_convection_%d" % Nz] = dict(simulations=n, frames=a.frames, **measure(ens, W, [0, 0, 1, 0, 0, 0], sc, masks(K, n), a.warmup, a.repeats))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
