"""Ensemble rate on the 8-simulation config3 shape (synthetic.wind_mixing_problem(8): 289 frames x 2 RK4 sub-steps): ms per ensemble training
iteration (colnde_ensemble_loss_grad_dev + colnde_ensemble_adam_step_dev) and aggregate model-iterations/s for K models in one handle, with the
per-kernel times of colnde_kernel_time; against the single handle and what a user has without ensembles — K handles, one stream each, enqueued
round-robin from one thread.  A K whose tapes do not fit is recorded as refused.  One JSON object per line on stdout (and to argv[1] if given).
usage: python tools/ensemble_rate.py [out.jsonl] [--iters N]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import colnde
from colnde import synthetic

ITERS = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 10
OUT = next((a for a in sys.argv[1:] if a.endswith(".jsonl")), None)
SC = [1, 1, 1, 5e-3, 5e-3, 5e-3]
KERNELS = ("forward", "adjoint", "dw1", "reduce", "adam")
dev = torch.device("cuda", 0)
p = synthetic.wind_mixing_problem(8)
P = p.cfg.n_params
lines = []


def emit(r):
    print(json.dumps(r), flush=True)
    lines.append(r)


def truth_of():
    with colnde.ColumnNDE(p.cfg, 8) as h:
        h.set_problem(p.x0, p.bcs)
        return h.forward(p.weights_truth)


truth = truth_of()
x0, bcs, tr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p.x0, p.bcs, truth))


def weights(K):
    rng = np.random.default_rng(1)
    return torch.from_numpy((p.weights[None, :] * (1 + 0.05 * rng.standard_normal((K, P)))).astype(np.float32)).to(dev)


def kernel_ms(h, n):
    return {k: round(h.kernel_time(k)[0] / n, 3) for k in KERNELS}


# the single handle: what one model costs today
with colnde.ColumnNDE(p.cfg, 8) as h:
    h.set_problem(x0, bcs, tr)
    w = weights(1)[0].contiguous()
    out = torch.empty(P + 8, device=dev)
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    for _ in range(3):
        h.loss_grad(w, SC, out=out)
        h.adam_step(w, out, m, v, 1e-4, beta_t=(0.9, 0.999))
    torch.cuda.synchronize()
    h.set_profiling(True)
    h.reset_kernel_times()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        h.loss_grad(w, SC, out=out)
        h.adam_step(w, out, m, v, 1e-4, beta_t=(0.9, 0.999))
    torch.cuda.synchronize()
    ms1 = (time.perf_counter() - t0) * 1e3 / ITERS
    emit({"case": "single_handle", "K": 1, "ms_per_iteration": round(ms1, 3), "model_iterations_per_s": round(1e3 / ms1, 2),
          "kernel_ms": kernel_ms(h, ITERS), "plan": h.plan()})

rates = {}
for K in (1, 4, 16, 64, 256):
    try:
        e = colnde.ColumnNDEEnsemble(p.cfg, 8, K)
    except colnde.ColndeError as err:
        emit({"case": "ensemble", "K": K, "refused": str(err)})
        continue
    try:
        e.set_problem(x0, bcs, tr)
        W = weights(K)
        out = torch.empty((K, P + 8), device=dev)
        m, v = torch.zeros((K, P), device=dev), torch.zeros((K, P), device=dev)
        etas = torch.full((K,), 1e-4, device=dev)
        for _ in range(3):
            e.loss_grad(W, SC, out=out)
            e.adam_step(W, out, m, v, etas, beta_t=(0.9, 0.999))
        torch.cuda.synchronize()
        e.set_profiling(True)
        e.reset_kernel_times()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            e.loss_grad(W, SC, out=out)
            e.adam_step(W, out, m, v, etas, beta_t=(0.9, 0.999))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / ITERS
        rates[K] = K * 1e3 / ms
        emit({"case": "ensemble", "K": K, "ms_per_iteration": round(ms, 3), "model_iterations_per_s": round(rates[K], 2),
              "vs_K1_rate": round(rates[K] / rates[1], 2) if 1 in rates else None, "vs_single_handle_ms": round(ms / ms1, 4) if K == 1 else None,
              "kernel_ms": kernel_ms(e, ITERS), "finite": bool(torch.isfinite(out[:, P + 6]).all().item()), "describe": e.describe().split(" | ")[0]})
    finally:
        e.close()

# the baseline without ensembles: K handles, one stream each, enqueued round-robin from one thread (the process's default hardware-queue count)
for K in (4, 16):
    hs, streams, st = [], [], []
    try:
        for k in range(K):
            h = colnde.ColumnNDE(p.cfg, 8)
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                h.set_problem(x0, bcs, tr)
            hs.append(h)
            streams.append(s)
            st.append((weights(K)[k].contiguous(), torch.empty(P + 8, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)))
        torch.cuda.synchronize()

        def round_robin():
            for h, s, (w, out, m, v) in zip(hs, streams, st):
                with torch.cuda.stream(s):
                    h.loss_grad(w, SC, out=out)
                    h.adam_step(w, out, m, v, 1e-4, beta_t=(0.9, 0.999))
        for _ in range(3):
            round_robin()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            round_robin()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / ITERS
        emit({"case": "k_handles_k_streams", "K": K, "ms_per_round": round(ms, 3), "model_iterations_per_s": round(K * 1e3 / ms, 2)})
    finally:
        for h in hs:
            h.close()

if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
