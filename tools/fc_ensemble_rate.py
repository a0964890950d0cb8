"""Free-convection ensemble rate on the two 8-simulation shapes bench.py --full times (synthetic.free_convection_problem(8, Nz): 129 save points x 4 RK4
sub-steps, Nz = 32 and 64): ms per ensemble training iteration (colnde_ensemble_loss_grad_dev + colnde_ensemble_adam_step_dev) and aggregate
model-iterations/s for K networks in one colnde_create_fc_ensemble handle, with the per-kernel times of colnde_kernel_time and the bytes per model;
against the single handle and what a user has without ensembles — 16 handles, one stream each, enqueued round-robin from one thread.  A K whose
tapes do not fit is recorded as refused.  One JSON object per line on stdout (and to argv[1] if given).
usage: python tools/fc_ensemble_rate.py [out.jsonl] [--iters N] [--warmup N]"""
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
WARMUP = int(sys.argv[sys.argv.index("--warmup") + 1]) if "--warmup" in sys.argv else 3
OUT = next((a for a in sys.argv[1:] if a.endswith(".jsonl")), None)
SC = [0, 0, 1, 0, 0, 0]
KERNELS = ("forward", "adjoint", "dw1", "reduce", "adam")
dev = torch.device("cuda", 0)
lines = []


def emit(r):
    print(json.dumps(r), flush=True)
    lines.append(r)


def kernel_ms(h, n):
    return {k: round(h.kernel_time(k)[0] / n, 3) for k in KERNELS}


def timed(step):
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ITERS


for Nz in (32, 64):
    p = synthetic.free_convection_problem(8, Nz=Nz)
    P = p.cfg.n_params
    with colnde.ColumnNDE(p.cfg, 8) as h:
        h.set_problem(p.x0, p.bcs)
        truth = h.forward(p.weights_truth)
    x0, bcs, tr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p.x0, p.bcs, truth))

    def weights(K):
        rng = np.random.default_rng(1)
        return torch.from_numpy((p.weights[None, :] * (1 + 0.05 * rng.standard_normal((K, P)))).astype(np.float32)).to(dev)

    # the single handle: what one network costs today
    with colnde.ColumnNDE(p.cfg, 8) as h:
        h.set_problem(x0, bcs, tr)
        w = weights(1)[0].contiguous()
        out = torch.empty(P + 8, device=dev)
        m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)

        def step():
            h.loss_grad(w, SC, out=out)
            h.adam_step(w, out, m, v, 1e-4, beta_t=(0.9, 0.999))
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize()
        h.set_profiling(True)
        h.reset_kernel_times()
        t0 = time.perf_counter()
        for _ in range(ITERS):
            step()
        torch.cuda.synchronize()
        ms1 = (time.perf_counter() - t0) * 1e3 / ITERS
        emit({"case": "single_handle", "Nz": Nz, "K": 1, "ms_per_iteration": round(ms1, 3), "model_iterations_per_s": round(1e3 / ms1, 2),
              "kernel_ms": kernel_ms(h, ITERS), "plan": h.plan()})

    rates = {}
    for K in (1, 4, 16, 64, 256):
        try:
            e = colnde.FreeConvectionEnsemble(p.cfg, 8, K)
        except colnde.ColndeError as err:
            emit({"case": "ensemble", "Nz": Nz, "K": K, "refused": str(err)})
            continue
        try:
            e.set_problem(x0, bcs, tr)
            W = weights(K)
            out = torch.empty((K, P + 8), device=dev)
            m, v = torch.zeros((K, P), device=dev), torch.zeros((K, P), device=dev)
            etas = torch.full((K,), 1e-4, device=dev)

            def step():
                e.loss_grad(W, SC, out=out)
                e.adam_step(W, out, m, v, etas, beta_t=(0.9, 0.999))
            for _ in range(WARMUP):
                step()
            torch.cuda.synchronize()
            e.set_profiling(True)
            e.reset_kernel_times()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ITERS
            rates[K] = K * 1e3 / ms
            desc = e.describe().split(" | ")[0]
            emit({"case": "ensemble", "Nz": Nz, "K": K, "ms_per_iteration": round(ms, 3), "model_iterations_per_s": round(rates[K], 2),
                  "vs_K1_rate": round(rates[K] / rates[1], 2) if 1 in rates else None, "vs_single_handle_ms": round(ms / ms1, 4) if K == 1 else None,
                  "kernel_ms": kernel_ms(e, ITERS), "finite": bool(torch.isfinite(out[:, P + 6]).all().item()),
                  "bytes_per_model": int(desc.split("tape_bytes_per_model=")[1].split()[0]), "describe": desc})
        finally:
            e.close()
        del W, out, m, v
        torch.cuda.empty_cache()

    # the largest K whose tapes fit beside what this process holds: the per-model bytes against the free memory (3 GB kept in reserve)
    if 1 in rates:
        per_model = next(r["bytes_per_model"] for r in lines if r.get("case") == "ensemble" and r.get("Nz") == Nz and "bytes_per_model" in r)
        free_b, total_b = torch.cuda.mem_get_info(dev)
        emit({"case": "memory", "Nz": Nz, "bytes_per_model": per_model, "free_bytes": int(free_b), "total_bytes": int(total_b),
              "largest_K_that_fits": int(min(65535, max(0, free_b - (3 << 30)) // per_model))})

    # the baseline without ensembles: 16 handles, one stream each, enqueued round-robin from one thread
    K = 16
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
        ms = timed(round_robin)
        emit({"case": "k_handles_k_streams", "Nz": Nz, "K": K, "ms_per_round": round(ms, 3), "model_iterations_per_s": round(K * 1e3 / ms, 2)})
    finally:
        for h in hs:
            h.close()

if OUT:
    with open(OUT, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")
