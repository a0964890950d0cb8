"""Tile-ensemble rate (colnde_create_tile_ensemble) on the reference's wide nets at its training shape: 8 and 18 simulations, train_tranges = 1:20:200
(10 save points), 40 RK4 steps per interval (wind_mixing/train_NDE.jl:138-141; the setting of tests/test_gpu_training_parity.py).  Per shape, size,
arithmetic and K: ms per warm training iteration (colnde_ensemble_loss_grad_dev + colnde_ensemble_adam_step_dev) of ONE ensemble handle against K
single handles called one after another in the same process — the only way to run this sweep without the ensemble.  The two are alternated, a host
clock around a synchronised loop, and the spread of the repeats is kept.  The bytes per model come from colnde_describe.  One JSON object per line on
stdout; the list goes to profiles/tile_ens_rate.json (or --out FILE).
usage: python tools/tile_ens_rate.py [--out FILE] [--iters N] [--repeats N] [--K 1,4,16,64] [--shapes a,b] [--sims 8,18] [--ma bf16x3_exact,f32_mfma]"""
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
from colnde.nde import ENGINE_TILE16


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


OUT = arg("--out", os.path.join(ROOT, "profiles", "tile_ens_rate.json"))
ITERS, REPEATS = int(arg("--iters", 2)), int(arg("--repeats", 3))
KS = [int(k) for k in arg("--K", "1,4,16,64").split(",")]
SHAPES = {
    "3x96-400-400-31_swish": dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity")),
    "3x96-400-31_mish": dict(layer_sizes=(96, 400, 31), activations=("mish", "identity")),
}
NAMES = arg("--shapes", ",".join(SHAPES)).split(",")
SIMS = [int(n) for n in arg("--sims", "8,18").split(",")]
MAS = arg("--ma", "bf16x3_exact,f32_mfma").split(",")
SC = [1, 1, 1, 5e-3, 5e-3, 5e-3]
dev = torch.device("cuda", 0)
lines = []


def emit(r):
    print(json.dumps(r), flush=True)
    lines.append(r)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:                      # rewritten after every line: a run that is cut short keeps what it measured
        json.dump(lines, f, indent=1)


def timed(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / ITERS


for name in NAMES:
    for n_sim in SIMS:
        p = synthetic.wind_mixing_problem(n_sim, n_frames=10, frame_stride=20, substeps=40, weight_divisor=1e2, **SHAPES[name])
        P = p.cfg.n_params
        with colnde.ColumnNDE(p.cfg, n_sim, engine=ENGINE_TILE16) as h:
            h.set_problem(p.x0, p.bcs)
            truth = h.forward(p.weights_truth)
        x0, bcs, tr = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p.x0, p.bcs, truth))
        for ma in MAS:
            for K in KS:
                rng = np.random.default_rng(1)
                W0 = (p.weights[None, :] * (1 + 0.05 * rng.standard_normal((K, P)))).astype(np.float32)
                rec = {"shape": name, "simulations": n_sim, "matrix_arithmetic": ma, "K": K, "steps": 9 * 40, "iters": ITERS}
                try:
                    e = colnde.TileNDEEnsemble(p.cfg, n_sim, K, matrix_arithmetic=ma)
                except colnde.ColndeError as err:
                    emit(dict(rec, refused=str(err)))
                    continue
                hs = []
                try:
                    e.set_problem(x0, bcs, tr)
                    W = torch.from_numpy(W0).to(dev)
                    out = torch.empty((K, P + 8), device=dev)
                    m, v = torch.zeros((K, P), device=dev), torch.zeros((K, P), device=dev)
                    etas = torch.full((K,), 1e-4, device=dev)
                    st = []
                    for k in range(K):
                        h = colnde.ColumnNDE(p.cfg, n_sim, engine=ENGINE_TILE16, matrix_arithmetic=ma)
                        h.set_problem(x0, bcs, tr)
                        hs.append(h)
                        st.append((torch.from_numpy(W0[k]).to(dev), torch.empty(P + 8, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)))

                    def ens_step():
                        e.loss_grad(W, SC, out=out)
                        e.adam_step(W, out, m, v, etas, beta_t=(0.9, 0.999))

                    def seq_step():
                        for h, (w, o, mm, vv) in zip(hs, st):
                            h.loss_grad(w, SC, out=o)
                            h.adam_step(w, o, mm, vv, 1e-4, beta_t=(0.9, 0.999))

                    ens_step()                                    # warm: tapes planned, kernels loaded
                    try:
                        seq_step()
                    except colnde.ColndeError:
                        # K handles' tapes do not fit beside the ensemble's (18 simulations, K = 64): ONE single handle called with the K weight vectors in turn —
                        # the same K sequential calls, each writing and reading its tapes as a handle of its own would
                        for h in hs[1:]:
                            h.close()
                        hs[1:] = []
                        hs = hs * K
                        rec["sequential_handles"] = 1
                        seq_step()
                    ens_ms, seq_ms = [], []
                    for _ in range(REPEATS):                      # alternated
                        ens_ms.append(timed(ens_step))
                        seq_ms.append(timed(seq_step))
                    desc = e.describe().split(" | ")[0]
                    per_model = int(desc.split("tape_bytes_per_model=")[1].split()[0])
                    em, sm = float(np.median(ens_ms)), float(np.median(seq_ms))
                    emit(dict(rec, ensemble_ms=[round(x, 3) for x in ens_ms], sequential_ms=[round(x, 3) for x in seq_ms], ensemble_ms_median=round(em, 3),
                              sequential_ms_median=round(sm, 3), sequential_over_ensemble=round(sm / em, 3), ensemble_faster=bool(max(ens_ms) < min(seq_ms)),
                              model_iterations_per_s=round(K * 1e3 / em, 2), bytes_per_model=per_model,
                              finite=bool(torch.isfinite(out[:, P + 6]).all().item()), describe=desc))
                finally:
                    e.close()
                    for h in {id(h): h for h in hs}.values():
                        h.close()
