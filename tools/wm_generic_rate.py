#!/usr/bin/env python
"""Rate of the generic wind-mixing embedding kernel (csrc/engine_wm_embed_any.hip): `colnde_ensemble_wm_embedded_dev` on a single handle of
3 x 96-400-400-31 and 3 x 96-400-31 — forcing only, with the implicit step, with step and faces — beside the only device path these nets had before,
`colnde_flux_dev` (tile16's rhs_kernel on the same three nets and columns; its pack launch is outside the timed slot), plus the unchanged
`colnde_implicit_diffusion_dev`.  For information: 96-50-20-31 under COLNDE_WM_GENERIC=1 against the persistent kernel.

The method of tools/wm_infer_rate.py: HIP-event time of each kernel through `colnde_kernel_time` (warm; `--reps` launches, mean per launch).  Writes one
JSON document.

    python tools/wm_generic_rate.py --out profiles/wm_generic_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MPP = (1e-4, 1e-1, 1.0, 0.25, 1.0, 1.67e-4, 9.81)
SHAPES = {"96-400-400-31": ((96, 400, 400, 31), ("swish", "swish", "identity")), "96-400-31": ((96, 400, 31), ("relu", "identity"))}


def timed(nde, slot, fn, warmup, reps):
    import torch
    nde.set_profiling(False)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    nde.reset_kernel_times()
    nde.set_profiling(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, launches = nde.kernel_time(slot)
    nde.set_profiling(False)
    assert launches == reps, (slot, launches)
    return ms / launches


def state(base, n, dev):
    import torch
    mu, sg = base.cfg.mu, base.cfg.sigma
    rep = (n + base.x0.shape[0] - 1) // base.x0.shape[0]
    x0 = torch.from_numpy(base.x0).to(dev).repeat(rep, 1)[:n].contiguous()
    u, v, T = ((sg[f] * x0[:, 32 * f:32 * f + 32] + mu[f]).contiguous() for f in range(3))
    bcs = torch.from_numpy(base.bcs.astype(np.float32)).to(dev).repeat(rep, 1)[:n].contiguous()
    top = torch.stack([sg[3 + k] * bcs[:, 1 + 2 * k] + mu[3 + k] for k in range(3)]).contiguous()
    return x0, bcs, u, v, T, top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 18, 200, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import colnde
    from colnde import synthetic
    dev = torch.device("cuda", 0)
    params = np.float32(MPP)[None]
    doc = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, results=[])
    for name, (sizes, acts) in SHAPES.items():
        base = synthetic.wind_mixing_problem(4096, n_frames=3, weight_divisor=1.0, layer_sizes=sizes, activations=acts)
        with colnde.ColumnNDE(base.cfg, 4) as nde:
            doc.setdefault("describe", {})[name] = nde.describe()
            w = torch.from_numpy(base.weights_truth).to(dev)
            for n in a.columns:
                x0, bcs, u, v, T, top = state(base, n, dev)
                emb = lambda **kw: nde.wm_embedded(w[None], u[None], v[None], T[None], top, 256.0, 60.0 if kw.get("step") else None, params, True, **kw)
                row = dict(shape=name, columns=n)
                row["forcing_ms"] = timed(nde, "flux_diag", lambda: emb(step=False, flux=False), a.warmup, a.reps)
                row["step_ms"] = timed(nde, "flux_diag", lambda: emb(step=True, flux=False), a.warmup, a.reps)
                row["step_faces_ms"] = timed(nde, "flux_diag", lambda: emb(step=True, flux=True), a.warmup, a.reps)
                row["flux_dev_ms"] = timed(nde, "rhs", lambda: nde.flux(x0, w, bcs), a.warmup, a.reps)
                row["implicit_diffusion_ms"] = timed(nde, "impldiff", lambda: nde.implicit_diffusion(u, v, T, 60.0, 8.0, MPP, True), a.warmup, a.reps)
                row["two_launches_ms"] = row["flux_dev_ms"] + row["implicit_diffusion_ms"]
                row["forcing_below_flux_dev"] = row["forcing_ms"] < row["flux_dev_ms"]
                row["step_below_two_launches"] = row["step_ms"] < row["two_launches_ms"]
                doc["results"].append(row)
                print(json.dumps(row), flush=True)
    # for information: the one shape both kernels serve
    base = synthetic.wind_mixing_problem(4096, n_frames=3, weight_divisor=1.0)
    with colnde.ColumnNDE(base.cfg, 4) as nde:
        w = torch.from_numpy(base.weights_truth).to(dev)
        x0, bcs, u, v, T, top = state(base, 18, dev)
        row = dict(shape="96-50-20-31", columns=18)
        for label, env in (("persistent", None), ("generic", "1")):
            os.environ.pop("COLNDE_WM_GENERIC", None)
            if env:
                os.environ["COLNDE_WM_GENERIC"] = env
            for what, kw in (("forcing_ms", dict(step=False, flux=False)), ("step_faces_ms", dict(step=True, flux=True))):
                fn = lambda: nde.wm_embedded(w[None], u[None], v[None], T[None], top, 256.0, 60.0 if kw["step"] else None, params, True, **kw)
                row[label + "_" + what] = timed(nde, "flux_diag", fn, a.warmup, a.reps)
        os.environ.pop("COLNDE_WM_GENERIC", None)
        doc["results"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
