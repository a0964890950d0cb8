"""Seconds per pass of the T -> wT pre-training (train_free_convection_nde.jl:182-216: one optimiser update per sample) for a sweep of K networks, on the
reference's data-set size — n = 10,377 samples (9 simulations x 1,153 frames), one ADAM pass, Nz = 32 and 64, synthetic samples:
  (a) K back-to-back `colnde_pretrain_flux_dev` calls on a single handle, each model with its own weights and moments (that kernel's one workgroup per
      call is what a sweep had before the ensemble call; --calls K, default 64)
  (b) one `colnde_ensemble_pretrain_flux_dev` call at K = 64
  (c) one at K = 256
and, for the `--conv 3` network (no single-handle call exists for it), one ensemble call at K = 1 and at K = 64.  Every call synchronises its stream, so
wall-clock time around the calls is the time of the launches; a short warm-up call (64 samples) precedes each timing.  The single-model microseconds per
update are recorded too: the serial chain's cost, the starting point of any later change to it.
    python tools/fc_pretrain_rate.py [--out profiles/fc_pretrain_ens_rate.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np

import colnde
from colnde import synthetic
from colnde.flux_compat import ADAM
from colnde.nde import fc_ensemble_n_params


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fc_pretrain_ens_rate.json")
    ap.add_argument("--n", type=int, default=9 * 1153)
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--Nz", type=int, nargs="+", default=[32, 64])
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    t = lambda x, dt=np.float32: torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).to(dev)
    rows = []
    for Nz in a.Nz:
        p = synthetic.free_convection_problem(1, Nz=Nz, n_save=3, substeps=2, t_end=0.01, weight_divisor=1.0)
        cfg, n = p.cfg, a.n
        rng = np.random.default_rng(Nz)
        X = t(np.linspace(-1.5, 1.5, Nz)[None, :] + 0.3 * rng.standard_normal((n, Nz)))
        B = t(np.stack([np.zeros(n), rng.uniform(0.1, 1.0, n)], axis=1))
        Y = t(0.3 * rng.standard_normal((n, Nz + 1)))
        order = rng.permutation(n).astype(np.int32)

        def weights(K, conv):
            base = synthetic.free_convection_conv_problem(1, conv, Nz=Nz, n_save=3, substeps=2, weight_divisor=1.0).weights if conv else p.weights
            assert base.shape == (fc_ensemble_n_params(cfg, conv),)
            return np.stack([synthetic.perturb_weights(np.random.default_rng(1000 + k), base, 0.05) for k in range(K)])

        # (a) one model after another on a single handle
        K = a.calls
        W = weights(K, 0)
        with colnde.ColumnNDE(cfg, 1) as eng:
            od = t(order, np.int32)
            th, m, v = t(W), torch.zeros((K, cfg.n_params), device=dev), torch.zeros((K, cfg.n_params), device=dev)
            eng.pretrain_flux(2, th[0].clone(), m[0].clone(), v[0].clone(), X[:64], B[:64], Y[:64], None, 0.0, ADAM(1e-3))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = [eng.pretrain_flux(2, th[k], m[k], v[k], X, B, Y, od, 0.0, ADAM(1e-3)) for k in range(K)]
            torch.cuda.synchronize()
            sec_a = time.perf_counter() - t0
        row = dict(Nz=Nz, conv=0, n_samples=n, optimiser="adam", single_handle_calls=K, single_handle_s=round(sec_a, 4),
                   single_model_s_per_pass=round(sec_a / K, 5), single_model_us_per_update=round(sec_a / K / n * 1e6, 3),
                   finite=bool(np.isfinite(losses).all()))
        print(json.dumps(row), flush=True)

        def ensemble(K, conv):
            Wk = weights(K, conv)
            with colnde.FreeConvectionEnsemble(cfg, 1, K, conv=conv) as ens:
                P = ens.n_params
                orders = t(np.tile(order, (K, 1)), np.int32)
                etas = torch.full((K,), 1e-3, device=dev)
                z = lambda: torch.zeros((K, P), device=dev)
                ens.pretrain_flux(t(Wk), z(), z(), X[:64], B[:64], Y[:64], None, None, "adam", etas)
                th, m, v = t(Wk), z(), z()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loss = ens.pretrain_flux(th, m, v, X, B, Y, orders, None, "adam", etas)
                torch.cuda.synchronize()
                sec = time.perf_counter() - t0
            return sec, bool(np.isfinite(loss).all() and torch.isfinite(th).all())

        for K_e in (64, 256):
            sec, ok = ensemble(K_e, 0)
            row["ensemble_K%d_s" % K_e] = round(sec, 4)
            row["ensemble_K%d_us_per_update_per_model" % K_e] = round(sec / n * 1e6, 3)
            row["finite"] = row["finite"] and ok
            print(json.dumps({"Nz": Nz, "K": K_e, "s": round(sec, 4)}), flush=True)
        row["one_after_another_over_ensemble_K64"] = round(sec_a / K * 64 / row["ensemble_K64_s"], 2)
        row["K256_over_K64"] = round(row["ensemble_K256_s"] / row["ensemble_K64_s"], 3)
        rows.append(row)
        crow = dict(Nz=Nz, conv=3, n_samples=n, optimiser="adam")
        for K_e in (1, 64):
            sec, ok = ensemble(K_e, 3)
            crow["ensemble_K%d_s" % K_e] = round(sec, 4)
            crow["ensemble_K%d_us_per_update_per_model" % K_e] = round(sec / n * 1e6, 3)
            crow["finite"] = crow.get("finite", True) and ok
        crow["K64_over_K1"] = round(crow["ensemble_K64_s"] / crow["ensemble_K1_s"], 3)
        print(json.dumps(crow), flush=True)
        rows.append(crow)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
