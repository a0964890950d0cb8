#!/usr/bin/env python3
"""bench.py — column-timesteps/s (forward + adjoint) of the 32-level wind-mixing NDE on N MI355X GPUs.

One "step" = one pass of the hot path over the resident batch: forward RK4 solve + discrete adjoint +
deterministic gradient reduce for every column of this rank (`colnde_loss_grad_dev`), then — for N > 1 —
one RCCL SUM all-reduce of [grad(19,563); 6 loss terms; total] (the only exchange step).
Columns shard across ranks with no other data-path collective: weak scaling, per-GPU columns fixed.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--columns C] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Rank 0 prints ONE JSON line (metric/unit from BASELINE.json) carrying `roofline` (dominant kernel = the adjoint
kernel, HIP-event timed on its own stream through colnde_kernel_time, from the K timed steps themselves).
A plain run does only what that line needs: set up, W warm-up steps, K timed steps, the line.  `--dump-outputs DIR`
writes what the last timed step computed (DIR/<name>.npy; the inputs are seeded, so two builds compare file for file).
`--full` adds everything else, all after the timed region: the K steps again without kernel events (shader clock,
board power), the device copy bandwidth, the F32_MFMA opt-out, the self-check against the C port, `cpu_baseline`
(the C port of the oracle on the box's host cores, bounded sample, rank 0 at N = 1 only), the other BASELINE
configs, the all-reduce timed alone (N > 1) and the full record on disk.

Matrix arithmetic (include/colnde.h COLNDE_MATRIX_*): the headline runs the library default, BF16X3_EXACT — f32 operands split exactly into
three bf16 parts, six bf16 MFMA products per k-block, f32 accumulation: f32 arithmetic on the bf16 pipe (`dtype` stays "f32"; VERDICT r3 ruling).
With --full the same step under F32_MFMA is measured after the timed region and reported beside it (`opt_out`).  Because the kernels then run a MIX of
bf16 and f32 MFMA instructions, `roofline.frac` is the matrix-pipe TIME fraction (executed bf16-MFMA flop / 2.5 PF + executed f32-MFMA flop /
157.3 TF, over the kernel's duration), never algorithmic flops over the f32 peak; the algorithmic f32-equivalent TFLOP/s is `roofline.achieved`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

# algorithmic figures per column-timestep (stated in DESIGN.md §4/§5): 2·Σ in·out per net, three nets.
# Each kernel is charged only the MLP flops it actually performs (padding, activations and physics are not counted):
L1, L2, L3 = 2 * 3 * 96 * 50, 2 * 3 * 50 * 20, 2 * 3 * 20 * 31      # 28,800 / 6,000 / 3,720 flop per RHS
MLP_FLOP_PER_RHS = L1 + L2 + L3                                     # 38,520
FWD_FLOP_PER_COLSTEP = 4 * MLP_FLOP_PER_RHS                         # forward kernel: 154,080
# adjoint pass per stage = dX (38,520) + dW (38,520) + whatever forward state is recomputed rather than taped
ADJ_FLOP_REGTILE = 4 * (MLP_FLOP_PER_RHS + (L2 + L3) + L2)          # rt_adjoint_kernel with Z1 taped: dX + dW2/dW3 + layer-2 recompute = 216,960
ADJ_FLOP_REGTILE_NOZ = ADJ_FLOP_REGTILE + 4 * L1                    # ... recomputing layer 1 as well: 332,160
DW1_FLOP_PER_COLSTEP = 4 * L1                                       # rt_dw1_kernel: 115,200
ADJ_FLOP_TILE16 = 4 * 3 * MLP_FLOP_PER_RHS                          # tile16 adjoint_kernel: recompute + dX + dW = 462,240 (SURVEY's "3x forward")
PEAK_FP32_MFMA_TFLOPS = 157.3                                      # MI355X_MICROARCH.md: FP32 matrix, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0                                     # ... BF16 matrix, dense (never the 2:1-sparsity figure)
PEAK_HBM_GBPS = 8000.0
HBM_ACHIEVABLE_GBPS = 6290.0                                       # ... measured float4 copy (79 % of the spec figure)
# MFMA instructions EXECUTED per 32-column stage by the regtile kernels (counted in the ISA of the shipped build: tools/loop_mix.py on
# `make -C csrc asm`; padding rows and the k-slots a 16-deep bf16 block leaves empty are executed work, not algorithmic work):
#   kernel: {matrix arithmetic: (bf16 MFMA flop, f32 MFMA flop)}; v_mfma_f32_32x32x16_bf16 = 32,768 flop, 16x16x32_bf16 = 16,384,
#   v_mfma_f32_32x32x2_f32 = 4,096, 16x16x4_f32 = 2,048
EXECUTED_MFMA_FLOP_PER_STAGE32 = {
    "forward": {"bf16x3_exact": (2 * 288 * 16384, 0), "f32_mfma": (0, 2 * 348 * 2048)},        # rt16_forward_kernel: two 16-column tiles
    "adjoint": {"bf16x3_exact": (162 * 32768, 336 * 4096), "f32_mfma": (0, 552 * 4096)},       # rt_adjoint_kernel<ACT, true[, true]>
    "dw1": {"bf16x3_exact": (180 * 32768, 0), "f32_mfma": (0, 240 * 4096)},                    # rt_dw1[_split]_kernel
}


DUMP_BUDGET_BYTES = 60 << 20                                       # --dump-outputs: all arrays of one run together (with the .npy headers below 64 MB)


def dump_outputs(dirname, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: the arrays the timed path handed its caller in the last timed step, one DIR/<name>.npy each, float32.  When they
    exceed `budget` bytes together, each keeps a fixed seeded sample of its elements (flattened, in index order) and the flat indices of
    that sample go beside it as DIR/<name>_index.npy (float64), so the sample is the same from run to run."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > budget:
            # 4 bytes of value + 8 of index per kept element; one element per array is set aside so that every array keeps at least one
            k = min(a.size, 1 + ((budget - 12 * len(arrays)) * a.nbytes // total) // 12)
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=k, replace=False))
            np.save(os.path.join(dirname, name + "_index.npy"), idx.astype(np.float64))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


def pipe_time_fraction(kernel, arithmetic, stages32, seconds):
    """Matrix-pipe time of the MFMA instructions a kernel executes, as a fraction of its duration: bf16 flop / 2.5 PF + f32 flop / 157.3 TF."""
    bf, f32 = EXECUTED_MFMA_FLOP_PER_STAGE32[kernel][arithmetic]
    return (stages32 * bf / (PEAK_BF16_MFMA_TFLOPS * 1e12) + stages32 * f32 / (PEAK_FP32_MFMA_TFLOPS * 1e12)) / seconds if seconds > 0 else None


class GpuSensors:
    """Shader clock and board power of THIS rank's GPU, read from the amdgpu sysfs nodes (hwmon freq1_input / power1_input of the PCI device
    torch reports) by a host thread every 20 ms while a loop runs.  Round 4 found the training steps POWER-limited on MI355X (about 1.3 kW, the
    shader clock at 2.0-2.2 GHz instead of 2.4): every roofline fraction in this line is quoted against the 2.4 GHz peaks, and this block says
    what the clock really was.  Never inside the timed region that produces `value`; None when the nodes are not readable."""

    def __init__(self, dev):
        import glob
        import threading
        self.samples, self._stop, self._thread, self.dir = [], False, None, None
        self._threading = threading
        try:
            import torch
            pr = torch.cuda.get_device_properties(dev)
            bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            hw = glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bdf)
            if hw and os.path.exists(os.path.join(hw[0], "freq1_input")):
                self.dir = hw[0]
        except Exception:
            self.dir = None

    def _read(self, name):
        try:
            return float(open(os.path.join(self.dir, name)).read())
        except Exception:
            return None

    def _run(self):
        while not self._stop:
            f, pw = self._read("freq1_input"), self._read("power1_input")
            if pw is None:
                pw = self._read("power1_average")
            self.samples.append((f, pw))
            time.sleep(0.02)

    def start(self):
        if self.dir is not None:
            self._thread = self._threading.Thread(target=self._run, daemon=True)
            self._thread.start()
        return self

    def stop(self):
        if self._thread is None:
            return None
        self._stop = True
        self._thread.join()
        fs = [f / 1e6 for f, _ in self.samples if f]
        ps = [pw / 1e6 for _, pw in self.samples if pw]
        if not fs:
            return None
        return {"shader_clock_MHz_mean": sum(fs) / len(fs), "shader_clock_MHz_min": min(fs), "shader_clock_MHz_max": max(fs),
                "board_power_W_mean": (sum(ps) / len(ps)) if ps else None, "board_power_cap_W": (self._read("power1_cap") or 0) / 1e6 or None,
                "samples": len(fs), "peak_clock_MHz_the_rooflines_assume": 2400,
                "source": self.dir, "sampled_over": "the second (untimed-for-value) pass of the same K steps"}


def measured_copy_bandwidth(dev, gib=4):
    """One device-to-device copy of `gib` GiB, outside every timed region: bytes read + bytes written per second (SURVEY §8d asks for the HBM
    fraction against a copy bandwidth measured on the box beside the vendor figure)."""
    import torch
    n = gib * (1 << 30) // 4
    try:
        src = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3):
            dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        return 3 * 2 * n * 4 / (a.elapsed_time(b) * 1e-3) / 1e9
    except Exception:
        return None
    finally:
        src = dst = None
        torch.cuda.empty_cache()


def reference_probe():
    """Is the reference's own path runnable on this box?  Looked for at run time: a `julia` on PATH.  (Even with one, the
    387 pinned packages of wind_mixing/Manifest.toml would have to be in a depot on the box: there is no network.)"""
    import shutil
    exe = shutil.which("julia")
    if exe is None:
        return {"julia": None, "note": "no `julia` on PATH (shutil.which): the reference's DiffEqFlux path cannot be timed on this box"}
    import subprocess
    try:
        ver = subprocess.run([exe, "--version"], capture_output=True, text=True, timeout=60).stdout.strip()
    except Exception as e:
        ver = "not runnable: %s" % e
    depot = os.path.expanduser("~/.julia")
    return {"julia": exe, "version": ver, "depot_present": os.path.isdir(depot),
            "note": "a julia binary is present; the reference environment (wind_mixing/Manifest.toml) is not shipped to the GPU box, so its path is still not timed here"}


def algorithmic_bytes_per_colstep(Nz, substeps):
    bx = 4 * 3 * Nz
    return dict(forward=bx / substeps, adjoint=2 * bx / substeps, total=3 * bx / substeps)


def cpu_baseline(problem, scalings, budget_s=20.0):
    """Time oracle/colnde_ref.c (float32 port of the oracle) on the host cores: same workload shape, bounded sample."""
    from oracle import cref
    cfg = problem.cfg
    # the GPU box's CPU share for one GPU is 16 cores (more threads only oversubscribe the cgroup)
    threads = max(1, min(os.cpu_count() or 1, len(os.sched_getaffinity(0)), 16))
    steps = cfg.n_steps
    # single thread first: 4 columns
    n1 = 4
    truth1 = cref.forward(cfg, problem.x0[:n1], problem.bcs[:n1], problem.weights_truth, n_threads=1)
    t0 = time.perf_counter()
    cref.loss_grad(cfg, problem.x0[:n1], problem.bcs[:n1], problem.weights, truth1, scalings, n_threads=1)
    t1 = time.perf_counter() - t0
    rate1 = n1 * steps / t1
    # all cores: size the sample for ~budget_s/2 of wall time
    per_col = t1 / n1
    ncol = int(max(threads, min(problem.n_columns, (budget_s / 2) / per_col * threads * 0.5)))
    ncol = max(threads, (ncol // threads) * threads)
    ncol = min(ncol, problem.n_columns)
    truth = cref.forward(cfg, problem.x0[:ncol], problem.bcs[:ncol], problem.weights_truth, n_threads=threads)
    t0 = time.perf_counter()
    cref.loss_grad(cfg, problem.x0[:ncol], problem.bcs[:ncol], problem.weights, truth, scalings, n_threads=threads)
    tn = time.perf_counter() - t0
    return {
        "value": ncol * steps / tn, "unit": "column-timesteps/s", "cores": threads, "kind": "port",
        "sample": "oracle/colnde_ref.c (float32 C port of the oracle, OpenMP over columns): %d columns x %d RK4 steps "
                  "fwd+adjoint of the same workload in %.1f s on %d threads; 1 thread: %d columns in %.1f s = %.0f column-timesteps/s"
                  % (ncol, steps, tn, threads, n1, t1, rate1),
        "value_1thread": rate1, "reference": reference_probe(),
    }


def check_forward_against_port(nde, prob, w, dev, n_sample=8, tol=5e-4):
    """After the timed region: `n_sample` columns of the bench's OWN forward solve (same handle, same weights, strided over the batch) against the
    float32 C port of the oracle over the full horizon.  Returns {max_abs_error, tolerance, columns, ok}; a miss fails the run."""
    import torch
    from oracle import cref
    n = prob.n_columns
    idx = np.unique(np.linspace(0, n - 1, n_sample).astype(np.int64))
    sol = nde.forward(w)
    got = sol[torch.from_numpy(idx).to(dev)].cpu().numpy()
    del sol
    torch.cuda.empty_cache()
    ref = cref.forward(prob.cfg, prob.x0[idx], prob.bcs[idx], w.cpu().numpy(), n_threads=min(len(idx), 8))
    err = float(np.abs(got - ref).max()) if np.isfinite(got).all() else float("inf")
    return {"max_abs_error": err, "tolerance": tol, "columns": [int(i) for i in idx], "ok": bool(err < tol),
            "against": "oracle/colnde_ref.c (float32 C port), full %d-step horizon, scaled units" % prob.cfg.n_steps}


def other_configs(dev, budget_s=120.0):
    """The BASELINE configs other than the headline one, run AFTER the headline's timed region and after its handle has been closed
    (config 4's tapes want most of the HBM): each a short timed loop of the same C-ABI calls, reported with ms per pass,
    column-timesteps/s and its fraction of the roofline that bounds it.  Parity for each of these cases lives in tests/ (-m gpu)."""
    import torch
    import colnde
    from colnde import synthetic
    out = {}
    t_start = time.perf_counter()

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def kernel_ms(nde):
        r = {}
        for k in ("forward", "adjoint", "dw1", "reduce"):
            ms, n = nde.kernel_time(k)
            if n:
                r[k] = ms / n
        return r

    def guarded(name, fn):
        if time.perf_counter() - t_start > budget_s:
            out[name] = {"skipped": "time budget of the configs block spent"}
            return
        try:
            out[name] = fn()
        except Exception as e:                                   # a failing side config must not take the headline line with it
            out[name] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    def grad_case(p, ncol, sc, n_timed, flop_per_rhs, rhs_per_step, label, ma="bf16x3_exact"):
        nde = colnde.ColumnNDE(p.cfg, ncol, matrix_arithmetic=ma)
        try:
            x0, bcs, w, wt = (torch.from_numpy(a).to(dev) for a in (p.x0, p.bcs, p.weights, p.weights_truth))
            nde.set_problem(x0, bcs)
            truth = nde.forward(wt)
            nde.set_problem(x0, bcs, truth)
            res = torch.empty(p.cfg.n_params + 8, device=dev)
            nde.loss_grad(w, sc, out=res)                         # plans and allocates the tapes
            nde.set_profiling(True)
            nde.reset_kernel_times()
            dt = timed(lambda: nde.loss_grad(w, sc, out=res), n_timed)
            km = kernel_ms(nde)
            cs = ncol * p.cfg.n_steps
            flop = 3 * rhs_per_step * flop_per_rhs                # forward + adjoint (dX, dW) per column-timestep: SURVEY §8d "3x forward"
            bx = 4 * p.cfg.n_state
            r = {"workload": label, "columns": ncol, "steps": p.cfg.n_steps, "ms": dt * 1e3, "column_timesteps_per_s": cs / dt,
                 "mfma": {"flop_per_column_timestep": flop, "achieved_TFLOPs": cs * flop / dt / 1e12,
                          "of_f32_mfma_peak": cs * flop / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                          "note": "algorithmic f32-equivalent flops over the f32 MFMA peak: a fraction of a roofline only for kernels that run f32 MFMA "
                                  "(plan.bf16x3_* all false); kernels on the bf16 pipe can exceed 1"},
                 "hbm": {"algorithmic_bytes_per_column_timestep": 3 * bx / p.cfg.substeps,
                         "frac": cs * 3 * bx / p.cfg.substeps / dt / 1e9 / PEAK_HBM_GBPS},
                 "kernel_ms": km, "plan": nde.plan(), "loss_total": float(res[p.cfg.n_params + 6].item())}
            if not np.isfinite(r["loss_total"]):
                r["error"] = "non-finite loss"
            return r
        finally:
            nde.close()

    def c2(ma="bf16x3_exact"):       # BASELINE configs[1]: forward only, 4,096 columns x 32 levels, 288 frames x 2 RK4 sub-steps
        p = synthetic.wind_mixing_problem(4096)
        nde = colnde.ColumnNDE(p.cfg, 4096, matrix_arithmetic=ma)
        try:
            x0, bcs, w = (torch.from_numpy(a).to(dev) for a in (p.x0, p.bcs, p.weights))
            nde.set_problem(x0, bcs)
            sol = nde.forward(w)
            dt = timed(lambda: nde.forward(w, out=sol), 10)
            cs = 4096 * p.cfg.n_steps
            return {"workload": "configs[1]: NDE forward only, 4096 columns x 32 levels x 576 RK4 steps", "columns": 4096, "steps": p.cfg.n_steps,
                    "ms": dt * 1e3, "column_timesteps_per_s": cs / dt,
                    "mfma": {"flop_per_column_timestep": FWD_FLOP_PER_COLSTEP, "achieved_TFLOPs": cs * FWD_FLOP_PER_COLSTEP / dt / 1e12,
                             "of_f32_mfma_peak": cs * FWD_FLOP_PER_COLSTEP / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS},
                    "hbm": {"algorithmic_bytes_per_column_timestep": 384 / p.cfg.substeps, "frac": cs * 384 / p.cfg.substeps / dt / 1e9 / PEAK_HBM_GBPS},
                    "engine": nde.engine, "plan_after_forward": nde.plan()}
        finally:
            nde.close()

    def c3(ma="bf16x3_exact"):       # BASELINE configs[2] as the reference trains it: 8 simulations
        p = synthetic.wind_mixing_problem(8)
        return grad_case(p, 8, [1, 1, 1, 5e-3, 5e-3, 5e-3], 5, MLP_FLOP_PER_RHS, 4,
                         "configs[2] as written: 8 simulations x 32 levels x 289 frames, fwd+adjoint (latency point)", ma)

    def c3ca(ma="bf16x3_exact"):     # the reference's kappa = 10 convective-adjustment branch (NDE_training.jl:140-143; ROCK4 at train_NDE.jl:143) on 8 simulations
        p = synthetic.wind_mixing_problem(8, modified_pacanowski_philander=False, zero_weights=False, convective_adjustment=True, kappa=10.0,
                                          stepper="rkc2", substeps=1)
        s = colnde.rkc_stages(p.cfg)
        r = grad_case(p, 8, [1, 1, 1, 5e-3, 5e-3, 5e-3], 3, MLP_FLOP_PER_RHS, s,
                      "configs[2]'s 8 simulations on the wind-mixing convective-adjustment branch (kappa = 10): 288 RKC2 steps of %d stages "
                      "(sub-stepped RK4 would need %d RHS evaluations per frame), fwd+adjoint" % (s, 4 * colnde.min_substeps(p.cfg.with_(stepper="rk4"))), ma)
        r["rhs_evaluations_per_step"] = s
        return r

    def fc(ncol, Nz, ca, n_timed, label, ma="bf16x3_exact"):
        p = synthetic.free_convection_problem(ncol, Nz=Nz, convective_adjustment=ca)
        rhs_per_step = 4
        if ca:      # ConvectiveAdjustmentNDE is stiff (K = 10): the stabilised RKC2 stepper, automatic stage count
            p.cfg = p.cfg.with_(stepper="rkc2")
            rhs_per_step = colnde.rkc_stages(p.cfg)
        mlp = 2 * (Nz * 4 * Nz + 16 * Nz * Nz + 4 * Nz * (Nz - 1))
        r = grad_case(p, ncol, [0, 0, 1, 0, 0, 0], n_timed, mlp, rhs_per_step, label, ma)
        r["rhs_evaluations_per_step"] = rhs_per_step
        return r

    def wide(ma="bf16x3_exact"):    # the reference's wide wind-mixing architecture (train_NDE.jl:101-102, train_NDE_args.jl:150-166): 3 x 96-400-400-31 swish, 4,096 columns
        p = synthetic.wind_mixing_problem(4096, n_frames=17, weight_divisor=1e2, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
        mlp = 3 * 2 * (96 * 400 + 400 * 400 + 400 * 31)
        r = grad_case(p, 4096, [1, 1, 1, 5e-3, 5e-3, 5e-3], 2, mlp, 4,
                      "wide wind-mixing networks: 3 x (96-400-400-31 swish), 4096 columns x 32 levels x 32 RK4 steps (17 frames), fwd+adjoint; tile16 with the "
                      "activation rows in global memory (DevModel::ag), taped dW", ma)
        return r

    def c5():       # BASELINE configs[4]: inference forcing, 256 x 256 columns x 32 levels (one GPU holds the whole grid here)
        cfg, T, tf, w = synthetic.inference_problem(256, 256)
        nde = colnde.ColumnNDE(cfg, 65536)
        try:
            Td, tfd, wd = (torch.from_numpy(a).to(dev) for a in (T, tf, w))
            nde.set_profiling(True)
            nde.infer_forcing(wd, Td, tfd, 1024.0)
            nde.reset_kernel_times()
            dt = timed(lambda: nde.infer_forcing(wd, Td, tfd, 1024.0), 20)
            ms, n = nde.kernel_time("infer")
            kt = ms / n * 1e-3
            mlp = 2 * (32 * 128 + 128 * 128 + 128 * 31)
            return {"workload": "configs[4]: double_gyre_nn forcing, 256x256 columns x 32 levels, 32-128-128-31", "columns": 65536,
                    "ms": dt * 1e3, "kernel_ms": kt * 1e3, "columns_per_s": 65536 / kt,
                    "mfma": {"flop_per_column": mlp, "achieved_TFLOPs": 65536 * mlp / kt / 1e12, "frac": 65536 * mlp / kt / 1e12 / PEAK_FP32_MFMA_TFLOPS},
                    "hbm": {"algorithmic_bytes_per_column": 260, "achieved_GBps": 65536 * 260 / kt / 1e9, "frac": 65536 * 260 / kt / 1e9 / PEAK_HBM_GBPS}}
        finally:
            nde.close()

    def impl():     # the implicit steps either side of the NN forcing, HBM-bound, 4 M columns x 32 levels
        cfg = synthetic.free_convection_problem(1, Nz=32, n_save=2).cfg
        nde = colnde.ColumnNDE(cfg, 1)
        try:
            ncol = 4 * 1024 * 1024
            g = torch.Generator(device="cpu").manual_seed(2)
            k = torch.arange(32)[None, :]
            u = (0.05 * torch.tanh((k - 24) / 4.0) + 2e-3 * torch.randn(ncol, 32, generator=g)).to(dev)
            v = (0.02 * torch.tanh((k - 20) / 5.0) + 2e-3 * torch.randn(ncol, 32, generator=g)).to(dev)
            T = (19.6 + 0.4 * k / 32 + 0.02 * torch.randn(ncol, 32, generator=g)).to(dev)
            outs = tuple(torch.empty_like(T) for _ in range(3))
            nde.set_profiling(True)
            prm = (1e-4, 1e-1, 1.0, 0.25, 1.0, 1.67e-4, 9.81)
            r = {"columns": ncol, "levels": 32}
            for name, kid, nbytes, fn in (
                    ("implicit_mpp_diffusion", "impldiff", 768, lambda: nde.implicit_diffusion(u, v, T, 60.0, 8.0, prm, True, out=outs)),
                    ("convective_adjustment", "convadj", 256, lambda: nde.convective_adjustment(T, 1200.0, 62.5, 10.0, out=outs[2]))):
                fn()
                nde.reset_kernel_times()
                timed(fn, 10)
                ms, n = nde.kernel_time(kid)
                kt = ms / n * 1e-3
                r[name] = {"kernel_ms": kt * 1e3, "columns_per_s": ncol / kt, "algorithmic_bytes_per_column": nbytes,
                           "hbm": {"achieved_GBps": ncol * nbytes / kt / 1e9, "frac": ncol * nbytes / kt / 1e9 / PEAK_HBM_GBPS}}
            return r
        finally:
            nde.close()

    def f32(fn):                    # the opt-out (COLNDE_MATRIX_F32_MFMA) twin of a case, reported beside the default
        def run():
            r = fn("f32_mfma")
            r["matrix_arithmetic"] = "opt-out: COLNDE_MATRIX_F32_MFMA (v_mfma_f32_* throughout)"
            return r
        return run

    guarded("config2_forward_4096", c2)
    guarded("config2_forward_4096_f32_mfma", f32(c2))
    guarded("config3_8_simulations", c3)
    guarded("config3_8_simulations_f32_mfma", f32(c3))
    guarded("config3_8_simulations_conv_adj_kappa10_rkc2", c3ca)
    guarded("config3_8_simulations_conv_adj_kappa10_rkc2_f32_mfma", f32(c3ca))
    guarded("wide_wind_mixing_4096", wide)
    guarded("config5_inference_65536", c5)
    guarded("implicit_steps_4M_columns", impl)
    fc8_32 = "free convection at a latency size: 8 simulations x 32 levels x 512 RK4 steps, fwd+adjoint (fc32 on 16-column tiles)"
    fc8_64 = "free convection at a latency size: 8 simulations x 64 levels x 512 RK4 steps, fwd+adjoint (fc32 on 16-column tiles)"
    guarded("free_convection_8_simulations_32_levels", lambda: fc(8, 32, False, 3, fc8_32))
    guarded("free_convection_8_simulations_32_levels_f32_mfma", f32(lambda ma: fc(8, 32, False, 3, fc8_32, ma)))
    guarded("free_convection_8_simulations_64_levels", lambda: fc(8, 64, False, 3, fc8_64))
    guarded("free_convection_8_simulations_64_levels_f32_mfma", f32(lambda ma: fc(8, 64, False, 3, fc8_64, ma)))
    guarded("free_convection_32_levels_16384", lambda: fc(16384, 32, False, 2, "free convection 32 levels (32-128-128-31 relu), 16384 columns x 512 RK4 steps, fwd+adjoint"))
    c4_label = "configs[3] one GPU's shard: FreeConvectionNDE, 16384 columns x 64 levels x 512 RK4 steps, 64-256-256-63 relu, fwd+adjoint"
    guarded("config4_shard_16384x64", lambda: fc(16384, 64, False, 2, c4_label))
    guarded("config4_shard_16384x64_f32_mfma", f32(lambda ma: fc(16384, 64, False, 2, c4_label, ma)))
    guarded("config4_shard_16384x64_conv_adj_rkc2", lambda: fc(16384, 64, True, 1, "configs[3] one GPU's shard: ConvectiveAdjustmentNDE (K = 10), 16384 columns x 64 levels x 512 RKC2 steps, fwd+adjoint"))
    return out


def free_convection_workload(args, world, rank, local_rank, dev, comm, dist):
    """BASELINE configs[3] as an N-GPU run: every rank holds `--columns` (default 16,384 = 65,536 / 4) columns of the 64-level FreeConvectionNDE
    (64-256-256-63 relu, 129 save points, 4 RK4 sub-steps: fc32 engine), one SUM all-reduce of [grad(98,623); 6 terms; total; 0] per iteration.
    Same timing contract as the headline: W warm-up steps, K timed steps between barriers, MAX over ranks, rank 0 prints one JSON line."""
    import torch
    import colnde
    from colnde import synthetic
    ncol = args.columns
    p = synthetic.free_convection_problem(ncol, Nz=64, seed=synthetic.SEED + rank)
    pw = synthetic.free_convection_problem(1, Nz=64, n_save=2, seed=synthetic.SEED)          # replicated weights: identical on every rank
    nde = colnde.ColumnNDE(p.cfg, ncol, device=local_rank)
    nde.set_global_columns(ncol * world)
    x0, bcs = torch.from_numpy(p.x0).to(dev), torch.from_numpy(p.bcs).to(dev)
    w, wt = torch.from_numpy(pw.weights).to(dev), torch.from_numpy(pw.weights_truth).to(dev)
    nde.set_problem(x0, bcs)
    truth = nde.forward(wt)
    nde.set_problem(x0, bcs, truth)
    out = torch.empty(nde.n_params + 8, dtype=torch.float32, device=dev)
    sc = [0, 0, 1, 0, 0, 0]
    sync_buf = torch.zeros(1, dtype=torch.float32, device=dev)

    def reduce_(t, op):
        if comm is not None:
            comm.allreduce(t, op)
        elif dist is not None:
            dist.all_reduce(t, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX}[op])

    def step():
        nde.loss_grad(w, sc, out=out)
        if comm is not None:
            comm.allreduce_result(nde, out)
        elif dist is not None:
            dist.all_reduce(out, op=dist.ReduceOp.SUM)

    def barrier():
        reduce_(sync_buf, "sum")
        torch.cuda.synchronize()

    spread = None
    if comm is not None or dist is not None:
        from colnde.distributed import weights_in_sync
        ok, spread = weights_in_sync(w, lambda t: reduce_(t, "max"))
        if not ok:
            raise SystemExit("bench.py: the ranks' weight vectors differ (checksum spread %.3e)" % spread)
    for _ in range(args.warmup):
        step()
    barrier()
    nde.set_profiling(True)
    nde.reset_kernel_times()
    sensors = GpuSensors(dev).start() if rank == 0 and args.full else None     # (a host thread reading two sysfs nodes every 20 ms: nothing on the GPU)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    te = torch.tensor([time.perf_counter() - t0], dtype=torch.float32, device=dev)
    clock = sensors.stop() if sensors is not None else None
    if clock:
        clock["sampled_over"] = "the timed K steps"
        if clock.get("board_power_W_mean"):
            clock["energy_J_per_step"] = clock["board_power_W_mean"] * float(te.item()) / args.steps
    reduce_(te, "max")
    torch.cuda.synchronize()
    elapsed = float(te.item())
    km = {k: nde.kernel_time(k)[0] / max(nde.kernel_time(k)[1], 1) for k in ("forward", "adjoint", "dw1", "reduce")}
    res = out.cpu().numpy()
    if rank == 0 and args.dump_outputs:
        npar = nde.n_params
        dump_outputs(args.dump_outputs, {"gradient": res[:npar], "loss_terms": res[npar:npar + 6], "loss_total": res[npar + 6:npar + 7]})
    if rank == 0:
        cs = ncol * world * p.cfg.n_steps
        mlp = 2 * (64 * 256 + 256 * 256 + 256 * 63)
        flop = 3 * 4 * mlp                                                  # forward + dX + dW per column-timestep
        per_gpu_tf = flop * cs / (elapsed / args.steps) / 1e12 / world
        dom = max(("forward", "adjoint", "dw1"), key=lambda k: km[k])
        dom_tf = 4 * mlp * ncol * p.cfg.n_steps / (km[dom] * 1e-3) / 1e12
        plan = nde.plan()
        on_bf16 = {"forward": plan.get("bf16x3_forward"), "adjoint": plan.get("bf16x3_adjoint"), "dw1": plan.get("bf16x3_dw")}
        # executed MFMA flop per RHS evaluation and column: the 63-row output layer runs as 64 rows; under the exact three-way split every
        # f32 product is SIX bf16 products (csrc/engine_fc_split.hip, dw_gemm_split_kernel), else one f32 MFMA product
        mlp_exec = 2 * (64 * 256 + 256 * 256 + 256 * 64)
        def pipe_frac(k):
            ex = 4 * mlp_exec * ncol * p.cfg.n_steps
            t = km[k] * 1e-3
            return (6 * ex / (PEAK_BF16_MFMA_TFLOPS * 1e12) if on_bf16[k] else ex / (PEAK_FP32_MFMA_TFLOPS * 1e12)) / t if t > 0 else None
        dom_frac = pipe_frac(dom)
        names = {"forward": "fcs_forward_kernel" if on_bf16["forward"] else "fc_forward_kernel",
                 "adjoint": "fcs_adjoint_kernel" if on_bf16["adjoint"] else "fc_adjoint_kernel",
                 "dw1": "dw_gemm_split_kernel" if on_bf16["dw1"] else "dw_gemm_lds_kernel"}
        step_ms = elapsed / args.steps * 1e3
        print(json.dumps({
            "metric": "column-timesteps/sec (fwd+adjoint), 64-level free-convection NDE (BASELINE configs[3])",
            "value": cs * args.steps / elapsed, "unit": "column-timesteps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "free_convection NDE training (BASELINE configs[3]: 65536 columns x 64 levels on 4 GPUs): %d columns/GPU x 64 levels x 129 save "
                                   "points x 4 RK4 sub-steps, FreeConvectionNDE, 64-256-256-63 relu, single MSE loss" % ncol,
                       "columns_per_gpu": ncol, "levels": 64, "rk4_steps": p.cfg.n_steps, "n_params": p.cfg.n_params, "parallelism": "columns sharded x%d" % world,
                       "matrix_arithmetic": nde.matrix_arithmetic,
                       "exchange": "none (one rank)" if (comm is None and dist is None) else ("colnde_comm (RCCL behind the C ABI)" if comm is not None else "torch.distributed nccl (RCCL)")},
            # achieved = ALGORITHMIC f32-equivalent TFLOP/s of the dominant kernel; frac = the time its EXECUTED MFMA instructions need on the matrix
            # pipe (bf16 flop / 2.5 PF, f32 flop / 157.3 TF) over its duration; peak = achieved / frac (same convention as the headline line)
            "roofline": {"kernel": names[dom], "bound": "mfma",
                         "achieved": dom_tf, "peak": (dom_tf / dom_frac) if dom_frac else PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": dom_frac, "traffic": None,
                         "frac_is": "matrix-pipe time fraction of the executed MFMA instruction mix", "avg_launch_ms": km[dom], "kernel_ms": km,
                         # the step runs power-limited: the peaks behind `frac` assume 2,400 MHz
                         "clock": clock, "frac_at_measured_clock": (dom_frac * 2400.0 / clock["shader_clock_MHz_mean"]) if (clock and dom_frac) else None,
                         "kernels": {k: {"kernel": names[k], "on_bf16_pipe": bool(on_bf16[k]), "avg_launch_ms": km[k], "matrix_pipe_time_frac": pipe_frac(k)}
                                     for k in ("forward", "adjoint", "dw1")},
                         "whole_step": {"algorithmic_flop_per_column_timestep": flop, "achieved": per_gpu_tf, "unit": "TFLOP/s per GPU",
                                        "matrix_pipe_time_frac": sum((pipe_frac(k) or 0.0) * km[k] for k in ("forward", "adjoint", "dw1")) / step_ms},
                         "plan": plan},
            "multi_gpu": None if spread is None else {"allreduce_floats": nde.n_params + 8, "weights_checksum_spread_over_ranks": spread},
            "cpu_baseline": None, "loss_total": float(res[nde.n_params + 6]), "grad_l2": float(np.linalg.norm(res[:nde.n_params])),
        }), flush=True)
    nde.close()
    if comm is not None:
        barrier()
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def inference_workload(args, world, rank, local_rank, dev, comm, dist):
    """BASELINE configs[4]: `compute_neural_network_forcing!` (free_convection/double_gyre_nn.jl:149-168) on the 256 x 256 columns x 32 levels of the
    double-gyre grid (`--global-columns`, default 65,536), dealt over the N ranks in contiguous shards (colnde.distributed.shard_columns; 8 GPUs x
    8,192 columns as the config is written).  A step = one colnde_infer_forcing_dev over the rank's shard.  NO data-path collective:
    the only exchanges are the barriers that bracket the timed region and the MAX over ranks of the elapsed time.  Strong scaling by construction
    (the grid is fixed); rank 0 prints one JSON line with every rank's own time."""
    import torch
    import colnde
    from colnde import synthetic
    from colnde.distributed import shard_columns
    n_global = args.global_columns if args.global_columns > 0 else 65536
    nx = 256 if n_global % 256 == 0 else 1
    cfg, T, tf, wts = synthetic.inference_problem(nx, n_global // nx)
    lo, hi = shard_columns(n_global, rank, world)
    ncol = hi - lo
    if ncol < 1:
        raise SystemExit("--global-columns %d leaves rank %d without columns" % (n_global, rank))
    nde = colnde.ColumnNDE(cfg, ncol, device=local_rank)
    Td, tfd, wd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (T[lo:hi], tf[lo:hi], wts))
    sync_buf = torch.zeros(1, dtype=torch.float32, device=dev)

    def reduce_(t, op):
        if comm is not None:
            comm.allreduce(t, op)
        elif dist is not None:
            dist.all_reduce(t, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX}[op])

    def barrier():
        reduce_(sync_buf, "sum")
        torch.cuda.synchronize()

    out = None
    for _ in range(max(args.warmup, 1)):
        out = nde.infer_forcing(wd, Td, tfd, 1024.0)
    barrier()
    nde.set_profiling(True)
    nde.reset_kernel_times()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = nde.infer_forcing(wd, Td, tfd, 1024.0)
    torch.cuda.synchronize()
    own = time.perf_counter() - t0
    barrier()
    te = torch.tensor([time.perf_counter() - t0], dtype=torch.float32, device=dev)
    reduce_(te, "max")
    torch.cuda.synchronize()
    elapsed = float(te.item())
    ms, n = nde.kernel_time("infer")
    kt = ms / max(n, 1) * 1e-3
    slots = torch.zeros(world, dtype=torch.float32, device=dev)
    slots[rank] = own / args.steps * 1e3
    reduce_(slots, "sum")
    # --full: the shard's first columns against the float32 C port (rank 0; outside the timed region)
    check = None
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"forcing": out.cpu().numpy()})              # rank 0's shard of the last timed step
    if rank == 0:
        if args.full:
            from oracle import cref
            k = min(ncol, 256)
            ref = cref.infer_forcing(cfg, T[lo:lo + k], tf[lo:lo + k], wts, 1024.0)
            got = out[:k].cpu().numpy()
            err = float(np.linalg.norm(got.astype(np.float64) - ref) / (np.linalg.norm(ref) + 1e-300))
            check = {"rel_l2_error": err, "tolerance": 2e-6, "columns": k, "ok": bool(err < 2e-6), "against": "oracle/colnde_ref.c"}
        mlp = 2 * (32 * 128 + 128 * 128 + 128 * 31)
        print(json.dumps({
            "metric": "columns/sec, double_gyre_nn inference forcing (BASELINE configs[4])", "value": n_global * args.steps / elapsed, "unit": "columns/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "double_gyre_nn inference: %d columns (256 x %d) x 32 levels, MLP 32-128-128-31 relu, sharded by column over %d GPU(s), no collective"
                                   % (n_global, n_global // 256 if nx == 256 else n_global, world),
                       "columns_global": n_global, "columns_rank0": ncol, "levels": 32, "parallelism": "columns sharded x%d (colnde.distributed.shard_columns)" % world,
                       "exchange": "none in the data path (barriers around the timed region only)", "matrix_arithmetic": "f32 MFMA (fc_infer_kernel)"},
            "roofline": {"kernel": "fc_infer_kernel", "bound": "hbm", "achieved": ncol * 260 / kt / 1e9, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": ncol * 260 / kt / 1e9 / PEAK_HBM_GBPS, "traffic": None, "algorithmic_bytes_per_column": 260, "avg_launch_ms": kt * 1e3,
                         "note": "launch-bound at this size (%d 32-column tiles on rank 0); algorithmic f32 MFMA rate %.1f TFLOP/s = %.2f of the f32 MFMA peak"
                                 % ((ncol + 31) // 32, ncol * mlp / kt / 1e12, ncol * mlp / kt / 1e12 / PEAK_FP32_MFMA_TFLOPS)},
            "multi_gpu": {"per_rank_ms_per_step_before_the_barrier": [float(x) for x in slots.cpu()], "collectives_in_the_data_path": 0},
            "cpu_baseline": None, "self_check": check,
        }), flush=True)
    nde.close()
    if comm is not None:
        barrier()
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if check is not None and not check["ok"]:
        raise SystemExit("bench.py: inference forcing misses the C port: %r" % (check,))


def _sig(x, n=6):
    """Floats to n significant digits (the compact line is read by a parser with a size limit)."""
    if isinstance(x, float):
        return float("%.*g" % (n, x)) if np.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _sig(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, n) for v in x]
    return x


def compact_line(full):
    """The ONE stdout line: the contract's keys from the full record, nothing else (tests/test_bench_line.py holds it below 8 KB).
    Everything left out here is in gpurun_out/bench_full.json and on stderr."""
    rf = full.get("roofline") or {}
    clock = rf.get("clock") or {}
    hbm = rf.get("hbm") or {}
    kern = rf.get("kernels") or {}
    cfgs = full.get("configs") or {}
    cb = full.get("cpu_baseline")
    oo = (full.get("opt_out") or {}).get("f32_mfma") or {}
    sc = full.get("self_check") or {}
    cfg = full.get("config") or {}

    def side(name, key="ms"):
        v = cfgs.get(name) if isinstance(cfgs, dict) else None
        return v.get(key) if isinstance(v, dict) else None

    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                       "vs_baseline", "dtype", "data")}
    line["config"] = {k: cfg.get(k) for k in ("workload", "columns_per_gpu", "columns_global", "levels", "frames", "substeps", "rk4_steps",
                                              "n_params", "matrix_arithmetic", "parallelism", "exchange") if k in cfg}
    line["roofline"] = {
        "kernel": rf.get("kernel"), "bound": rf.get("bound"), "achieved": rf.get("achieved"), "peak": rf.get("peak"),
        "peak_is": rf.get("peak_is"), "unit": rf.get("unit"), "frac": rf.get("frac"), "traffic": rf.get("traffic"),
        "avg_launch_ms": rf.get("avg_launch_ms"), "launches": rf.get("launches"),
        "frac_at_measured_clock": rf.get("frac_at_measured_clock"),
        "kernel_ms": {k: (kern.get(k) or {}).get("avg_launch_ms") for k in ("forward", "adjoint", "dw1") if k in kern},
        "hbm": {k: hbm.get(k) for k in ("achieved", "peak", "unit", "frac", "algorithmic_bytes_per_column_timestep",
                                        "device_copy_GBps_measured_on_this_box") if k in hbm},
        "hbm_bytes_per_launch_from_counters": {k.replace("_hbm_bytes_per_launch", ""): v for k, v in (rf.get("pmc") or {}).items()
                                               if k.endswith("_hbm_bytes_per_launch")} or None,
        "clock": {"shader_MHz_mean": clock.get("shader_clock_MHz_mean"), "board_W_mean": clock.get("board_power_W_mean"),
                  "board_W_cap": clock.get("board_power_cap_W"), "J_per_step": clock.get("energy_J_per_step"),
                  "peaks_assume_MHz": 2400} if clock else None,
    }
    line["cpu_baseline"] = None if not cb else {k: cb.get(k) for k in ("value", "unit", "cores", "value_1thread", "kind", "sample")}
    line["opt_out"] = {"f32_mfma": {"value": oo.get("value"), "ms_per_step": oo.get("ms_per_step")}} if oo else None
    line["self_check"] = {k: sc.get(k) for k in ("ok", "max_abs_error", "tolerance", "error") if k in sc} if sc else None
    if full.get("multi_gpu"):
        mg = full["multi_gpu"]
        line["multi_gpu"] = {k: mg.get(k) for k in ("per_rank_ms_per_step_before_the_barrier", "allreduce_alone_ms", "allreduce_floats",
                                                    "weights_checksum_spread_over_ranks") if k in mg}
    if isinstance(cfgs, dict) and cfgs:
        # the other BASELINE configs, one scalar each (ms per pass; the full blocks are in bench_full.json)
        line["side_configs_ms"] = {
            "config2_forward_4096_ms": side("config2_forward_4096"), "config3_8sim_ms": side("config3_8_simulations"),
            "config4_shard_ms": side("config4_shard_16384x64"), "config4_shard_conv_adj_rkc2_ms": side("config4_shard_16384x64_conv_adj_rkc2"),
            "config5_inference_kernel_ms": side("config5_inference_65536", "kernel_ms"), "wide_wind_mixing_4096x32steps_ms": side("wide_wind_mixing_4096"),
            "errors": [k for k, v in cfgs.items() if isinstance(v, dict) and ("error" in v or "skipped" in v)] or None}
    line["loss_total"] = full.get("loss_total")
    line["grad_l2"] = full.get("grad_l2")
    line["full_record"] = full.get("full_record")                 # set by --full, the only runs that write the record
    return _sig(line)


def launcher_command(n_gpus, argv):
    """The command `python bench.py --gpus N ...` turns itself into: one rank per GPU under torch.distributed.run.  `--standalone`
    lets the launcher bind its own rendezvous port (no probe-then-reuse race); `--local-addr 127.0.0.1` because the box's hostname
    may not resolve."""
    return [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
            "--nproc-per-node", str(n_gpus), os.path.abspath(__file__)] + list(argv)


def self_launch(n_gpus, argv):
    """Spawn the N ranks as children, relay their output (rank 0 prints the JSON line) and return their exit status.  This process
    never loads HIP or torch: GPUs are counted from the KFD topology in sysfs (colnde.distributed.visible_gpu_count)."""
    import subprocess
    from colnde.distributed import visible_gpu_count
    visible = visible_gpu_count()
    if visible is not None and visible < n_gpus:
        print("bench.py: --gpus %d but only %d GPU(s) visible on this node (KFD topology / *_VISIBLE_DEVICES)" % (n_gpus, visible), file=sys.stderr)
        return 2
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(launcher_command(n_gpus, argv), env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--columns", type=int, default=None, help="columns per GPU (weak scaling); default 32768 (wind_mixing: one 32-column wavefront per SIMD) or 16384 (free_convection)")
    ap.add_argument("--frames", type=int, default=289, help="saved frames (2-day suite: 289)")
    ap.add_argument("--substeps", type=int, default=2)
    ap.add_argument("--global-columns", type=int, default=0, help="N > 1: a GLOBAL column count dealt over the ranks in contiguous, possibly "
                    "ragged shards (colnde.distributed.shard_columns) instead of --columns per GPU: strong scaling, exercises uneven shards")
    ap.add_argument("--workload", choices=["wind_mixing", "free_convection", "inference"], default="wind_mixing",
                    help="wind_mixing (default): the headline, BASELINE's metric.  free_convection: BASELINE configs[3] on N GPUs — FreeConvectionNDE, --columns "
                         "(default 16384) columns per GPU x 64 levels x 512 RK4 steps, one RCCL all-reduce of the 98,631-float result buffer per iteration.  "
                         "inference: BASELINE configs[4] — the double_gyre_nn forcing on --global-columns (default 65536 = 256 x 256) columns x 32 levels dealt "
                         "over the N GPUs by column, no collective")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32, at most 64 MB in all: a fixed seeded sample beyond that)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beyond the headline figure: the steps again without kernel events "
                         "(clock, power), copy bandwidth, the F32_MFMA opt-out, the self-check against the C port, the CPU baseline, the other BASELINE "
                         "configs, the all-reduce alone (N > 1), the full record on disk")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-configs", action="store_true", help="with --full: skip the F32_MFMA opt-out and the block that times the other BASELINE configs after the headline (N = 1 only)")
    args = ap.parse_args()

    if args.substeps < 1 or args.steps < 1 or args.frames < 2:
        raise SystemExit("bench.py times a FIXED discretisation: --substeps >= 1 (the library's substeps = 0 picks a count from reltol at run time), --steps >= 1, --frames >= 2")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # invoked plainly with N > 1: become the launcher.  Nothing in this process touches HIP or imports torch;
        # the ranks are fresh children, never an exec of a process that holds a HIP context.
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))

    import torch
    import colnde
    from colnde import synthetic

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (colnde has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # The exchange step goes through the C ABI's own RCCL communicator (colnde_comm_*, what a Julia host would call);
    # COLNDE_BENCH_COMM=torch selects torch.distributed's backend "nccl" (= RCCL) instead.  COLNDE_BENCH_FORCE_DIST exercises the
    # path with one rank.
    dist = comm = None
    if world > 1 or os.environ.get("COLNDE_BENCH_FORCE_DIST"):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL prints a version banner on stdout when a communicator comes up; stdout carries the ONE JSON line, so the
        # banner goes to stderr (file-descriptor level: the print comes from native code)
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if os.environ.get("COLNDE_BENCH_COMM", "colnde") == "torch":
                import torch.distributed as dist
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
                dist.barrier()
            else:
                from colnde.distributed import bootstrap_comm
                comm = bootstrap_comm(rank, world, local_rank)
                warm = torch.zeros(1, dtype=torch.float32, device=dev)
                comm.allreduce(warm, "sum")
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    if args.columns is None:
        args.columns = 32768 if args.workload == "wind_mixing" else 16384
    if args.workload == "free_convection":
        return free_convection_workload(args, world, rank, local_rank, dev, comm, dist)
    if args.workload == "inference":
        return inference_workload(args, world, rank, local_rank, dev, comm, dist)

    ncol = args.columns
    n_global = ncol * world
    if args.global_columns > 0:
        from colnde.distributed import shard_columns
        lo, hi = shard_columns(args.global_columns, rank, world)
        ncol, n_global = hi - lo, args.global_columns
        if ncol < 1:
            raise SystemExit("--global-columns %d leaves rank %d without columns" % (args.global_columns, rank))
    # each rank generates only its shard of the global synthetic suite (seeded per rank: independent columns)
    prob = synthetic.wind_mixing_problem(ncol, n_frames=args.frames, substeps=args.substeps,
                                         seed=synthetic.SEED + rank)
    # weights are replicated: every rank must start from the identical vector
    wprob = synthetic.wind_mixing_problem(1, n_frames=2, seed=synthetic.SEED)
    cfg = prob.cfg
    scal = np.array([1.0, 1.0, 1.0, 5e-3, 5e-3, 5e-3], dtype=np.float64)   # NDE_training.jl:257-258 defaults

    nde = colnde.ColumnNDE(cfg, ncol, device=local_rank)
    nde.set_global_columns(n_global)
    x0 = torch.from_numpy(prob.x0).to(dev)
    bcs = torch.from_numpy(prob.bcs).to(dev)
    w = torch.from_numpy(wprob.weights).to(dev)
    w_truth = torch.from_numpy(wprob.weights_truth).to(dev)
    nde.set_problem(x0, bcs)
    truth = nde.forward(w_truth)                       # synthetic "truth": trajectory of a perturbed weight set
    nde.set_problem(x0, bcs, truth)
    out = torch.empty(nde.n_params + 8, dtype=torch.float32, device=dev)

    sync_buf = torch.zeros(1, dtype=torch.float32, device=dev)

    def step():
        nde.loss_grad(w, scal, out=out)
        if comm is not None:
            comm.allreduce_result(nde, out)
        elif dist is not None:
            dist.all_reduce(out, op=dist.ReduceOp.SUM)

    def barrier():
        if comm is not None:
            comm.allreduce(sync_buf, "sum")          # every rank arrives before any leaves
        elif dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if comm is None and dist is None:
            return x
        te = torch.tensor([x], dtype=torch.float32, device=dev)
        if comm is not None:
            comm.allreduce(te, "max")
        else:
            dist.all_reduce(te, op=dist.ReduceOp.MAX)
        torch.cuda.synchronize()
        return float(te.item())

    def allreduce_raw(t, op):
        if comm is not None:
            comm.allreduce(t, op)
        else:
            dist.all_reduce(t, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX}[op])

    weights_spread = None
    if comm is not None or dist is not None:
        # divergence guard: every rank must hold the identical weight vector before (and, in training, between) the all-reduced steps
        from colnde.distributed import weights_in_sync
        ok, weights_spread = weights_in_sync(w, lambda t: allreduce_raw(t, "max"))
        if not ok:
            raise SystemExit("bench.py: the ranks' weight vectors differ (checksum spread %.3e)" % weights_spread)

    for _ in range(args.warmup):
        step()
    barrier()
    nde.set_profiling(True)
    nde.reset_kernel_times()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    own_compute = time.perf_counter() - t0            # this rank's K steps, before it waits for the slowest rank
    barrier()
    own = time.perf_counter() - t0
    elapsed = max_over_ranks(own)
    ms_fwd, n_fwd = nde.kernel_time("forward")
    ms_adj, n_adj = nde.kernel_time("adjoint")
    ms_red, n_red = nde.kernel_time("reduce")
    ms_dw1, n_dw1 = nde.kernel_time("dw1")
    nde.set_profiling(False)
    res = out.cpu().numpy()                           # the last timed step's result buffer [grad; 6 loss terms; total; 0]
    if rank == 0 and args.dump_outputs:
        npar = nde.n_params
        dump_outputs(args.dump_outputs, {"gradient": res[:npar], "loss_terms": res[npar:npar + 6], "loss_total": res[npar + 6:npar + 7]})
    elapsed_plain = clock = None
    if args.full:
        # the same K steps once more with the per-kernel HIP events off (reported beside the headline, never instead of it)
        barrier()
        sensors = GpuSensors(dev).start() if rank == 0 else None
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        elapsed_plain = max_over_ranks(time.perf_counter() - t0)
        clock = sensors.stop() if sensors is not None else None
        if clock and clock.get("board_power_W_mean"):
            clock["energy_J_per_step"] = clock["board_power_W_mean"] * elapsed_plain / args.steps       # what a power-limited board makes the figure of merit
    per_rank_ms = allreduce_ms = None
    if comm is not None or dist is not None:
        slots = torch.zeros(world, dtype=torch.float32, device=dev)
        slots[rank] = own_compute / args.steps * 1e3
        allreduce_raw(slots, "sum")
        per_rank_ms = [float(x) for x in slots.cpu()]
        if args.full:
            # the exchange step alone: K all-reduces of the result buffer, back to back
            scratch = out.clone()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                allreduce_raw(scratch, "sum")
            torch.cuda.synchronize()
            allreduce_ms = max_over_ranks(time.perf_counter() - t0) / args.steps * 1e3

    if rank == 0:
        colsteps_per_step = n_global * cfg.n_steps
        value = colsteps_per_step * args.steps / elapsed
        units_per_launch = ncol * cfg.n_steps                     # one adjoint launch covers this rank's columns
        stages32 = units_per_launch * 4 / 32.0                    # 32-column RK4 stages per launch (what EXECUTED_MFMA_FLOP_PER_STAGE32 counts)
        adj_s = ms_adj / max(n_adj, 1) * 1e-3
        fwd_s = ms_fwd / max(n_fwd, 1) * 1e-3
        ab = algorithmic_bytes_per_colstep(cfg.Nz, cfg.substeps)
        # per-launch HBM bytes and SQ shares of the three kernels from the rocprofv3 PMC passes of THIS workload and build
        # (tools/profile_round.sh -> tools/traffic_from_pmc.py, tools/sq_table.py -> profiles/traffic.json): null when they do not match
        traffic = pmc = None
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if (tj.get("columns") == ncol and tj.get("frames") == args.frames and tj.get("substeps") == args.substeps
                        and tj.get("matrix_arithmetic", "f32_mfma") == nde.matrix_arithmetic):
                    traffic = tj.get("adjoint_hbm_bytes_per_launch")
                    pmc = {k: tj[k] for k in ("forward_hbm_bytes_per_launch", "adjoint_hbm_bytes_per_launch", "dw1_hbm_bytes_per_launch",
                                              "sq", "source") if k in tj}
            except Exception:
                traffic = pmc = None
        regtile = nde.engine == 2
        plan = nde.plan()
        ztape = regtile and plan["z1_taped"]
        adj_flop = (ADJ_FLOP_REGTILE if ztape else ADJ_FLOP_REGTILE_NOZ) if regtile else ADJ_FLOP_TILE16
        dw1_s = ms_dw1 / max(n_dw1, 1) * 1e-3
        achieved_tf = adj_flop * units_per_launch / adj_s / 1e12
        step_flop = FWD_FLOP_PER_COLSTEP + adj_flop + (DW1_FLOP_PER_COLSTEP if regtile else 0)
        arith = {k: ("bf16x3_exact" if plan["bf16x3_" + k2] else "f32_mfma") for k, k2 in (("forward", "forward"), ("adjoint", "adjoint"), ("dw1", "dw"))}

        def kernel_block(name, seconds, flop_per_colstep):
            if not (regtile and ztape and seconds > 0):
                return {"avg_launch_ms": seconds * 1e3}
            frac = pipe_time_fraction(name, arith[name], stages32, seconds)
            bf, f32 = EXECUTED_MFMA_FLOP_PER_STAGE32[name][arith[name]]
            r = {"avg_launch_ms": seconds * 1e3, "matrix_arithmetic": arith[name],
                 "algorithmic_f32_equivalent_TFLOPs": flop_per_colstep * units_per_launch / seconds / 1e12,
                 "executed_bf16_mfma_TFLOPs": stages32 * bf / seconds / 1e12, "executed_f32_mfma_TFLOPs": stages32 * f32 / seconds / 1e12,
                 "matrix_pipe_time_frac": frac}
            if pmc and name + "_hbm_bytes_per_launch" in pmc:
                r["hbm_TBps_from_counters"] = pmc[name + "_hbm_bytes_per_launch"] / seconds / 1e12
                r["hbm_frac_of_achievable_6.29TBps"] = r["hbm_TBps_from_counters"] * 1e3 / HBM_ACHIEVABLE_GBPS
            return r

        kb = {"forward": kernel_block("forward", fwd_s, FWD_FLOP_PER_COLSTEP), "adjoint": kernel_block("adjoint", adj_s, adj_flop),
              "dw1": kernel_block("dw1", dw1_s, DW1_FLOP_PER_COLSTEP)}
        mixed = regtile and ztape
        dom_frac = kb["adjoint"].get("matrix_pipe_time_frac") if mixed else achieved_tf / PEAK_FP32_MFMA_TFLOPS
        whole_pipe = (sum((kb[k].get("matrix_pipe_time_frac") or 0.0) * kb[k]["avg_launch_ms"] for k in kb) / (elapsed / args.steps * 1e3)) if mixed else None
        line = {
            "metric": "column-timesteps/sec (fwd+adjoint), 32-level wind-mixing NDE",
            "value": value, "unit": "column-timesteps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_per_step_without_kernel_events": None if elapsed_plain is None else elapsed_plain / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if args.global_columns > 0 else "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": "wind_mixing train_NDE 2DaySuite shape (BASELINE configs[2]: 8 sims x 32 levels x 289 frames, fwd+adjoint): synthetic suite replicated to "
                            "%d columns/GPU x %d levels x %d frames, %d RK4 sub-steps/frame, MPP + zero_weights + train_gradient, "
                            "3 x (96-50-20-31 mish), six-term loss" % (ncol, cfg.Nz, args.frames, cfg.substeps),
                "columns_per_gpu": ncol, "columns_global": n_global, "levels": cfg.Nz, "frames": args.frames, "substeps": cfg.substeps,
                "rk4_steps": cfg.n_steps, "n_params": cfg.n_params, "parallelism": "columns sharded x%d" % world,
                "matrix_arithmetic": "f32 via exact 3xbf16 split, fp32 accumulate (COLNDE_MATRIX_BF16X3_EXACT, the library default)"
                                     if nde.matrix_arithmetic == "bf16x3_exact" else "f32 MFMA (COLNDE_MATRIX_F32_MFMA)",
                "exchange": "none (one rank)" if (comm is None and dist is None) else
                            ("colnde_comm (RCCL behind the C ABI)" if comm is not None else "torch.distributed nccl (RCCL)"),
            },
            "roofline": {
                "kernel": "rt_adjoint_kernel" if regtile else "adjoint_kernel", "bound": "mfma",
                # achieved = ALGORITHMIC f32-equivalent TFLOP/s of the dominant kernel; frac = the time its EXECUTED MFMA mix needs on the
                # matrix pipe (bf16 flop / 2.5 PF + f32 flop / 157.3 TF) over its duration; peak = achieved / frac, the algorithmic rate at which
                # this instruction mix would saturate the pipe.  (Under F32_MFMA the mix is all-f32 and peak is the f32 MFMA peak of 157.3.)
                "achieved": achieved_tf, "peak": (achieved_tf / dom_frac) if dom_frac else PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "peak_is": "derived: achieved / frac (the algorithmic rate at which this bf16 + f32 MFMA mix would fill the matrix pipe)" if mixed
                           else "f32 MFMA dense peak (MI355X_MICROARCH.md)",
                "frac": dom_frac, "traffic": traffic,
                "matrix_arithmetic": ("f32 via exact 3xbf16 split, fp32 accumulate: " if nde.matrix_arithmetic == "bf16x3_exact" else "f32 MFMA: ") +
                                     ", ".join("%s kernel %s" % (k, v) for k, v in arith.items()),
                "limiter": "VALU issue beside the matrix pipe (one wave per SIMD: MFMA chains and vector phases are serial; SQ shares in `pmc.sq` when "
                           "the profile of this build is present), with HBM tape traffic next (`kernels.*.hbm_TBps_from_counters`)",
                "algorithmic_flop_per_column_timestep": adj_flop,
                "whole_step": {"algorithmic_flop_per_column_timestep": step_flop,
                               "achieved": step_flop * colsteps_per_step / (elapsed / args.steps) / 1e12 / world, "unit": "TFLOP/s per GPU (algorithmic, f32-equivalent)",
                               "matrix_pipe_time_frac": whole_pipe,
                               "of_f32_mfma_peak": None if mixed and nde.matrix_arithmetic == "bf16x3_exact" else
                                                   step_flop * colsteps_per_step / (elapsed / args.steps) / 1e12 / world / PEAK_FP32_MFMA_TFLOPS},
                "avg_launch_ms": adj_s * 1e3, "launches": n_adj,
                "kernels": kb,
                # the step runs power-limited: at the measured clock the matrix pipe's peak is (clock / 2400) of the figure `frac` is quoted against
                "clock": clock,
                "frac_at_measured_clock": (dom_frac * 2400.0 / clock["shader_clock_MHz_mean"]) if (clock and dom_frac) else None,
                "hbm": {"achieved": ab["adjoint"] * units_per_launch / adj_s / 1e9, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                        "frac": ab["adjoint"] * units_per_launch / adj_s / 1e9 / PEAK_HBM_GBPS,
                        "algorithmic_bytes_per_column_timestep": ab["adjoint"],
                        "achievable_GBps_guide": HBM_ACHIEVABLE_GBPS},
                "pmc": pmc,
                "reduce_kernel_avg_ms": ms_red / max(n_red, 1),
                "engine": {1: "tile16", 2: "regtile"}.get(nde.engine, str(nde.engine)),
                "plan": plan,
            },
            "multi_gpu": None if per_rank_ms is None else {
                "per_rank_ms_per_step_before_the_barrier": per_rank_ms, "allreduce_alone_ms": allreduce_ms,
                "allreduce_floats": nde.n_params + 8, "weights_checksum_spread_over_ranks": weights_spread},
            "loss_total": float(res[nde.n_params + 6]),
            "grad_l2": float(np.linalg.norm(res[:nde.n_params])),
        }
        extras = world == 1 and args.full                # the measurements and checks beyond the headline: --full, one rank, outside the timed region
        if extras:
            # outside the timed region: the box's own copy bandwidth, beside the guide's 6.29 TB/s and the 8 TB/s vendor figure
            cp = measured_copy_bandwidth(dev)
            line["roofline"]["hbm"]["device_copy_GBps_measured_on_this_box"] = cp
            if cp:
                line["roofline"]["hbm"]["frac_of_measured_copy"] = ab["adjoint"] * units_per_launch / adj_s / 1e9 / cp
        if extras and regtile and not args.no_configs:
            # opt-out, outside the timed region, same handle and tapes: the same step under COLNDE_MATRIX_F32_MFMA (v_mfma_f32_* throughout)
            try:
                gd = out[:nde.n_params].clone()
                loss_d = float(out[nde.n_params + 6])
                nde.set_matrix_arithmetic("f32_mfma")
                step()
                torch.cuda.synchronize()
                nde.set_profiling(True)
                nde.reset_kernel_times()
                sens32 = GpuSensors(dev).start()
                t0 = time.perf_counter()
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                t_f32 = (time.perf_counter() - t0) / 3
                clock32 = sens32.stop()
                if clock32 and clock32.get("board_power_W_mean"):
                    clock32["energy_J_per_step"] = clock32["board_power_W_mean"] * t_f32
                km = {k: nde.kernel_time(k)[0] / max(nde.kernel_time(k)[1], 1) for k in ("forward", "adjoint", "dw1")}
                g32 = out[:nde.n_params]
                third = nde.n_params // 3
                l1 = lambda g: torch.cat([g[n * third:n * third + 4850] for n in range(3)]).double()
                line["opt_out"] = {"f32_mfma": {
                    "switch": "colnde_config.matrix_arithmetic = COLNDE_MATRIX_F32_MFMA (colnde_set_matrix_arithmetic on the same handle)",
                    "ms_per_step": t_f32 * 1e3, "value": colsteps_per_step / t_f32, "kernel_ms": km, "clock": clock32,
                    "adjoint_kernel_of_f32_mfma_peak": adj_flop * units_per_launch / (km["adjoint"] * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                    "default_vs_f32_mfma": {
                        "gradient_rel_l2": float((gd.double() - g32.double()).norm() / g32.double().norm()),
                        # the layer-1 blocks alone (W1, b1 lead each net's third of the vector): with the bench's weights/1e5 they are ~1e-10 of the whole
                        # gradient's norm and a cancellation of 75 M terms, on which f32 MFMA itself stands 2e-3 from the float64 oracle
                        # (tests/test_gpu_parity.py, LONG_GRAD_REL[1e5]); the well-conditioned measurements (7e-8) are the tests on weights/1e2 and weights/4
                        "layer1_gradient_rel_l2": float((l1(gd) - l1(g32)).norm() / l1(g32).norm()),
                        "loss_rel": abs(loss_d - float(out[nde.n_params + 6])) / abs(float(out[nde.n_params + 6]))}}}
            except Exception as e:
                line["opt_out"] = {"f32_mfma": {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}}
            finally:
                nde.set_profiling(False)
                nde.set_matrix_arithmetic("bf16x3_exact")
        if extras:
            # the bench checks its own launch (VERDICT r3 task 4c): 8 columns of this handle's forward solve against the float32 C port
            try:
                line["self_check"] = check_forward_against_port(nde, prob, w, dev)
            except Exception as e:
                line["self_check"] = {"ok": False, "error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        if extras and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(prob, scal)
        else:
            line["cpu_baseline"] = None
    nde.close()
    if rank == 0:
        full_path = os.path.join(ROOT, "gpurun_out", "bench_full.json")

        def save_full():
            try:
                os.makedirs(os.path.dirname(full_path), exist_ok=True)
                with open(full_path, "w") as f:
                    json.dump(line, f)
            except OSError:
                pass

        if args.full:
            line["full_record"] = os.path.relpath(full_path, ROOT)
        if world == 1 and args.full and not args.no_configs:
            # The side configs run after the headline's timed region with its tapes released.  The headline is safe before they start: on stderr
            # and in gpurun_out/ (a side config that takes the process down cannot take the measurement with it).
            save_full()
            print("bench.py headline (the compact line follows on stdout after the side configs): " + json.dumps(compact_line(line)), file=sys.stderr, flush=True)
            del truth, x0, bcs, out
            torch.cuda.empty_cache()
            try:
                line["configs"] = other_configs(dev)
            except Exception as e:
                line["configs"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        # The FULL record (side configs, per-kernel blocks, PMC tables, plan) goes to gpurun_out/bench_full.json; stdout carries ONE compact
        # line (< 8 KB: VERDICT r4 — the 25 KB line of round 4 did not parse) with exactly what the contract reads, and stderr stays short too.
        # A plain run writes no record: its line is all it measured.
        if args.full:
            save_full()
        print(json.dumps(compact_line(line)), flush=True)
        if world == 1 and line.get("self_check") and not line["self_check"].get("ok"):
            raise SystemExit("bench.py: the forward solve of the timed handle misses the C port: %r" % (line["self_check"],))
    if comm is not None:
        barrier()
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
