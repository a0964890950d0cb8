"""`ColumnNDE` — one handle on the HIP tile engine for a set of columns (simulations).

Thin, typed front-end of the C ABI (include/colnde.h).  NumPy arrays go through the host-pointer entry
points; torch CUDA(ROCm) tensors go through the `_dev` twins on torch's current stream (PyTorch is used
for device memory, streams and torch.distributed only).  The reference-named closures
(`NDE`, `NDE!`, `loss_NDE`, `loss_gradient_NDE`, `solve_nde`, …) live in wind_mixing.py / free_convection.py.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np

from . import _lib
from ._arrays import _dtype_name, _f32, _is_torch, _ptr, check_ensemble_arrays
from .embed import (EmbeddingMixin, FcEnsembleEmbedded, WmEnsembleEmbedded, check_fc_embed_arrays, check_fc_ens_embed_arrays, check_wm_diag_arrays,
                    check_wm_embed_arrays, check_wm_ens_embed_arrays)
from .config import CONVECTIVE_ADJUSTMENT_NDE, FREE_CONVECTION, WIND_MIXING, MATRIX_ARITHMETIC_NAMES, NDEConfig, matrix_arithmetic_id, to_c_config

KERNEL_IDS = {"forward": 0, "adjoint": 1, "reduce": 2, "rhs": 3, "infer": 4, "dw1": 5, "convadj": 6, "adam": 7, "impldiff": 8, "fc_embed": 9, "flux_diag": 10, "wm_profile": 11}
ENGINE_AUTO, ENGINE_TILE16, ENGINE_REGTILE, ENGINE_FC32 = 0, 1, 2, 3


def min_substeps(cfg: NDEConfig) -> int:
    """`colnde_min_substeps`: the least RK4 sub-steps per save interval inside the diffusive stability bound (no GPU needed)."""
    c, keep = to_c_config(cfg, 1, 0, 0)
    n = _lib.lib().colnde_min_substeps(ctypes.byref(c))
    if n < 0:
        raise _lib.ColndeError(_lib.lib().colnde_last_error().decode("utf-8", "replace"))
    return int(n)


def schedule_min(cfg: NDEConfig):
    """`colnde_schedule_min`: the RK4 stability bound of every save interval's own length, as a tuple of n_save - 1 counts (no GPU needed)."""
    c, keep = to_c_config(cfg, 1, 0, 0)
    counts = (ctypes.c_int * (cfg.n_save - 1))()
    _lib.check(_lib.lib().colnde_schedule_min(ctypes.byref(c), counts))
    return tuple(int(v) for v in counts)


def rkc_stages(cfg: NDEConfig) -> int:
    """`colnde_rkc_stages`: stages per RKC2 step this configuration runs with (no GPU needed)."""
    c, keep = to_c_config(cfg, 1, 0, 0)
    n = _lib.lib().colnde_rkc_stages(ctypes.byref(c))
    if n < 0:
        raise _lib.ColndeError(_lib.lib().colnde_last_error().decode("utf-8", "replace"))
    return int(n)


class ColumnNDE(EmbeddingMixin):
    def __init__(self, cfg: NDEConfig, n_columns: int, device: int = 0, engine: int = 0, matrix_arithmetic="bf16x3_exact", conv: int = 0):
        """matrix_arithmetic: "bf16x3_exact" (default: f32 products as six bf16 MFMA products of exact three-way operand splits, f32 accumulation,
        wherever the engine has a split kernel) or "f32_mfma" (v_mfma_f32_* throughout) — include/colnde.h COLNDE_MATRIX_*.
        conv = c > 1: the free-convection driver's `--conv c` network (`colnde_create_conv`) — cfg is the plain fc32 configuration, the first
        Dense takes Nz - c + 1 inputs behind a c-tap filter, and the weight vector has `free_convection.conv_n_params(Nz, c)` entries."""
        cfg.validate()
        self.cfg = cfg
        self.n_columns = int(n_columns)
        self.device = int(device)
        self.conv = int(conv)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        c, keep = to_c_config(cfg, n_columns, device, engine, matrix_arithmetic)
        if self.conv:
            _lib.check(L.colnde_create_conv(ctypes.byref(c), self.conv, ctypes.byref(self._h)))
        else:
            _lib.check(L.colnde_create(ctypes.byref(c), ctypes.byref(self._h)))
        self._L = L
        self.n_params = L.colnde_n_params(self._h)
        if self.conv:
            assert L.colnde_conv_filter(self._h) == self.conv
            assert self.n_params == self.conv + 1 + cfg.n_params - 4 * cfg.Nz * (self.conv - 1)
        else:
            assert self.n_params == cfg.n_params
        self.n_columns_total = self.n_columns
        self.engine = L.colnde_engine(self._h)      # engine actually selected (ENGINE_TILE16 or ENGINE_REGTILE)

    # ---- lifetime -------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.colnde_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- configuration --------------------------------------------------------------------------------
    def set_stream(self, stream_ptr: int):
        _lib.check(self._L.colnde_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def set_matrix_arithmetic(self, matrix_arithmetic):
        """Switch the handle between "bf16x3_exact" and "f32_mfma" for a same-handle A/B.  The tapes stay; a planned dW GEMM
        takes the slice count (and the slab rows) a fresh handle of the new arithmetic plans, so the results are that handle's bit for bit."""
        _lib.check(self._L.colnde_set_matrix_arithmetic(self._h, matrix_arithmetic_id(matrix_arithmetic)))

    @property
    def matrix_arithmetic(self) -> str:
        return MATRIX_ARITHMETIC_NAMES[self._L.colnde_matrix_arithmetic(self._h)]

    def set_global_columns(self, n_total: int):
        _lib.check(self._L.colnde_set_global_columns(self._h, int(n_total)))
        self.n_columns_total = int(n_total)

    def set_profiling(self, on: bool = True):
        _lib.check(self._L.colnde_set_profiling(self._h, int(bool(on))))

    def kernel_time(self, which: str):
        ms = ctypes.c_float(0)
        n = ctypes.c_int(0)
        _lib.check(self._L.colnde_kernel_time(self._h, KERNEL_IDS[which], ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def plan(self):
        """How the gradient path runs (valid after the first loss_grad): engine, column blocks, which tapes are in use."""
        info = (ctypes.c_int * 8)()
        _lib.check(self._L.colnde_plan(self._h, info))
        return dict(engine=info[0], block_columns=info[1], n_blocks=info[2], z1_taped=bool(info[3]) and info[0] == ENGINE_REGTILE,
                    time_segments=info[3] if info[0] == ENGINE_FC32 else 0,
                    conv=info[6] if info[0] == ENGINE_FC32 else 0,       # fc32: the filter length of a conv handle; tile16: the net-split bits
                    dw_taped=bool(info[4]), dw_slices=info[5], split_forward=bool(info[6] & 1) and info[0] != ENGINE_FC32,
                    split_adjoint=bool(info[6] & 2) and info[0] != ENGINE_FC32, split_rich_tape=bool(info[6] & 4) and info[0] != ENGINE_FC32,
                    approximate_gradient=bool(info[7] & 1),
                    # which kernel families run the exact three-way bf16 split (the others: f32 MFMA)
                    bf16x3_forward=bool(info[7] & 2), bf16x3_adjoint=bool(info[7] & 4), bf16x3_dw=bool(info[7] & 8),
                    matrix_arithmetic=self.matrix_arithmetic)

    def describe(self) -> str:
        """`colnde_describe`: the plan spelled out, plus every COLNDE_* tuning switch set in this process that the library reads."""
        need = self._L.colnde_describe(self._h, None, 0)
        if need < 0:
            _lib.check(1)
        buf = ctypes.create_string_buffer(need)
        self._L.colnde_describe(self._h, buf, need)
        return buf.value.decode()

    def pretrain_flux(self, flux_type: int, theta, m, v, profiles, bcs, fluxes, order, gradient_scaling: float, opt, update: bool = True):
        """`colnde_pretrain_flux_dev`: one `Flux.train!` pass (one ADAM update per sample, in `order`) over device tensors; `opt` is a
        flux_compat.ADAM whose running powers are advanced.  Returns the mean per-sample loss (update=False: at fixed weights)."""
        self._chk_dev(theta, (self.n_params,))
        n = int(profiles.shape[0])
        self._chk_dev(profiles, (n, self.cfg.n_state))
        self._chk_dev(bcs, (n, self.cfg.n_bc))
        self._chk_dev(fluxes, (n, self.cfg.Nz + 1))
        if update:
            if m is None or v is None:
                raise ValueError("the ADAM moments m and v are needed when update=True")
            self._chk_dev(m, (self.n_params,))
            self._chk_dev(v, (self.n_params,))
        import torch
        if order is not None and (order.dtype != torch.int32 or not order.is_cuda or order.numel() != n):
            raise ValueError("order must be an int32 device tensor of n entries")
        self.use_torch_stream()
        bt = (ctypes.c_double * 2)(*opt.beta_t)
        loss = ctypes.c_float(0)
        _lib.check(self._L.colnde_pretrain_flux_dev(self._h, int(flux_type), theta.data_ptr(), m.data_ptr() if m is not None else None,
                                                    v.data_ptr() if v is not None else None, profiles.data_ptr(), bcs.data_ptr(),
                                                    fluxes.data_ptr(), order.data_ptr() if order is not None else None, n,
                                                    float(gradient_scaling), opt.eta, opt.beta[0], opt.beta[1], opt.eps, bt, int(bool(update)),
                                                    ctypes.byref(loss)))
        if update:
            opt.beta_t = [bt[0], bt[1]]
        return float(loss.value)

    def reset_kernel_times(self):
        _lib.check(self._L.colnde_reset_kernel_times(self._h))

    # ---- problem data ---------------------------------------------------------------------------------
    def set_problem(self, x0, bcs, truth=None):
        c = self.cfg
        if _is_torch(x0):
            self._chk_dev(x0, (self.n_columns, c.n_state))
            self._chk_dev(bcs, (self.n_columns, c.n_bc))
            if truth is not None:
                self._chk_dev(truth, (self.n_columns, c.n_save, c.n_state))
            self.use_torch_stream()
            _lib.check(self._L.colnde_set_problem_dev(self._h, x0.data_ptr(), bcs.data_ptr(),
                                                      truth.data_ptr() if truth is not None else None))
            return
        x0 = _f32(x0, (self.n_columns, c.n_state))
        bcs = _f32(bcs, (self.n_columns, c.n_bc))
        tr = _f32(truth, (self.n_columns, c.n_save, c.n_state)) if truth is not None else None
        _lib.check(self._L.colnde_set_problem(self._h, _ptr(x0), _ptr(bcs), _ptr(tr)))

    def _chk_dev(self, t, shape):
        import torch
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
            raise ValueError("expected a contiguous float32 device tensor of shape %s" % (tuple(shape),))
        if t.device.index != self.device:
            raise ValueError("tensor on device %s, handle on device %d" % (t.device, self.device))

    # ---- one RHS evaluation ---------------------------------------------------------------------------
    def rhs(self, x, weights, bcs, t: float = 0.0):
        c = self.cfg
        if _is_torch(x):
            import torch
            n = x.shape[0]
            self._chk_dev(x, (n, c.n_state))
            self._chk_dev(weights, (self.n_params,))
            self._chk_dev(bcs, (n, c.n_bc))
            dx = torch.empty_like(x)
            self.use_torch_stream()
            _lib.check(self._L.colnde_rhs_dev(self._h, x.data_ptr(), weights.data_ptr(), bcs.data_ptr(), float(t),
                                              dx.data_ptr(), n))
            return dx
        x = _f32(x)
        n = x.shape[0]
        x = _f32(x, (n, c.n_state))
        w = _f32(weights, (self.n_params,))
        b = _f32(bcs, (n, c.n_bc))
        dx = np.empty_like(x)
        _lib.check(self._L.colnde_rhs(self._h, _ptr(x), _ptr(w), _ptr(b), float(t), _ptr(dx), n))
        return dx

    # ---- flux diagnostics -----------------------------------------------------------------------------
    def flux(self, x, weights, bcs, t: float = 0.0):
        """`predict_flux` (wind_mixing/src/NDE_training.jl:83-147): [n][n_nets][Nz + 1] face fluxes (scaled) of n states; T-only models: the wT that the
        dataset-level `solve_nde` re-evaluates per saved step (free_convection/src/solve.jl:32-46)."""
        c = self.cfg
        nn = 3 if c.n_state == 3 * c.Nz else 1
        if _is_torch(x):
            import torch
            n = x.shape[0]
            self._chk_dev(x, (n, c.n_state))
            self._chk_dev(weights, (self.n_params,))
            self._chk_dev(bcs, (n, c.n_bc))
            fl = torch.empty((n, nn, c.Nz + 1), dtype=torch.float32, device=x.device)
            self.use_torch_stream()
            _lib.check(self._L.colnde_flux_dev(self._h, x.data_ptr(), weights.data_ptr(), bcs.data_ptr(), float(t), fl.data_ptr(), n))
            return fl
        x = _f32(x)
        n = x.shape[0]
        x = _f32(x, (n, c.n_state))
        w = _f32(weights, (self.n_params,))
        b = _f32(bcs, (n, c.n_bc))
        fl = np.empty((n, nn, c.Nz + 1), dtype=np.float32)
        _lib.check(self._L.colnde_flux(self._h, _ptr(x), _ptr(w), _ptr(b), float(t), _ptr(fl), n))
        return fl

    def loss_per_tstep(self, weights):
        """`loss_per_tstep` (wind_mixing/src/loss.jl:44-46) of the six profile terms: [n_columns][6][n_save], unscaled mse per save point."""
        shape = (self.n_columns, 6, self.cfg.n_save)
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_params,))
            out = torch.empty(shape, dtype=torch.float32, device=weights.device)
            self.use_torch_stream()
            _lib.check(self._L.colnde_loss_per_tstep_dev(self._h, weights.data_ptr(), out.data_ptr()))
            return out
        w = _f32(weights, (self.n_params,))
        out = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_loss_per_tstep(self._h, _ptr(w), _ptr(out)))
        return out

    # ---- error-controlled time stepping ---------------------------------------------------------------
    @property
    def substeps(self) -> int:
        """Sub-steps per save interval in use (cfg.substeps, or what the handle chose from reltol)."""
        return int(self._L.colnde_substeps(self._h))

    def set_substeps(self, substeps: int) -> None:
        """colnde_set_substeps: impose a sub-step count (the MAX over ranks of what each shard chose — colnde.distributed.agree_substeps); before the
        first loss_grad of this handle."""
        _lib.check(self._L.colnde_set_substeps(self._h, int(substeps)))

    @property
    def n_steps(self) -> int:
        """Time steps of one solve with the sub-step count IN USE (cfg.n_steps is 0 for a config created with substeps = 0); under a step schedule
        (set_schedule) the sum of its counts."""
        return int(self._L.colnde_schedule(self._h, None))

    # ---- a step schedule: RK4 steps per save interval (include/colnde.h: colnde_set_schedule) ----------
    def set_schedule(self, counts) -> None:
        """colnde_set_schedule: the RK4 steps of every save interval (n_save - 1 positive integers, the same for all columns and members) in
        cfg.substeps' place; None clears it.  The four-wave net-split kernels only (single wind-mixing handles up to 8,192 columns, wind-mixing
        ensembles); before the first loss_grad of a single handle."""
        if counts is None:
            _lib.check(self._L.colnde_set_schedule(self._h, None))
            return
        c = [int(v) for v in counts]
        if len(c) != self.cfg.n_save - 1:
            raise ValueError("a schedule holds one count per save interval: expected %d, got %d" % (self.cfg.n_save - 1, len(c)))
        _lib.check(self._L.colnde_set_schedule(self._h, (ctypes.c_int * len(c))(*c)))

    def schedule(self):
        """colnde_schedule: the steps of every save interval in use, as a tuple (cfg.substeps each without a schedule); n_steps is their sum."""
        c = (ctypes.c_int * (self.cfg.n_save - 1))()
        if self._L.colnde_schedule(self._h, c) < 0:
            _lib.check(1)
        return tuple(int(v) for v in c)

    def choose_schedule(self, weights, reltol: float = 0.0):
        """colnde_choose_schedule: from the per-interval stability minima (powers of two), double the save intervals that add the most to the error
        estimate until it meets `reltol` (0: cfg.reltol); the handle keeps the schedule.  Returns (counts, estimate).  Single handles, before the
        first loss_grad."""
        w = _f32(weights.cpu().numpy() if _is_torch(weights) else weights, (self.n_params,))
        c, est = (ctypes.c_int * (self.cfg.n_save - 1))(), ctypes.c_float(0)
        _lib.check(self._L.colnde_choose_schedule(self._h, _ptr(w), float(reltol), c, ctypes.byref(est)))
        return tuple(int(v) for v in c), float(est.value)

    def error_estimate(self, weights) -> float:
        """Richardson estimate of the solve's error at the current sub-step count against one at twice the count, in the integrator's mixed norm
        max |e| / (1e-3 + |u|) (include/colnde.h: colnde_error_estimate) — what `reltol` bounds."""
        est = ctypes.c_float(0)
        if _is_torch(weights):
            self._chk_dev(weights, (self.n_params,))
            self.use_torch_stream()
            _lib.check(self._L.colnde_error_estimate_dev(self._h, weights.data_ptr(), ctypes.byref(est)))
        else:
            w = _f32(weights, (self.n_params,))
            _lib.check(self._L.colnde_error_estimate(self._h, _ptr(w), ctypes.byref(est)))
        return float(est.value)

    def choose_substeps(self, weights, reltol: float = 0.0):
        """The least power-of-two sub-step count (not below the stability bound) whose error estimate meets `reltol` (0: cfg.reltol); the handle
        keeps it.  Returns (substeps, estimate).  Before the first loss_grad only: the count sizes the tapes."""
        w = _f32(weights.cpu().numpy() if _is_torch(weights) else weights, (self.n_params,))
        s, est = ctypes.c_int(0), ctypes.c_float(0)
        _lib.check(self._L.colnde_choose_substeps(self._h, _ptr(w), float(reltol), ctypes.byref(s), ctypes.byref(est)))
        return int(s.value), float(est.value)

    # ---- forward solve --------------------------------------------------------------------------------
    def forward(self, weights, out=None):
        c = self.cfg
        shape = (self.n_columns, c.n_save, c.n_state)
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_params,))
            sol = out if out is not None else torch.empty(shape, dtype=torch.float32, device=weights.device)
            self._chk_dev(sol, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_forward_dev(self._h, weights.data_ptr(), sol.data_ptr()))
            return sol
        w = _f32(weights, (self.n_params,))
        sol = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_forward(self._h, _ptr(w), _ptr(sol)))
        return sol

    # ---- losses ---------------------------------------------------------------------------------------
    def loss(self, weights, scalings: Sequence[float]):
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_params,))
            out = torch.empty(8, dtype=torch.float32, device=weights.device)
            self.use_torch_stream()
            _lib.check(self._L.colnde_loss_dev(self._h, weights.data_ptr(), sc, out.data_ptr()))
            return out
        w = _f32(weights, (self.n_params,))
        terms = (ctypes.c_float * 6)()
        total = ctypes.c_float(0)
        _lib.check(self._L.colnde_loss(self._h, _ptr(w), sc, terms, ctypes.byref(total)))
        return float(total.value), np.array(list(terms), dtype=np.float32)

    def loss_grad(self, weights, scalings: Sequence[float], out=None):
        """NumPy: (total, terms[6], grad[n_params]).  torch: one device tensor [grad; terms(6); total; 0]
        (the buffer to all-reduce when columns are sharded over ranks)."""
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_params,))
            if out is None:
                out = torch.empty(self.n_params + 8, dtype=torch.float32, device=weights.device)
            self._chk_dev(out, (self.n_params + 8,))
            self.use_torch_stream()
            _lib.check(self._L.colnde_loss_grad_dev(self._h, weights.data_ptr(), sc, out.data_ptr()))
            return out
        w = _f32(weights, (self.n_params,))
        terms = (ctypes.c_float * 6)()
        total = ctypes.c_float(0)
        grad = np.empty(self.n_params, dtype=np.float32)
        _lib.check(self._L.colnde_loss_grad(self._h, _ptr(w), sc, terms, ctypes.byref(total), _ptr(grad)))
        return float(total.value), np.array(list(terms), dtype=np.float32), grad

    def adam_step(self, weights, grad, m, v, eta: float, beta=(0.9, 0.999), eps: float = 1e-8, beta_t=None):
        """One fused `Flux.Optimise.ADAM` apply!/update! on device vectors (in place).  beta_t = running powers (β₁ᵗ, β₂ᵗ)."""
        import torch
        n = weights.numel()
        for t in (weights, m, v):
            self._chk_dev(t, (n,))
        if not (grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous() and grad.numel() >= n):
            raise ValueError("grad must be a contiguous float32 device tensor with at least %d elements" % n)
        bt = beta if beta_t is None else beta_t
        self.use_torch_stream()
        _lib.check(self._L.colnde_adam_step_dev(self._h, weights.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), float(eta),
                                                float(beta[0]), float(beta[1]), float(eps), float(bt[0]), float(bt[1]), n))
        return weights

    # ---- data preparation on device (wind_mixing/src/data_containers.jl:343-427) -------------------------
    def coarse_grain(self, x, n: int, location: str = "center"):
        """`coarse_grain(Φ, n, Center)` / `coarse_grain_linear_interpolation(Φ, n, Face)` on the rows of a device tensor [rows, N]."""
        import torch
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2):
            raise ValueError("expected a contiguous float32 device tensor [rows, N]")
        out = torch.empty(x.shape[0], int(n), dtype=torch.float32, device=x.device)
        self.use_torch_stream()
        _lib.check(self._L.colnde_coarse_grain_dev(self._h, x.data_ptr(), x.shape[0], x.shape[1], int(n),
                                                   {"center": 0, "face": 1}[location], out.data_ptr()))
        return out

    def zscore(self, x):
        """`ZeroMeanUnitVarianceScaling(data)` and its application: returns (scaled, mu_sigma) — both stay on the device."""
        import torch
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            raise ValueError("expected a contiguous float32 device tensor")
        ms = torch.empty(2, dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        self.use_torch_stream()
        _lib.check(self._L.colnde_zscore_stats_dev(self._h, x.data_ptr(), x.numel(), ms.data_ptr()))
        _lib.check(self._L.colnde_scale_dev(self._h, x.data_ptr(), x.numel(), ms.data_ptr(), out.data_ptr()))
        return out, ms


PHYSICS_KEYS = ("nu0", "nu_minus", "dRi", "Ric", "Pr")     # colnde_create_ensemble's physics row (mpp_parameters order)


WM_PRETRAIN_NETS = {"uw": 1, "vw": 2, "wT": 4}      # bits of `nets` of colnde_ensemble_pretrain_wm_flux_dev


def wm_pretrain_nets_mask(nets) -> int:
    """The bit mask of `nets`: an int in 1..7 as it is, or names out of ("uw", "vw", "wT")."""
    if isinstance(nets, (int, np.integer)) and not isinstance(nets, bool):
        mask = int(nets)
    else:
        names = (nets,) if isinstance(nets, str) else tuple(nets) if isinstance(nets, (tuple, list, set, frozenset)) else (None,)
        if not all(isinstance(nm, str) and nm in WM_PRETRAIN_NETS for nm in names):
            raise ValueError("nets: names out of ('uw', 'vw', 'wT') or a bit mask in 1..7, got %r" % (nets,))
        mask = sum(WM_PRETRAIN_NETS[nm] for nm in set(names))
    if not 1 <= mask <= 7:
        raise ValueError("nets: names out of ('uw', 'vw', 'wT') or a bit mask in 1..7, got %r" % (nets,))
    return mask


def check_wm_pretrain_arrays(cfg: NDEConfig, n_models: int, theta, profiles, bcs, fluxes, order=None, etas=None, m=None, v=None):
    """Shape, dtype and order-range rules of `ColumnNDEEnsemble.pretrain_fluxes` (no GPU needed; NumPy arrays or torch tensors), raised before any
    handle is touched: theta, m, v [K, n_params] float32; profiles [n, 3Nz], bcs [n, 6], fluxes [3, n, Nz + 1] (uw, vw, wT; scaled) float32 with
    n >= 1; order [K, 3, n] int32 with every entry in 0..n-1 (an index may repeat), or None; etas [K, 3] float32 or None.  Returns n."""
    K = int(n_models)
    if K < 1:
        raise ValueError("n_models must be >= 1, got %d" % K)
    if cfg.model != 0 or cfg.n_nets != 3:
        raise ValueError("the flux pre-training of an ensemble's three nets takes a wind-mixing configuration (free-convection ensembles: check_fc_pretrain_arrays)")
    P, Nz = cfg.n_params, cfg.Nz
    if len(tuple(profiles.shape)) != 2 or int(profiles.shape[0]) < 1:
        raise ValueError("profiles: expected shape [n, %d] with n >= 1, got %s" % (3 * Nz, tuple(profiles.shape)))
    n = int(profiles.shape[0])
    for name, a, shape in (("theta", theta, (K, P)), ("m", m, (K, P)), ("v", v, (K, P)), ("profiles", profiles, (n, 3 * Nz)), ("bcs", bcs, (n, 6)),
                           ("fluxes", fluxes, (3, n, Nz + 1)), ("etas", etas, (K, 3))):
        if a is None:
            continue
        if tuple(a.shape) != shape:
            raise ValueError("%s: expected shape %s for %d models and %d samples, got %s" % (name, shape, K, n, tuple(a.shape)))
        if _dtype_name(a) != "float32":
            raise ValueError("%s: expected float32, got %s" % (name, _dtype_name(a)))
    if order is not None:
        if tuple(order.shape) != (K, 3, n):
            raise ValueError("order: expected shape %s (one row per model and net), got %s" % ((K, 3, n), tuple(order.shape)))
        if _dtype_name(order) != "int32":
            raise ValueError("order: expected int32, got %s" % _dtype_name(order))
        lo, hi = int(order.min()), int(order.max())
        if lo < 0 or hi >= n:
            raise ValueError("order: entries must lie in 0..%d, got %d..%d" % (n - 1, lo, hi))
    return n


def is_net_split_shape(cfg: NDEConfig) -> bool:
    """The configurations `colnde_create_ensemble` accepts (csrc: rt_supported; no GPU needed): the wind-mixing NDE at Nz = 32 with three 96-50-20-31
    nets, one hidden activation and an identity output layer, on the training RHS without smoothing.  Everything else a tile16 handle trains is
    `TileNDEEnsemble`'s."""
    return (cfg.model == WIND_MIXING and cfg.Nz == 32 and tuple(cfg.layer_sizes) == (96, 50, 20, 31) and len(cfg.activations) == 3 and
            cfg.activations[0] == cfg.activations[1] and cfg.activations[2] == "identity" and not cfg.smooth_NN and not cfg.smooth_Ri and
            not cfg.inplace_variant)


class ColumnNDEEnsemble(ColumnNDE):
    """K models of ONE architecture on the same columns (`colnde_create_ensemble`): own weights, own Pacanowski-Philander constants, own ADAM rate —
    the sweep of wind_mixing/train_NDE_args.jl (one model per process there) with every kernel launched once for all K models.
    physics: [K, 5] = (nu0, nu_minus, dRi, Ric, Pr) per model, or None (cfg's constants for all).  The problem (`set_problem`) and the loss
    scalings are shared.  NumPy inputs go through the host entry points, torch device tensors through the `_dev` twins on torch's current stream.
    The single-model calls of `ColumnNDE` (rhs, flux, error_estimate, ...) are refused by the library on this handle."""

    def __init__(self, cfg: NDEConfig, n_columns: int, n_models: int, physics=None, device: int = 0, matrix_arithmetic="bf16x3_exact"):
        cfg.validate()
        check_ensemble_arrays(n_models, cfg.n_params, physics=None if physics is None else np.asarray(physics))
        self.cfg = cfg
        self.n_columns = int(n_columns)
        self.n_models = int(n_models)
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        c, keep = to_c_config(cfg, n_columns, device, 0, matrix_arithmetic)
        ph = None if physics is None else _f32(physics, (self.n_models, 5))
        _lib.check(L.colnde_create_ensemble(ctypes.byref(c), self.n_models, _ptr(ph), ctypes.byref(self._h)))
        self._L = L
        self.n_params = L.colnde_n_params(self._h)
        assert self.n_params == cfg.n_params and L.colnde_n_models(self._h) == self.n_models
        self.n_columns_total = self.n_columns
        self.engine = L.colnde_engine(self._h)

    def set_physics(self, physics):
        ph = np.asarray(physics)
        check_ensemble_arrays(self.n_models, self.n_params, physics=ph)
        _lib.check(self._L.colnde_ensemble_set_physics(self._h, _ptr(_f32(ph))))

    def _weights_dev(self, weights):
        """torch device weights [K, P] as given; NumPy weights copied to the device (the ensemble calls are device-pointer calls)."""
        import torch
        if _is_torch(weights):
            self._chk_dev(weights, (self.n_models, self.n_params))
            return weights, True
        w = _f32(weights, (self.n_models, self.n_params))
        return torch.from_numpy(w).to(torch.device("cuda", self.device)), False

    def forward(self, weights, out=None):
        """sol [K, n_columns, n_save, n_state]: a torch tensor for torch weights, NumPy for NumPy weights."""
        import torch
        c = self.cfg
        w, is_t = self._weights_dev(weights)
        shape = (self.n_models, self.n_columns, c.n_save, c.n_state)
        sol = out if out is not None else torch.empty(shape, dtype=torch.float32, device=w.device)
        self._chk_dev(sol, shape)
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_forward_dev(self._h, w.data_ptr(), sol.data_ptr()))
        return sol if is_t else sol.cpu().numpy()

    def loss(self, weights, scalings: Sequence[float]):
        """[K, 8] = [scaled terms(6); total; 0] per model."""
        import torch
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        w, is_t = self._weights_dev(weights)
        out = torch.empty((self.n_models, 8), dtype=torch.float32, device=w.device)
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_loss_dev(self._h, w.data_ptr(), sc, out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def loss_grad(self, weights, scalings: Sequence[float], out=None):
        """[K, n_params + 8]: per model the row `colnde_loss_grad_dev` writes — [grad; scaled terms(6); total; 0]."""
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        shape = (self.n_models, self.n_params + 8)
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_models, self.n_params))
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=weights.device)
            self._chk_dev(out, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_ensemble_loss_grad_dev(self._h, weights.data_ptr(), sc, out.data_ptr()))
            return out
        w = _f32(weights, (self.n_models, self.n_params))
        res = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_ensemble_loss_grad(self._h, _ptr(w), sc, _ptr(res)))
        return res

    # ---- the error estimate member by member, one schedule for all K (include/colnde.h: colnde_ensemble_error_estimate) ----
    def ensemble_error_estimate(self, weights):
        """`colnde_ensemble_error_estimate[_dev]`: ndarray [K, n_save], row k what `ColumnNDE.error_estimate` gives for member k at every save point
        alone (column 0 is 0; a member whose solve is not finite has +inf in its own row).  Two tape-less solves of all K members — under the counts
        in force and with every interval doubled — and one kernel; the handle is left as it was.  Torch device weights go to the `_dev` form on
        torch's current stream."""
        est = np.empty((self.n_models, self.cfg.n_save), dtype=np.float32)
        if _is_torch(weights):
            self._chk_dev(weights, (self.n_models, self.n_params))
            self.use_torch_stream()
            _lib.check(self._L.colnde_ensemble_error_estimate_dev(self._h, weights.data_ptr(), _ptr(est)))
        else:
            w = _f32(weights, (self.n_models, self.n_params))
            _lib.check(self._L.colnde_ensemble_error_estimate(self._h, _ptr(w), _ptr(est)))
        return est

    def choose_ensemble_schedule(self, weights, reltol: float = 0.0):
        """`colnde_ensemble_choose_schedule`: `ColumnNDE.choose_schedule`'s greedy run on the maximum over the members (wind-mixing ensembles under
        RK4); the handle keeps the schedule and plans its tapes for it.  Returns (counts, estimates): the counts and ndarray [K], every member's own
        estimate at them (the largest drives the schedule).  reltol = 0: cfg.reltol."""
        w = _f32(weights.cpu().numpy() if _is_torch(weights) else weights, (self.n_models, self.n_params))
        c, est = (ctypes.c_int * (self.cfg.n_save - 1))(), np.empty((self.n_models,), dtype=np.float32)
        _lib.check(self._L.colnde_ensemble_choose_schedule(self._h, _ptr(w), float(reltol), c, _ptr(est)))
        return tuple(int(v) for v in c), est

    # ---- the member loss: every member its own scalings and its own training simulations (include/colnde.h: colnde_ensemble_set_member_loss) ----
    def set_member_loss(self, scalings=None, column_weights=None):
        """`colnde_ensemble_set_member_loss`: member k is differentiated under sum_q s[k][q] sum_c w[k][c] (term q of column c) / sum_c w[k][c].
        scalings [K, 6] or None (every scaling 1); column_weights [K, n_columns] or None (every column 1; a 0/1 row is the member's training
        simulations).  Both None clears it.  Host arrays, copied before the call returns; the upload is ordered on torch's current stream."""
        sc = None if scalings is None else _f32(scalings, (self.n_models, 6))
        cw = None if column_weights is None else _f32(column_weights, (self.n_models, self.n_columns))
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_set_member_loss(self._h, _ptr(sc), _ptr(cw)))

    def member_loss(self, weights):
        """[K, 8] = [scaled terms(6); total; 0] per model under the member loss that was set (`loss` with every member's own scalings and columns)."""
        import torch
        w, is_t = self._weights_dev(weights)
        out = torch.empty((self.n_models, 8), dtype=torch.float32, device=w.device)
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_member_loss_dev(self._h, w.data_ptr(), out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def member_loss_grad(self, weights, out=None):
        """[K, n_params + 8] under the member loss that was set: `loss_grad`'s rows, every member under its own scalings and columns."""
        shape = (self.n_models, self.n_params + 8)
        if _is_torch(weights):
            import torch
            self._chk_dev(weights, (self.n_models, self.n_params))
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=weights.device)
            self._chk_dev(out, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_ensemble_member_loss_grad_dev(self._h, weights.data_ptr(), out.data_ptr()))
            return out
        w = _f32(weights, (self.n_models, self.n_params))
        res = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_ensemble_member_loss_grad(self._h, _ptr(w), _ptr(res)))
        return res

    def adam_step(self, weights, result, m, v, etas, beta=(0.9, 0.999), eps: float = 1e-8, beta_t=None):
        """Flux ADAM for every model (in place): weights, m, v [K, P]; the gradient read from `result` [K, P + 8] (loss_grad's buffer); etas [K]."""
        import torch
        K, P = self.n_models, self.n_params
        for t in (weights, m, v):
            self._chk_dev(t, (K, P))
        self._chk_dev(result, (K, P + 8))
        self._chk_dev(etas, (K,))
        bt = beta if beta_t is None else beta_t
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_adam_step_dev(self._h, weights.data_ptr(), result.data_ptr(), m.data_ptr(), v.data_ptr(), etas.data_ptr(),
                                                         float(beta[0]), float(beta[1]), float(eps), float(bt[0]), float(bt[1])))
        return weights

    def pretrain_fluxes(self, theta, m, v, profiles, bcs, fluxes, order, gradient_scaling: float, etas, nets=("uw", "vw", "wT"), beta=(0.9, 0.999),
                        eps: float = 1e-8, beta_t=None, update: bool = True):
        """`colnde_ensemble_pretrain_wm_flux_dev`: one `Flux.train!` pass of `train_NN` (wind_mixing/src/NN_training.jl:207-249) for the chosen flux
        nets of all K models in one launch, each model under its own closure constants, over device tensors: theta, m, v [K, n_params] (the chosen
        nets' blocks updated in place), profiles [n, 3Nz], bcs [n, 6], fluxes [3, n, Nz + 1] (uw, vw, wT), order [K, 3, n] int32 or None (0..n-1 for
        every chain), etas [K, 3].  nets: names out of ("uw", "vw", "wT") or a bit mask in 1..7.  beta_t: a list [beta1^t, beta2^t] advanced in place
        by n steps (with update; None: a fresh optimiser's).  update=False: nothing is written (m, v, etas may be None), the mean loss at the given
        weights.  Returns the mean losses [K, 3] (NumPy; 0 for a net not chosen): with update, the mean of each sample's loss just before its own update."""
        mask = wm_pretrain_nets_mask(nets)
        if update and etas is None:
            raise ValueError("the rates etas [K, 3] are needed when update=True")
        if update and (m is None or v is None):
            raise ValueError("the ADAM moments m and v are needed when update=True")
        n = check_wm_pretrain_arrays(self.cfg, self.n_models, theta, profiles, bcs, fluxes, order, etas, m, v)
        K, P, Nz = self.n_models, self.n_params, self.cfg.Nz
        for t, shape in ((theta, (K, P)), (m, (K, P)), (v, (K, P)), (profiles, (n, 3 * Nz)), (bcs, (n, 6)), (fluxes, (3, n, Nz + 1)), (etas, (K, 3))):
            if t is not None:
                self._chk_dev(t, shape)
        if order is not None and not (order.is_cuda and order.is_contiguous() and order.device.index == self.device):
            raise ValueError("order must be a contiguous int32 tensor on the handle's device")
        if beta_t is None:
            beta_t = [float(beta[0]), float(beta[1])]
        P_ = lambda a: a.data_ptr() if a is not None else None
        self.use_torch_stream()
        bt = (ctypes.c_double * 2)(float(beta_t[0]), float(beta_t[1]))
        loss = (ctypes.c_float * (3 * K))()
        _lib.check(self._L.colnde_ensemble_pretrain_wm_flux_dev(self._h, mask, P_(theta), P_(m), P_(v), P_(profiles), P_(bcs), P_(fluxes), P_(order), n,
                                                                float(gradient_scaling), P_(etas), float(beta[0]), float(beta[1]), float(eps), bt,
                                                                int(bool(update)), loss))
        if update:
            beta_t[0], beta_t[1] = bt[0], bt[1]
        return np.array(loss, dtype=np.float32).reshape(K, 3)


    def profile(self, weights, sol, physics=None, flux: bool = True, Ri: bool = True, losses: bool = True) -> "EnsembleProfile":
        """What `NDE_profile` (wind_mixing/src/training_postprocessing.jl:404-431, :310-317) evaluates on the saved states of a solve, for ALL K
        models (`colnde_ensemble_profile`): uw, vw, wT [K, n_columns, n_save, Nz + 1] (`predict_flux` per state, scaled units; flux), the Richardson
        number without ε, NaN on the two boundary faces as in the reference (Ri), and `loss_per_tstep` [K, n_columns, 6, n_save] (losses; needs
        truth).  weights [K, n_params]; sol [K, n_columns, n_save, 3 Nz]: the states to diagnose — `forward`'s output or any other solve; nothing
        is solved here.  physics [K, 5] overrides the closure constants for this call only (rows with nu0 = nu_minus = 0: the networks' own share
        of the flux).  numpy arrays or torch device tensors (weights and sol of one kind)."""
        c, K = self.cfg, self.n_models
        check_wm_profile_arrays(K, self.n_params, self.n_columns, c.n_save, c.Nz, weights, sol, physics, flux, Ri, losses)
        ph = None if physics is None else (ctypes.c_float * (5 * K))(*[float(x) for x in np.asarray(physics, dtype=np.float64).reshape(-1)])
        fshape, lshape = (K, self.n_columns, c.n_save, c.Nz + 1), (K, self.n_columns, 6, c.n_save)
        n_out = (3 if flux else 0) + (1 if Ri else 0)
        if _is_torch(sol):
            import torch
            self._chk_dev(weights, (K, self.n_params))
            self._chk_dev(sol, (K, self.n_columns, c.n_save, c.n_state))
            faces = [torch.empty(fshape, dtype=torch.float32, device=sol.device) for _ in range(n_out)]
            ls = torch.empty(lshape, dtype=torch.float32, device=sol.device) if losses else None
            self.use_torch_stream()
            P = lambda a: a.data_ptr() if a is not None else None
            fn = self._L.colnde_ensemble_profile_dev
        else:
            weights, sol = _f32(weights, (K, self.n_params)), _f32(sol, (K, self.n_columns, c.n_save, c.n_state))
            faces = [np.empty(fshape, np.float32) for _ in range(n_out)]
            ls = np.empty(lshape, np.float32) if losses else None
            P = _ptr
            fn = self._L.colnde_ensemble_profile
        f3 = faces[:3] if flux else [None] * 3
        ri = faces[-1] if Ri else None
        _lib.check(fn(self._h, P(weights), P(sol), ph, P(f3[0]), P(f3[1]), P(f3[2]), P(ri), P(ls)))
        return EnsembleProfile(f3[0], f3[1], f3[2], ri, ls)


class TileNDEEnsemble(ColumnNDEEnsemble):
    """K wind-mixing models of ANY architecture a tile16 handle trains (`colnde_create_tile_ensemble`): the reference's wide nets
    (wind_mixing/train_NDE.jl:97-102 — 96-400-400-31, 96-32-400-31, 96-400-31), other depths and activations, other Nz, and the 96-50-20-31 shape on
    tile16's own kernels.  Row k of `forward`, `loss` and `loss_grad` holds the bits of `ColumnNDE(cfg_k, n_columns, engine=ENGINE_TILE16)`.
    Everything but the constructor is `ColumnNDEEnsemble`'s; the library refuses, by name, the calls whose kernels read the net-split shape
    (`set_member_loss` / `member_loss*`, `set_schedule`, `wm_embedded`, `profile`, `pretrain_fluxes`) and every single-model call."""

    def __init__(self, cfg: NDEConfig, n_columns: int, n_models: int, physics=None, device: int = 0, matrix_arithmetic="bf16x3_exact"):
        cfg.validate()
        check_ensemble_arrays(n_models, cfg.n_params, physics=None if physics is None else np.asarray(physics))
        self.cfg = cfg
        self.n_columns = int(n_columns)
        self.n_models = int(n_models)
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        c, keep = to_c_config(cfg, n_columns, device, 0, matrix_arithmetic)
        ph = None if physics is None else _f32(physics, (self.n_models, 5))
        _lib.check(L.colnde_create_tile_ensemble(ctypes.byref(c), self.n_models, _ptr(ph), ctypes.byref(self._h)))
        self._L = L
        self.n_params = L.colnde_n_params(self._h)
        assert self.n_params == cfg.n_params and L.colnde_n_models(self._h) == self.n_models
        self.n_columns_total = self.n_columns
        self.engine = L.colnde_engine(self._h)


class EnsembleProfile(NamedTuple):
    """What `ColumnNDEEnsemble.profile` returns: uw, vw, wT, Ri [K, n_columns, n_save, Nz + 1] and losses [K, n_columns, 6, n_save]; None for
    an output group that was not asked for."""
    uw: object
    vw: object
    wT: object
    Ri: object
    losses: object


def check_wm_profile_arrays(n_models: int, n_params: int, n_columns: int, n_save: int, Nz: int, weights, sol, physics=None, flux: bool = True,
                            Ri: bool = True, losses: bool = True):
    """Shape and argument rules of `ColumnNDEEnsemble.profile` (no GPU needed), raised before any library call."""
    K = int(n_models)
    check_ensemble_arrays(K, n_params, weights=weights, physics=None if physics is None else np.asarray(physics))
    shape = (K, int(n_columns), int(n_save), 3 * int(Nz))
    if tuple(sol.shape) != shape:
        raise ValueError("sol: expected shape %s for %d models, got %s" % (shape, K, tuple(sol.shape)))
    if _is_torch(sol) != _is_torch(weights):
        raise ValueError("weights and sol must be of one kind: both torch device tensors or both NumPy arrays")
    if not (flux or Ri or losses):
        raise ValueError("no outputs: at least one of flux, Ri, losses must be asked for")


CLOSURE_N_PARAMS = 5


FC_ENSEMBLE_MAX_COLUMNS = 4096      # the size up to which a single handle runs 16-column tiles (fc_tile_width)


FC_CONV_FILTERS = range(2, 9)       # filter lengths of the --conv network (FC_CONV_MAX = 8 taps)


def fc_ensemble_n_params(cfg: NDEConfig, conv: int = 0) -> int:
    """Parameters per model of a `FreeConvectionEnsemble`: the plain network's, or — conv = c > 1 — the conv chain's
    (`free_convection.conv_n_params(Nz, c)`: c + 1 filter entries, the first Dense 4Nz x (Nz - c + 1))."""
    c = int(conv)
    return cfg.n_params if not c else c + 1 + cfg.n_params - 4 * cfg.Nz * (c - 1)


def check_fc_ensemble_arrays(cfg: NDEConfig, n_columns: int, n_models: int, weights=None, etas=None, coeff=None, sol=None, result=None, conv: int = 0):
    """Shape rules of `FreeConvectionEnsemble` (no GPU needed), raised before any library call: a free-convection config of the fc32 shape
    Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1) with Nz = 32 or 64, 1 <= n_columns <= 4096, n_models >= 1; weights [K, n_params],
    etas and coeff [K], sol [K, n_columns, n_save, Nz], result [K, n_params + 8].  conv = c (2..8): K `--conv c` networks — cfg stays the plain
    configuration and n_params is `fc_ensemble_n_params(cfg, c)`."""
    if int(conv) and int(conv) not in FC_CONV_FILTERS:
        raise ValueError("conv = %d outside 2..8 (0: the plain three-Dense network)" % int(conv))
    if cfg.model not in (FREE_CONVECTION, CONVECTIVE_ADJUSTMENT_NDE):
        raise ValueError("FreeConvectionEnsemble needs a free-convection config (FreeConvectionNDE or ConvectiveAdjustmentNDE); wind mixing: ColumnNDEEnsemble")
    Nz = cfg.Nz
    if Nz not in (32, 64) or tuple(cfg.layer_sizes) != (Nz, 4 * Nz, 4 * Nz, Nz - 1) or tuple(cfg.activations) != ("relu", "relu", "identity"):
        raise ValueError("FreeConvectionEnsemble covers Dense(Nz,4Nz,relu), Dense(4Nz,4Nz,relu), Dense(4Nz,Nz-1) with Nz = 32 or 64; got Nz = %d, layers %s, "
                         "activations %s" % (Nz, tuple(cfg.layer_sizes), tuple(cfg.activations)))
    if not 1 <= int(n_columns) <= FC_ENSEMBLE_MAX_COLUMNS:
        raise ValueError("n_columns = %d outside 1..%d (the 16-column tiles)" % (int(n_columns), FC_ENSEMBLE_MAX_COLUMNS))
    K = int(n_models)
    n_params = fc_ensemble_n_params(cfg, conv)
    check_ensemble_arrays(K, n_params, weights=weights, etas=etas)
    for name, a, shape in (("coeff", coeff, (K,)), ("sol", sol, (K, int(n_columns), cfg.n_save, Nz)), ("result", result, (K, n_params + 8))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError("%s: expected shape %s for %d models, got %s" % (name, shape, K, tuple(a.shape)))


FC_PRETRAIN_OPTIMISERS = {"adam": 0, "descent": 1}      # `optimiser` of colnde_ensemble_pretrain_flux_dev


def check_fc_pretrain_arrays(cfg: NDEConfig, n_models: int, theta, T, bcs, fluxes, order=None, coeff=None, etas=None, m=None, v=None, conv: int = 0):
    """Shape, dtype and order-range rules of `FreeConvectionEnsemble.pretrain_flux` (no GPU needed; NumPy arrays or torch tensors), raised before any
    handle is touched: theta, m, v [K, n_params] float32 (n_params = `fc_ensemble_n_params(cfg, conv)`); T [n, Nz], bcs [n, 2] = [bottom, top],
    fluxes [n, Nz + 1] float32 with n >= 1; order [K, n] int32 with every entry in 0..n-1 (an index may repeat), or None; coeff, etas [K] float32 or
    None.  Returns n."""
    check_fc_ensemble_arrays(cfg, 1, n_models, conv=conv)
    K, P, Nz = int(n_models), fc_ensemble_n_params(cfg, conv), cfg.Nz
    if len(tuple(T.shape)) != 2 or int(T.shape[0]) < 1:
        raise ValueError("T: expected shape [n, %d] with n >= 1, got %s" % (Nz, tuple(T.shape)))
    n = int(T.shape[0])
    for name, a, shape in (("theta", theta, (K, P)), ("m", m, (K, P)), ("v", v, (K, P)), ("T", T, (n, Nz)), ("bcs", bcs, (n, 2)), ("fluxes", fluxes, (n, Nz + 1)),
                           ("coeff", coeff, (K,)), ("etas", etas, (K,))):
        if a is None:
            continue
        if tuple(a.shape) != shape:
            raise ValueError("%s: expected shape %s for %d models and %d samples, got %s" % (name, shape, K, n, tuple(a.shape)))
        if _dtype_name(a) != "float32":
            raise ValueError("%s: expected float32, got %s" % (name, _dtype_name(a)))
    if order is not None:
        if tuple(order.shape) != (K, n):
            raise ValueError("order: expected shape %s (one row per model), got %s" % ((K, n), tuple(order.shape)))
        if _dtype_name(order) != "int32":
            raise ValueError("order: expected int32, got %s" % _dtype_name(order))
        lo, hi = int(order.min()), int(order.max())
        if lo < 0 or hi >= n:
            raise ValueError("order: entries must lie in 0..%d, got %d..%d" % (n - 1, lo, hi))
    return n


class FreeConvectionEnsemble(ColumnNDEEnsemble):
    """K free-convection networks of the fc32 shape on the same simulations (`colnde_create_fc_ensemble`): the sweep of
    free_convection/train_free_convection_nde.jl (one process per seed / optimiser rate / penalty setting there) and the judging of a training run
    (free_convection/src/testing.jl: the network of every epoch on every simulation), every kernel launched once for all K.  `forward`, `loss`,
    `loss_grad` and `adam_step` are `ColumnNDEEnsemble`'s, with its NumPy / torch rules; row k holds the bits a `ColumnNDE` handle computes for
    model k's weights.  There are no constants to vary: `set_physics` and `wm_embedded` are refused.  `fc_embedded` (inherited from `ColumnNDE`)
    takes the K networks into the embedding ocean column in one launch.
    conv = c > 1: K `--conv c` networks (`colnde_create_conv_ensemble`) — cfg is the plain configuration, a model's vector has
    `free_convection.conv_n_params(Nz, c)` entries and row k holds the bits of `ColumnNDE(cfg, n, conv=c)`; `causal_penalty` masks the first Dense
    weight of the conv chain, 4Nz x (Nz - c + 1)."""

    def __init__(self, cfg: NDEConfig, n_columns: int, n_models: int, device: int = 0, engine: int = 0, matrix_arithmetic="bf16x3_exact", conv: int = 0):
        cfg.validate()
        check_fc_ensemble_arrays(cfg, n_columns, n_models, conv=conv)
        self.conv = int(conv)
        self.cfg = cfg
        self.n_columns = int(n_columns)
        self.n_models = int(n_models)
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        c, keep = to_c_config(cfg, n_columns, device, engine, matrix_arithmetic)
        if self.conv:
            _lib.check(L.colnde_create_conv_ensemble(ctypes.byref(c), self.conv, self.n_models, ctypes.byref(self._h)))
        else:
            _lib.check(L.colnde_create_fc_ensemble(ctypes.byref(c), self.n_models, ctypes.byref(self._h)))
        self._L = L
        self.n_params = L.colnde_n_params(self._h)
        assert self.n_params == fc_ensemble_n_params(cfg, self.conv) and L.colnde_n_models(self._h) == self.n_models
        assert L.colnde_conv_filter(self._h) == self.conv
        self.n_columns_total = self.n_columns
        self.engine = L.colnde_engine(self._h)

    def column_loss(self, sol):
        """[K, n_columns, n_save]: the mean over the levels of (sol - truth)^2 per model, simulation and save point, scaled units —
        `Flux.mse(true, nde, agg = x -> mean(x, dims=1))` (testing.jl:83).  sol: `forward`'s output (torch on the device, or NumPy)."""
        import torch
        check_fc_ensemble_arrays(self.cfg, self.n_columns, self.n_models, sol=sol, conv=self.conv)
        is_t = _is_torch(sol)
        s = sol if is_t else torch.from_numpy(_f32(sol)).to(torch.device("cuda", self.device))
        self._chk_dev(s, tuple(sol.shape))
        out = torch.empty(tuple(sol.shape[:3]), dtype=torch.float32, device=s.device)
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_column_loss_dev(self._h, s.data_ptr(), out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def causal_penalty(self, weights, coeff, result):
        """The soft spatial-causality penalty (train_free_convection_nde.jl:186-197) added to `result` [K, n_params + 8] (loss_grad's buffer):
        total += c_k sum_{r<q} W1_k[r, q]^2, gradient += 2 c_k W1_k[r, q]; coeff [K].  Torch device tensors are updated in place; NumPy arrays
        are copied to the device and the updated result is returned."""
        import torch
        check_fc_ensemble_arrays(self.cfg, self.n_columns, self.n_models, weights=weights, coeff=coeff, result=result, conv=self.conv)
        if _is_torch(result):
            for t, shape in ((weights, (self.n_models, self.n_params)), (coeff, (self.n_models,)), (result, (self.n_models, self.n_params + 8))):
                self._chk_dev(t, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_ensemble_causal_penalty_dev(self._h, weights.data_ptr(), coeff.data_ptr(), result.data_ptr()))
            return result
        dev = torch.device("cuda", self.device)
        w, c, r = (torch.from_numpy(_f32(a)).to(dev) for a in (weights, coeff, result))
        self.use_torch_stream()
        _lib.check(self._L.colnde_ensemble_causal_penalty_dev(self._h, w.data_ptr(), c.data_ptr(), r.data_ptr()))
        return r.cpu().numpy()

    def pretrain_flux(self, theta, m, v, T, bcs, fluxes, order, coeff, opt_kind, etas, beta=(0.9, 0.999), eps: float = 1e-8, beta_t=None, update: bool = True):
        """`colnde_ensemble_pretrain_flux_dev`: one `Flux.train!` pass of the T -> wT pre-training (train_free_convection_nde.jl:182-216) for all K
        networks in one launch, over device tensors: theta, m, v [K, n_params] (updated in place), T [n, Nz], bcs [n, 2], fluxes [n, Nz + 1], order
        [K, n] int32 or None (0..n-1 for every model), coeff [K] or None (the soft spatial-causality penalty c_k sum(abs2, W1[mask])), etas [K].
        opt_kind "adam" | "descent" (or 0 | 1); under "descent" m and v may be None and beta_t stays.  beta_t: a list [beta1^t, beta2^t] advanced in place
        by n steps (ADAM with update; None: a fresh optimiser's).  update=False: nothing is written, the mean loss at the given weights.
        Returns the K mean losses (NumPy): with update, the mean of each sample's loss just before its own update."""
        kind = FC_PRETRAIN_OPTIMISERS.get(opt_kind, opt_kind) if isinstance(opt_kind, str) else opt_kind
        if kind not in (0, 1):
            raise ValueError("opt_kind: 'adam' (0) or 'descent' (1), got %r" % (opt_kind,))
        adam = kind == 0
        if update and etas is None:
            raise ValueError("the rates etas [K] are needed when update=True")
        if update and adam and (m is None or v is None):
            raise ValueError("the ADAM moments m and v are needed when update=True under 'adam'")
        n = check_fc_pretrain_arrays(self.cfg, self.n_models, theta, T, bcs, fluxes, order, coeff, etas, m if adam else None, v if adam else None, conv=self.conv)
        K, P, Nz = self.n_models, self.n_params, self.cfg.Nz
        for t, shape in ((theta, (K, P)), (T, (n, Nz)), (bcs, (n, 2)), (fluxes, (n, Nz + 1)), (coeff, (K,)), (etas, (K,))) + (((m, (K, P)), (v, (K, P))) if adam else ()):
            if t is not None:
                self._chk_dev(t, shape)
        if order is not None and not (order.is_cuda and order.is_contiguous() and order.device.index == self.device):
            raise ValueError("order must be a contiguous int32 tensor on the handle's device")
        if beta_t is None:
            beta_t = [float(beta[0]), float(beta[1])]
        P_ = lambda a: a.data_ptr() if a is not None else None
        self.use_torch_stream()
        bt = (ctypes.c_double * 2)(float(beta_t[0]), float(beta_t[1]))
        loss = (ctypes.c_float * K)()
        _lib.check(self._L.colnde_ensemble_pretrain_flux_dev(self._h, P_(theta), P_(m) if adam else None, P_(v) if adam else None, P_(T), P_(bcs), P_(fluxes),
                                                             P_(order), n, P_(coeff), int(kind), P_(etas), float(beta[0]), float(beta[1]), float(eps), bt,
                                                             int(bool(update)), loss))
        if update and adam:
            beta_t[0], beta_t[1] = bt[0], bt[1]
        return np.array(loss, dtype=np.float32)

    def set_physics(self, physics):
        _lib.check(self._L.colnde_ensemble_set_physics(self._h, _ptr(_f32(np.asarray(physics)))))


def check_closure_arrays(n_sets: int, params=None, out=None):
    """Shape and type checks of a closure handle's per-set arrays (no GPU needed): params [K, 5] (PHYSICS_KEYS order), out [K, 13].  NumPy arrays are
    converted to float32 by the callers; a torch tensor must already be a contiguous float32 device tensor (the `_dev` calls read it in place)."""
    K = int(n_sets)
    if K < 1:
        raise ValueError("n_sets must be >= 1, got %d" % K)
    for name, a, shape in (("params", params, (K, CLOSURE_N_PARAMS)), ("out", out, (K, CLOSURE_N_PARAMS + 8))):
        if a is None:
            continue
        if tuple(a.shape) != shape:
            raise ValueError("%s: expected shape %s for %d sets, got %s" % (name, shape, K, tuple(a.shape)))
        if _is_torch(a):
            import torch
            if a.dtype != torch.float32 or not a.is_contiguous() or not a.is_cuda:
                raise ValueError("%s: expected a contiguous float32 device tensor, got %s on %s" % (name, a.dtype, a.device))


def closure_min_substeps(cfg: NDEConfig, params) -> int:
    """`colnde_closure_min_substeps`: the RK4 stability bound for the five constants (nu0, nu_minus, dRi, Ric, Pr); no GPU needed."""
    c, keep = to_c_config(cfg, 1, 0, 0)
    p = (ctypes.c_float * 5)(*[float(x) for x in params])
    n = _lib.lib().colnde_closure_min_substeps(ctypes.byref(c), p)
    if n < 0:
        raise _lib.ColndeError(_lib.lib().colnde_last_error().decode("utf-8", "replace"))
    return int(n)


class ClosureColumns(ColumnNDE):
    """The column model WITHOUT networks (`colnde_create_closure`): K sets of the five Pacanowski-Philander constants solved, scored and differentiated
    side by side — `DE` / `loss_mpp` of wind_mixing/src/diffusivity_parameter_optimisation.jl.  params: [K, 5] = (nu0, nu_minus, dRi, Ric, Pr) per set.
    NumPy inputs go through the host entry points (which check every set's stability bound), torch device tensors through the `_dev` twins on torch's
    current stream.  The calls of `ColumnNDE` that take a weight vector are refused by the library on this handle."""

    def __init__(self, cfg: NDEConfig, n_columns: int, n_sets: int = 1, device: int = 0):
        check_closure_arrays(n_sets)
        self.cfg = cfg
        self.n_columns = int(n_columns)
        self.n_sets = self.n_models = int(n_sets)
        self.device = int(device)
        self._h = ctypes.c_void_p()
        L = _lib.lib()
        c, keep = to_c_config(cfg, n_columns, device, 0)
        _lib.check(L.colnde_create_closure(ctypes.byref(c), self.n_sets, ctypes.byref(self._h)))
        self._L = L
        self.n_params = L.colnde_n_params(self._h)
        assert self.n_params == CLOSURE_N_PARAMS and L.colnde_n_models(self._h) == self.n_sets
        self.n_columns_total = self.n_columns
        self.engine = "closure"

    def _params_dev(self, params):
        import torch
        check_closure_arrays(self.n_sets, params=params if _is_torch(params) else np.asarray(params))
        if _is_torch(params):
            self._chk_dev(params, (self.n_sets, CLOSURE_N_PARAMS))
            return params, True
        p = _f32(params, (self.n_sets, CLOSURE_N_PARAMS))
        return torch.from_numpy(p).to(torch.device("cuda", self.device)), False

    def forward(self, params, out=None):
        """sol [K, n_columns, n_save, 3 Nz]: a torch tensor for torch params, NumPy for NumPy params."""
        c = self.cfg
        shape = (self.n_sets, self.n_columns, c.n_save, c.n_state)
        if _is_torch(params):
            import torch
            p, _ = self._params_dev(params)
            sol = out if out is not None else torch.empty(shape, dtype=torch.float32, device=p.device)
            self._chk_dev(sol, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_closure_forward_dev(self._h, p.data_ptr(), sol.data_ptr()))
            return sol
        check_closure_arrays(self.n_sets, params=np.asarray(params))
        p = _f32(params, (self.n_sets, CLOSURE_N_PARAMS))
        sol = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_closure_forward(self._h, _ptr(p), _ptr(sol)))
        return sol

    def loss(self, params, scalings: Sequence[float]):
        """[K, 8] = [scaled terms(6); total; 0] per set."""
        import torch
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        p, is_t = self._params_dev(params)
        out = torch.empty((self.n_sets, 8), dtype=torch.float32, device=p.device)
        self.use_torch_stream()
        _lib.check(self._L.colnde_closure_loss_dev(self._h, p.data_ptr(), sc, out.data_ptr()))
        return out if is_t else out.cpu().numpy()

    def loss_grad(self, params, scalings: Sequence[float], out=None):
        """[K, 13]: per set [dL/dnu0, dL/dnu_minus, dL/ddRi, dL/dRic, dL/dPr; scaled terms(6); total; 0]."""
        sc = (ctypes.c_float * 6)(*[float(s) for s in scalings])
        shape = (self.n_sets, CLOSURE_N_PARAMS + 8)
        if _is_torch(params):
            import torch
            p, _ = self._params_dev(params)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=p.device)
            check_closure_arrays(self.n_sets, out=out)
            self._chk_dev(out, shape)
            self.use_torch_stream()
            _lib.check(self._L.colnde_closure_loss_grad_dev(self._h, p.data_ptr(), sc, out.data_ptr()))
            return out
        check_closure_arrays(self.n_sets, params=np.asarray(params))
        p = _f32(params, (self.n_sets, CLOSURE_N_PARAMS))
        res = np.empty(shape, dtype=np.float32)
        _lib.check(self._L.colnde_closure_loss_grad(self._h, _ptr(p), sc, _ptr(res)))
        return res
