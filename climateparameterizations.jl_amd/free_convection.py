"""Host-side mirror of the reference's free-convection NDE interface (`FreeConvection` package).

    FreeConvectionNDE / ConvectiveAdjustmentNDE(NN, ds; iterations)     free_convection/src/free_convection_nde.jl:1-47,
                                                                        convective_adjustment_nde.jl:1-57   -> FreeConvectionNDE class
    FreeConvectionNDEParameters(ds, T_scaling, wT_scaling)               free_convection_nde.jl:49-62        -> nde_params rows [bottom, top]
    solve_nde(nde, NN, T₀, alg, nde_params)                              free_convection/src/solve.jl:1-6
    solve_nde(ds, NN, NDEType, algorithm, T_scaling, wT_scaling) -> (T, wT)  free_convection/src/solve.jl:8-51 -> solve_nde_dataset
    nde_loss()  and the Flux.train! loop                                  free_convection/src/training.jl:44-74
    compute_neural_network_forcing!                                       free_convection/double_gyre_nn.jl:149-168
    convective_adjustment!(model, Δt, K)                                  free_convection/double_gyre_nn.jl:27-62, src/oceananigans_nn.jl:13-40
    progress_neural_network(simulation), diagnose_wT_NN(model)            free_convection/src/oceananigans_nn.jl:153-165, :100-118

The Oceananigans `FieldDataset` wrangling and DataDeps download stay outside (network + foreign types).
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np

from .config import NDEConfig, FREE_CONVECTION, CONVECTIVE_ADJUSTMENT_NDE
from .flux_compat import ADAM
from .nde import ColumnNDE


# ---- the `--conv c` network (train_free_convection_nde.jl:50-53, 110-122): pure NumPy, no GPU ------------------------------------------------------
#   Chain(reshape, Conv((c, 1), 1 => 1, relu), reshape, Dense(M, 4Nz, relu), Dense(4Nz, 4Nz, relu), Dense(4Nz, Nz-1)),   M = Nz - c + 1
#   θ = [w (c); b (1); vec(W1) (4Nz x M, column-major); b1; vec(W2); b2; vec(W3); b3]      (Flux.params order)
#   y[i] = relu(b + Σ_k w[k] x[i + c - k])  (NNlib's conv flips the kernel) = relu(b + Σ_j T[i, j] x[j]) with the Toeplitz T[i, i + d] = w[c - d]

def conv_n_params(Nz: int, c: int) -> int:
    M = Nz - c + 1
    return c + 1 + 4 * Nz * M + 4 * Nz + 16 * Nz * Nz + 4 * Nz + 4 * Nz * (Nz - 1) + Nz - 1


def conv_dense_layer_sizes(Nz: int, c: int):
    """The four-layer dense network `conv_to_dense` writes: relu, relu, relu, identity."""
    return (Nz, Nz - c + 1, 4 * Nz, 4 * Nz, Nz - 1)


def conv_to_dense(theta, Nz: int, c: int):
    """θ of the `--conv c` network -> θ of the equivalent four-layer dense network `conv_dense_layer_sizes(Nz, c)` whose first layer is the
    M x Nz Toeplitz matrix of the filter with the bias b on every row (Flux.destructure order: vec(W0) column-major, b0, then the rest)."""
    theta = np.asarray(theta)
    if theta.shape != (conv_n_params(Nz, c),):
        raise ValueError("theta: expected %d entries for Nz = %d, conv = %d, got %s" % (conv_n_params(Nz, c), Nz, c, theta.shape))
    M = Nz - c + 1
    W0 = np.zeros((M, Nz), dtype=theta.dtype)
    i = np.arange(M)
    for d in range(c):
        W0[i, i + d] = theta[c - 1 - d]
    b0 = np.full(M, theta[c], dtype=theta.dtype)
    return np.concatenate([W0.reshape(-1, order="F"), b0, theta[c + 1:]])


def conv_grad_from_dense(g, Nz: int, c: int):
    """The gradient with respect to the dense θ of `conv_to_dense` folded back onto the `--conv` θ: ∂W0 summed along its diagonals, ∂b0 over its
    entries, the rest appended."""
    g = np.asarray(g)
    M = Nz - c + 1
    if g.shape != (M * Nz + M + conv_n_params(Nz, c) - (c + 1),):
        raise ValueError("g: expected the gradient of the %s network, got %s" % (conv_dense_layer_sizes(Nz, c), g.shape))
    G0 = g[:M * Nz].reshape((M, Nz), order="F")
    i = np.arange(M)
    gw = np.array([G0[i, i + (c - 1 - k)].sum() for k in range(c)], dtype=g.dtype)
    gb = np.array([g[M * Nz:M * Nz + M].sum()], dtype=g.dtype)
    return np.concatenate([gw, gb, g[M * Nz + M:]])


class FreeConvectionNDE:
    """One NDE per simulation in the reference (`ndes[id]`); here all simulations are columns of one handle."""

    def __init__(self, cfg: NDEConfig, T0, nde_params, true_sols=None, device: int = 0,
                 causal_penalty: Optional[Callable] = None, conv: int = 0, matrix_arithmetic="bf16x3_exact"):
        """`causal_penalty`: the optional term of `nde_loss` (training.jl:44,57-58: `Flux.mse(...) + causal_penalty(NN)`), a
        function of the weights alone; here a callable θ -> (value, ∂value/∂θ) since there is no Zygote to differentiate it.
        `conv` = c > 1: the driver's `--conv c` network; cfg stays the plain (Nz, 4Nz, 4Nz, Nz-1) configuration and the weights are the
        `conv_n_params(Nz, c)` entries of Flux.params(NN).  solve_nde, nde_loss, nde_loss_and_grad and both training loops work unchanged."""
        if cfg.model not in (FREE_CONVECTION, CONVECTIVE_ADJUSTMENT_NDE):
            raise ValueError("need a free-convection config")
        self.cfg = cfg
        self.conv = int(conv)
        self.causal_penalty = causal_penalty
        T0 = np.ascontiguousarray(T0, dtype=np.float32)
        self.n_simulations = T0.shape[0]
        self.engine = ColumnNDE(cfg, self.n_simulations, device=device, conv=self.conv, matrix_arithmetic=matrix_arithmetic)
        self.engine.set_problem(T0, np.ascontiguousarray(nde_params, dtype=np.float32), true_sols)

    def dTdt(self, T, p, t=0.0):
        """`∂T∂t(T, p, t)` with p = [weights; bottom_flux, top_flux, σ_T, σ_wT, H, τ] (free_convection_nde.jl:29-38);
        the four trailing scalars must equal the config's (they are compile-time constants of the handle)."""
        p = np.asarray(p, dtype=np.float32)
        n = self.cfg.n_params
        tail = p[n:]
        c = self.cfg
        expect = np.array([c.sigma[2], c.sigma[5], c.H, c.tau], dtype=np.float32)
        if tail.shape[0] != 6 or not np.allclose(tail[2:], expect, rtol=1e-6):
            raise ValueError("p tail must be [bottom, top, σ_T, σ_wT, H, τ] matching the handle's configuration")
        T2 = np.atleast_2d(np.asarray(T, dtype=np.float32))
        out = self.engine.rhs(T2, p[:n], np.broadcast_to(tail[None, :2], (T2.shape[0], 2)), float(t))
        return out[0] if np.ndim(T) == 1 else out

    def solve_nde(self, weights):
        """`solve(nde, alg; reltol=1e-4, u0=T₀, p=[w; nde_params])` per simulation → [n_sims, Nz, Nt]."""
        return np.transpose(self.engine.forward(weights), (0, 2, 1))

    def nde_loss(self, weights) -> float:
        """`Flux.mse(cat(nde_sols…), true_sols)` (training.jl:55-62)."""
        total, _ = self.engine.loss(weights, [0, 0, 1, 0, 0, 0])
        if self.causal_penalty is not None:
            total += float(self.causal_penalty(np.asarray(weights, dtype=np.float32))[0])
        return total

    def nde_loss_and_grad(self, weights):
        total, _, grad = self.engine.loss_grad(weights, [0, 0, 1, 0, 0, 0])
        if self.causal_penalty is not None:
            pv, pg = self.causal_penalty(np.asarray(weights, dtype=np.float32))
            total, grad = total + float(pv), grad + np.asarray(pg, dtype=grad.dtype)
        return total, grad

    def close(self):
        self.engine.close()


def train_neural_differential_equation(nde: FreeConvectionNDE, weights, opt: ADAM, epochs: int,
                                       cb: Optional[Callable] = None):
    """`Flux.train!(nde_loss, Flux.params(NN), repeated((), epochs), opt, cb)` (training.jl:71)."""
    theta = np.array(weights, dtype=np.float32)
    history: List[float] = []
    for _ in range(epochs):
        total, grad = nde.nde_loss_and_grad(theta)
        history.append(total)
        opt.update(theta, grad.astype(np.float64))
        if cb is not None:
            cb(theta, total)
    return theta, history


def solve_nde_dataset(engine: ColumnNDE, weights, nde_params):
    """Dataset-level `solve_nde(ds, NN, NDEType, algorithm, T_scaling, wT_scaling)` (free_convection/src/solve.jl:8-51) for every simulation of the
    handle (set_problem gave it T₀ and the scaled [bottom, top] fluxes `nde_params`): the solution at the save points and the flux re-evaluated at each
    of them — `wT_NN_n = [bottom; NN(T_n); top]`, minus `min(0, 10 ∂T/∂z)` for ConvectiveAdjustmentNDE (:32-46) — both UNSCALED
    (`inv(T_scaling).(T)`, `inv(wT_scaling).(wT)`).  Returns (T [n, Nt, Nz], wT [n, Nt, Nz + 1])."""
    c = engine.cfg
    sol = engine.forward(np.asarray(weights, np.float32))                       # [n, Nt, Nz], scaled
    n, nt, nz = sol.shape
    bc = np.repeat(np.asarray(nde_params, np.float32)[:, None, :2], nt, axis=1).reshape(n * nt, 2)
    wT = engine.flux(sol.reshape(n * nt, nz), weights, bc).reshape(n, nt, nz + 1)
    return c.sigma[2] * sol + c.mu[2], c.sigma[5] * wT + c.mu[5]


def compute_neural_network_dz_wT(engine: ColumnNDE, weights, T_interior, surface_flux, Lz: float):
    """What `compute_neural_network_forcing!` stores: `params.∂z_wT_NN .= ∂z_wT(wT)` (double_gyre_nn.jl:165), +∂z wT; the forcing function
    `neural_network_∂z_wT` negates it (:135) — `compute_neural_network_forcing` below returns that forcing."""
    T = np.asarray(T_interior, dtype=np.float32)
    nx, ny, nz = T.shape
    out = engine.infer_dz_wT(weights, T.reshape(nx * ny, nz), np.asarray(surface_flux, np.float32).reshape(-1), Lz)
    return out.reshape(nx, ny, nz)


def compute_neural_network_forcing(engine: ColumnNDE, weights, T_interior, surface_flux, Lz: float):
    """`compute_neural_network_forcing!` (double_gyre_nn.jl:149-168): T_interior [Nx, Ny, Nz] model units,
    surface_flux [Nx, Ny]; returns the T-forcing array −∂z wT of the same shape."""
    T = np.asarray(T_interior, dtype=np.float32)
    nx, ny, nz = T.shape
    out = engine.infer_forcing(weights, T.reshape(nx * ny, nz), np.asarray(surface_flux, np.float32).reshape(-1), Lz)
    return out.reshape(nx, ny, nz)


def convective_adjustment(engine: ColumnNDE, T_interior, dt: float, K: float, dz: float, halo_bottom=None, halo_top=None):
    """`convective_adjustment!(model, Δt, K)` (double_gyre_nn.jl:27-62; 1-D: src/oceananigans_nn.jl:13-40) on the T
    interior [Nx, Ny, Nz] (or [n, Nz]): returns Tⁿ⁺¹ of the same shape.  halo_bottom / halo_top [Nx, Ny]: the halo
    cells Oceananigans filled for T's boundary conditions (None: zero-gradient fill)."""
    T = np.asarray(T_interior, dtype=np.float32)
    shape = T.shape
    T2 = T.reshape(-1, shape[-1])
    hb = None if halo_bottom is None else np.asarray(halo_bottom, np.float32).reshape(-1)
    ht = None if halo_top is None else np.asarray(halo_top, np.float32).reshape(-1)
    return engine.convective_adjustment(T2, dt, dz, K, hb, ht).reshape(shape)


def _embed_args(T, top_flux, halos):
    T = np.asarray(T, dtype=np.float32)
    shape = T.shape
    T2 = T.reshape(-1, shape[-1])
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_flux, np.float32).reshape(-1), (T2.shape[0],)))
    if halos is not None:
        halos = tuple(None if a is None else np.asarray(a, np.float32).reshape(-1) for a in halos)
    return T2, shape, top, halos


def progress_neural_network(engine: ColumnNDE, weights, T, top_flux, Lz: float, dt: float, K: float, halos=None):
    """One iteration of `progress_neural_network` (src/oceananigans_nn.jl:153-165; per column of double_gyre_nn.jl:211-234): the stored
    `∂z_wT_NN` of T as given (:159-160), then `convective_adjustment!(model, Δt, K)` (:162), in one launch.  T [..., Nz] (k = 0 deepest,
    the units `compute_neural_network_dz_wT` takes), top_flux a scalar or one value per column, halos = None or (halo_bottom, halo_top) as
    `convective_adjustment`.  Returns (∂z_wT_NN, Tⁿ⁺¹) in T's shape; the forcing the ocean model applies is −∂z_wT_NN (:132)."""
    T2, shape, top, halos = _embed_args(T, top_flux, halos)
    dz_wT, T_new = engine.fc_embedded_step(weights, T2, top, Lz, dt, K, halos)
    return dz_wT.reshape(shape), T_new.reshape(shape)


def diagnose_wT_NN(engine: ColumnNDE, weights, T, top_flux, Lz: float, K: float, halos=None):
    """`diagnose_wT_NN(model)` (src/oceananigans_nn.jl:100-118): the total face flux wT_NN − κ ∂T/∂z on the Nz + 1 faces, κ = K where the
    face gradient is negative (the end faces from the halo cells).  Arguments as `progress_neural_network`; returns [..., Nz + 1]."""
    T2, shape, top, halos = _embed_args(T, top_flux, halos)
    return engine.fc_diagnose_wT(weights, T2, top, Lz, K, halos).reshape(shape[:-1] + (shape[-1] + 1,))


def _ens_embed_args(ens, T, top_flux, halos):
    K = int(getattr(ens, "n_models", 1))
    T = np.asarray(T, dtype=np.float32)
    shape = T.shape
    T3 = np.ascontiguousarray(T.reshape(K, -1, shape[-1]))
    n = T3.shape[1]
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_flux, np.float32).reshape(-1), (n,)))
    if halos is not None:
        halos = tuple(None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(K, n)) for a in halos)
    return T3, shape, top, halos


def ensemble_progress_neural_network(ens, weights, T, top_flux, Lz: float, dt: float, K: float, halos=None, diagnose: bool = False):
    """`progress_neural_network` (src/oceananigans_nn.jl:153-165) for the K members of a `FreeConvectionEnsemble` — plain or `--conv` — in one launch
    (`ColumnNDE.fc_embedded`); a single `ColumnNDE(cfg, n, conv=c)` is K = 1.  T [K, ..., Nz], each member its own state; top_flux a scalar or one
    value per column, shared by the members; halos = None or (halo_bottom, halo_top), each [K, ...] or None; weights [K, n_params] or None (the
    images of the previous call).  Returns (∂z_wT_NN, Tⁿ⁺¹) in T's shape — with diagnose=True also `diagnose_wT_NN` of the state as given,
    [K, ..., Nz + 1].  Row k is what `progress_neural_network` gives for a plain member k, bit for bit."""
    T3, shape, top, halos = _ens_embed_args(ens, T, top_flux, halos)
    r = ens.fc_embedded(weights, T3, top, Lz, K, dt, halos, step=True, faces=bool(diagnose))
    out = (r.dz_wT.reshape(shape), r.T_new.reshape(shape))
    return out + (r.faces.reshape(shape[:-1] + (shape[-1] + 1,)),) if diagnose else out


def ensemble_diagnose_wT_NN(ens, weights, T, top_flux, Lz: float, K: float, halos=None):
    """`diagnose_wT_NN(model)` (src/oceananigans_nn.jl:100-118) for the K members in one launch: [K, ..., Nz + 1].  Arguments as
    `ensemble_progress_neural_network`."""
    T3, shape, top, halos = _ens_embed_args(ens, T, top_flux, halos)
    return ens.fc_embedded(weights, T3, top, Lz, K, None, halos, step=False, faces=True).faces.reshape(shape[:-1] + (shape[-1] + 1,))


def train_neural_differential_equation_device(nde: FreeConvectionNDE, weights, opt: ADAM, epochs: int, process_group=None, comm=None):
    """`Flux.train!` (training.jl:71) with θ and the ADAM state resident on the GPU: per epoch one `colnde_loss_grad_dev`,
    [one SUM all-reduce when the simulations are sharded over `process_group`], one fused `colnde_adam_step_dev`.
    Returns (θ, loss history) like `train_neural_differential_equation`; the per-epoch callback is not available here."""
    import torch
    eng = nde.engine
    dev = torch.device("cuda", eng.device)
    n = eng.n_params
    theta = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous()
    out = torch.empty(n + 8, dtype=torch.float32, device=dev)
    m = torch.zeros(n, dtype=torch.float32, device=dev)
    v = torch.zeros(n, dtype=torch.float32, device=dev)
    if opt.m is not None:
        m.copy_(torch.as_tensor(opt.m, dtype=torch.float32)); v.copy_(torch.as_tensor(opt.v, dtype=torch.float32))
    hist = []
    for _ in range(epochs):
        eng.loss_grad(theta, [0, 0, 1, 0, 0, 0], out=out)
        if comm is not None:
            comm.allreduce_result(eng, out)
        elif process_group is not None:
            import torch.distributed as dist
            dist.all_reduce(out, op=dist.ReduceOp.SUM, group=process_group)
        hist.append(out[n + 6].clone())
        eng.adam_step(theta, out, m, v, opt.eta, opt.beta, opt.eps, beta_t=tuple(opt.beta_t))
        opt.beta_t[0] *= opt.beta[0]
        opt.beta_t[1] *= opt.beta[1]
    opt.m, opt.v = m.double().cpu().numpy(), v.double().cpu().numpy()
    history = [float(x) for x in torch.stack(hist).cpu().numpy()] if hist else []
    return theta.cpu().numpy(), history


# ---- ensembles: many networks on the same simulations (colnde_create_fc_ensemble) -----------------------------------------------------------------

def _fc_ensemble(cfg: NDEConfig, T0, nde_params, true_sols, W, device, matrix_arithmetic, conv=0):
    """Shape checks first (no handle is requested for arrays that do not fit), then the ensemble with its problem set."""
    from .nde import FreeConvectionEnsemble, check_fc_ensemble_arrays
    T0 = np.ascontiguousarray(T0, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    if T0.ndim != 2 or W.ndim != 2:
        raise ValueError("T0 must be [n_sims, Nz] and the weights [K, n_params], got %s and %s" % (T0.shape, W.shape))
    n, K = T0.shape[0], W.shape[0]
    check_fc_ensemble_arrays(cfg, n, K, weights=W, conv=conv)
    bcs = np.ascontiguousarray(nde_params, dtype=np.float32)
    if T0.shape != (n, cfg.Nz) or bcs.shape != (n, 2):
        raise ValueError("T0: expected [n_sims, %d], nde_params: [n_sims, 2] ([bottom, top]); got %s and %s" % (cfg.Nz, T0.shape, bcs.shape))
    truth = None if true_sols is None else np.ascontiguousarray(true_sols, dtype=np.float32)
    if truth is not None and truth.shape != (n, cfg.n_save, cfg.Nz):
        raise ValueError("true_sols: expected %s, got %s" % ((n, cfg.n_save, cfg.Nz), truth.shape))
    ens = FreeConvectionEnsemble(cfg, n, K, device=device, matrix_arithmetic=matrix_arithmetic, conv=conv)
    ens.set_problem(T0, bcs, truth)
    return ens, W


def train_neural_differential_equation_ensemble(T0, nde_params, true_sols, cfg: NDEConfig, W, etas, epochs: int, causal_coeff=None, device: int = 0,
                                                beta=(0.9, 0.999), eps: float = 1e-8, matrix_arithmetic="bf16x3_exact", conv: int = 0,
                                                training_simulations=None):
    """`train_neural_differential_equation!` (training.jl:44-74) for K networks at once — the sweep of train_free_convection_nde.jl (one process per
    seed, optimiser rate or `--spatial_causality` there) on the same simulations.  T0 [n_sims, Nz], nde_params [n_sims, 2] = [bottom, top],
    true_sols [n_sims, Nt, Nz] (scaled); W [K, n_params], etas [K]; causal_coeff [K] or None: model k trains on
    `Flux.mse(...) + c_k sum(abs2, W1[mask])` (train_free_convection_nde.jl:186-197; 1 is the reference's penalty, 0 none).  θ and the ADAM state stay
    on the device; per epoch one loss + gradient, one penalty add (with coefficients) and one ADAM step for all K.
    conv = c > 1: K `--conv c` networks, cfg the plain configuration, W [K, conv_n_params(Nz, c)]; the penalty masks the conv chain's first Dense weight.
    training_simulations: a list of K index lists — member k trains on its own simulations (`--training-simulations`,
    train_free_convection_nde.jl:60-66) through the member loss (`set_member_loss` with 0/1 column weights, `member_loss_grad`); every member is
    still solved on all simulations, and `nde_loss_history` gives the loss on those it did not train on.  None: the calls issued before.
    Returns (θ [K, n_params], loss history [epochs, K] — the penalty included, as `nde_loss` returns it)."""
    import torch
    from .nde import check_fc_ensemble_arrays
    from .wind_mixing import member_column_weights
    et = np.ascontiguousarray(etas, dtype=np.float32)
    cc = None if causal_coeff is None else np.ascontiguousarray(causal_coeff, dtype=np.float32)
    Wn = np.asarray(W)
    check_fc_ensemble_arrays(cfg, np.shape(T0)[0], Wn.shape[0] if Wn.ndim == 2 else 0, weights=Wn, etas=et, coeff=cc, conv=conv)
    ens, Wc = _fc_ensemble(cfg, T0, nde_params, true_sols, W, device, matrix_arithmetic, conv)
    try:
        dev = torch.device("cuda", ens.device)
        K, n = ens.n_models, ens.n_params
        theta = torch.from_numpy(Wc).to(dev).contiguous()
        eta_d = torch.from_numpy(et).to(dev)
        cc_d = None if cc is None else torch.from_numpy(cc).to(dev)
        out = torch.empty((K, n + 8), dtype=torch.float32, device=dev)
        m = torch.zeros((K, n), dtype=torch.float32, device=dev)
        v = torch.zeros((K, n), dtype=torch.float32, device=dev)
        bt = [beta[0], beta[1]]
        hist = []
        member = training_simulations is not None
        if member:
            ens.set_member_loss(np.tile(np.array([0, 0, 1, 0, 0, 0], np.float32), (K, 1)), member_column_weights(K, ens.n_columns, training_simulations))
        for _ in range(epochs):
            if member:
                ens.member_loss_grad(theta, out=out)
            else:
                ens.loss_grad(theta, [0, 0, 1, 0, 0, 0], out=out)
            if cc_d is not None:
                ens.causal_penalty(theta, cc_d, out)
            hist.append(out[:, n + 6].clone())
            ens.adam_step(theta, out, m, v, eta_d, beta, eps, beta_t=tuple(bt))
            bt[0] *= beta[0]
            bt[1] *= beta[1]
        history = torch.stack(hist).cpu().numpy() if hist else np.zeros((0, K), np.float32)
        return theta.cpu().numpy(), history
    finally:
        ens.close()


def compute_nde_solution_history(T0, nde_params, cfg: NDEConfig, W_history, device: int = 0, matrix_arithmetic="bf16x3_exact", conv: int = 0):
    """`compute_nde_solution_history` (free_convection/src/testing.jl:1-32): the NDE re-solved for the network of EVERY epoch on every simulation —
    one forward call for all E networks.  W_history [E, n_params]; returns T [E, n_sims, Nz, Nt], unscaled (`inv(T_scaling)`).  conv = c > 1: the
    `--conv c` networks of a run trained with that switch."""
    ens, Wc = _fc_ensemble(cfg, T0, nde_params, None, W_history, device, matrix_arithmetic, conv)
    try:
        sol = ens.forward(Wc)                                                    # [E, n, Nt, Nz], scaled
    finally:
        ens.close()
    return np.transpose(cfg.sigma[2] * sol + cfg.mu[2], (0, 1, 3, 2))


def nde_loss_history(T0, nde_params, true_sols, cfg: NDEConfig, W_history, device: int = 0, matrix_arithmetic="bf16x3_exact", conv: int = 0):
    """What `plot_epoch_loss` and `animate_nde_loss` plot (testing.jl:34-105), in scaled units: per epoch and simulation `Flux.mse(true, nde)`
    ([E, n_sims]) and `Flux.mse(true, nde, agg = x -> mean(x, dims=1))` per save time ([E, n_sims, Nt]).  One forward call and one column-loss
    call for all E networks; the first is the mean of the second over the save times."""
    import torch
    ens, Wc = _fc_ensemble(cfg, T0, nde_params, true_sols, W_history, device, matrix_arithmetic, conv)
    try:
        sol = ens.forward(torch.from_numpy(Wc).to(torch.device("cuda", ens.device)))
        per_t = ens.column_loss(sol).cpu().numpy()
    finally:
        ens.close()
    return per_t.astype(np.float64).mean(axis=2).astype(np.float32), per_t


# ---- T -> wT pre-training of a whole sweep (train_free_convection_nde.jl:182-216) --------------------------------------------------------------------

def pretrain_orders(seeds, n: int, n_passes: int):
    """The sample orders of `train_neural_network_ensemble`: [n_passes, K, n] int32 — model k draws a fresh permutation of 0..n-1 per pass from
    `numpy.random.default_rng(seeds[k])` (`Flux.train!` over the shuffled data set; the reference's process k seeds its own shuffle)."""
    rngs = [np.random.default_rng(int(s)) for s in seeds]
    return np.stack([np.stack([r.permutation(n) for r in rngs]) for _ in range(n_passes)]).astype(np.int32) if n_passes else np.zeros((0, len(rngs), n), np.int32)


def train_neural_network_ensemble(ens, W, T, bcs, wT, etas=None, epochs: int = 10, optimizers=(("adam", 1e-3), ("descent", 1e-2)), causal_coeff=None,
                                  seeds=None, beta=(0.9, 0.999), eps: float = 1e-8):
    """The driver's pre-training loop `for opt in optimizers, e in 1:epochs; Flux.train!(loss, ps, data, opt, cb = nn_callback)`
    (train_free_convection_nde.jl:198-216) for the K networks of `ens` (a `FreeConvectionEnsemble`, plain or conv — the handle that then trains the
    NDE) at once: one `pretrain_flux` launch per epoch, one optimiser update per sample and model, each model walking its own fresh permutation
    (`pretrain_orders(seeds, n, passes)`; seeds None: 0..K-1).  W [K, n_params]; T [n, Nz], bcs [n, 2] = [bottom, top], wT [n, Nz + 1], scaled.
    optimizers: (kind, rate) pairs, "adam" | "descent"; an ADAM's moments and running powers start afresh with it and carry across its epochs.
    etas: None (every model takes each optimiser's rate) or [len(optimizers), K] per-model rates.  causal_coeff [K] or None: model k's loss is
    mse([bottom; NN(T); top], wT) + c_k sum(abs2, W1[mask]).
    Returns (theta [K, n_params], history [passes, K]): after each pass the loss over the training set at the weights it left (`nn_callback`)."""
    import torch
    from .nde import FC_PRETRAIN_OPTIMISERS, check_fc_pretrain_arrays
    K = ens.n_models
    Wn = np.ascontiguousarray(W, dtype=np.float32)
    Tn, Bn, Yn = (np.ascontiguousarray(a, dtype=np.float32) for a in (T, bcs, wT))
    cc = None if causal_coeff is None else np.ascontiguousarray(causal_coeff, dtype=np.float32)
    kinds = []
    for kind, _ in optimizers:
        if kind not in FC_PRETRAIN_OPTIMISERS:
            raise ValueError("optimizers: kinds are 'adam' and 'descent', got %r" % (kind,))
        kinds.append(kind)
    if etas is None:
        et = np.array([[rate] * K for _, rate in optimizers], dtype=np.float32).reshape(len(kinds), K)
    else:
        et = np.ascontiguousarray(etas, dtype=np.float32)
        if et.shape != (len(kinds), K):
            raise ValueError("etas: expected shape %s (one row of per-model rates per optimiser), got %s" % ((len(kinds), K), et.shape))
    if int(epochs) < 0:
        raise ValueError("epochs must be >= 0")
    seeds = list(range(K)) if seeds is None else list(seeds)
    if len(seeds) != K:
        raise ValueError("seeds: expected %d entries (one per model), got %d" % (K, len(seeds)))
    n_passes = len(kinds) * int(epochs)
    n = check_fc_pretrain_arrays(ens.cfg, K, Wn, Tn, Bn, Yn, coeff=cc, conv=ens.conv)
    orders = pretrain_orders(seeds, n, n_passes)
    if n_passes:
        check_fc_pretrain_arrays(ens.cfg, K, Wn, Tn, Bn, Yn, order=orders[0], conv=ens.conv)
    dev = torch.device("cuda", ens.device)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev).contiguous()
    theta, Td, Bd, Yd, cd = up(Wn.copy()), up(Tn), up(Bn), up(Yn), up(cc)
    history = np.zeros((n_passes, K), np.float32)
    p = 0
    for i, kind in enumerate(kinds):
        adam = kind == "adam"
        m = torch.zeros_like(theta) if adam else None
        v = torch.zeros_like(theta) if adam else None
        bt = [float(beta[0]), float(beta[1])]
        eta_d = up(et[i])
        for _ in range(int(epochs)):
            ens.pretrain_flux(theta, m, v, Td, Bd, Yd, up(orders[p]), cd, kind, eta_d, beta, eps, bt, update=True)
            history[p] = ens.pretrain_flux(theta, None, None, Td, Bd, Yd, None, cd, kind, None, beta, eps, bt, update=False)
            p += 1
    return theta.cpu().numpy(), history
