"""Host-side mirror of the reference's wind-mixing NDE interface (`WindMixing` package), over the HIP engine.

Same names, argument meaning and return shapes as the Julia closures this path replaces:

    NDE(x, p, t)                     wind_mixing/src/NDE_training.jl:56-81      out-of-place RHS, p = [weights; BCs]
    NDE!(dx, x, p, t)  -> NDE_inplace  wind_mixing/src/training_postprocessing.jl:131-153
    solve_NDE_nonmutating / solve_NDE_mutating                                NDE_training.jl:376-406, training_postprocessing.jl:55-159
    loss_NDE(weights, BCs), loss_gradient_NDE(weights, BCs)                   NDE_training.jl:290-323
        -> (total, scaled_losses{u,v,T,∂u∂z,∂v∂z,∂T∂z}, loss_scalings)
    ∇loss  -> grad_loss(weights)      the pullback GalacticOptim obtains from Zygote (NDE_training.jl:327-333)
    calculate_loss_scalings, apply_loss_scalings                               wind_mixing/src/loss.jl:11-42
    train_NDE                                                                  NDE_training.jl:167-374 (optimiser loop :340-372)
    modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment)   wind_mixing/src/NDE_oceananigans.jl:61-101
        -> modified_pacanowski_philander_step   (implicit diffusion step of the 1-D ocean embedding)

Data loading, JLD2 logging and plotting stay outside (out of scope).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from .config import NDEConfig, WIND_MIXING
from .flux_compat import ADAM
from .nde import ColumnNDE

LOSS_KEYS = ("u", "v", "T", "dudz", "dvdz", "dTdz")


def calculate_loss_scalings(losses, fractions, train_gradient: bool):
    """wind_mixing/src/loss.jl:11-31.  `losses` in LOSS_KEYS order; `fractions` = dict(T, dTdz, profile)."""
    Lu, Lv, LT, Lgu, Lgv, LgT = [float(x) for x in losses]
    vel = (1 - fractions["T"]) / fractions["T"] * LT / (Lu + Lv)
    profile_loss = vel * (Lu + Lv) + LT
    if train_gradient:
        velg = (1 - fractions["dTdz"]) / fractions["dTdz"] * LgT / (Lgu + Lgv)
        gradient_loss = velg * (Lgu + Lgv) + LgT
        tot = (1 - fractions["profile"]) / fractions["profile"] * profile_loss / gradient_loss
    else:
        velg = tot = 0.0
    return np.array([vel, vel, 1.0, tot * velg, tot * velg, tot], dtype=np.float64)


def apply_loss_scalings(losses, scalings):
    """wind_mixing/src/loss.jl:33-42."""
    return {k: float(s) * float(l) for k, s, l in zip(LOSS_KEYS, scalings, losses)}


@dataclass
class TrainResult:
    weights: np.ndarray
    history: List[dict]
    schedule: Optional[tuple] = None             # train_NDE_ensemble(schedule="choose"): the counts chosen for all K members ...
    schedule_estimate: Optional[float] = None    # ... and this member's own error estimate at them


class WindMixingNDE:
    """The closures `train_NDE` builds (NDE_training.jl:252-323) for one set of simulations (columns)."""

    def __init__(self, cfg: NDEConfig, uvT0, BCs, uvT_trains=None, device: int = 0,
                 gradient_scaling: float = 5e-3, training_fractions: Optional[dict] = None,
                 weights0=None, matrix_arithmetic: str = "bf16x3_exact"):
        if cfg.model != WIND_MIXING:
            raise ValueError("WindMixingNDE needs a wind-mixing config")
        self.cfg = cfg
        uvT0 = np.ascontiguousarray(uvT0, dtype=np.float32)
        self.n_simulations = uvT0.shape[0]
        self.BCs = np.ascontiguousarray(BCs, dtype=np.float32)
        self.engine = ColumnNDE(cfg, self.n_simulations, device=device, matrix_arithmetic=matrix_arithmetic)
        self.engine.set_problem(uvT0, self.BCs, uvT_trains)
        self.uvT0, self.uvT_trains = uvT0, uvT_trains          # (train_NDE_ensemble hands the same problem to an ensemble handle)
        self._rhs_engine = None
        # determine_loss_scalings (NDE_training.jl:256-288)
        if training_fractions is None:
            g = gradient_scaling if cfg.train_gradient else 0.0
            self.loss_scalings = np.array([1, 1, 1, g, g, g], dtype=np.float64)
        else:
            if weights0 is None:
                raise ValueError("training_fractions needs the initial weights (one forward solve, NDE_training.jl:260)")
            _, terms = self.engine.loss(weights0, [1, 1, 1, 1, 1, 1] if cfg.train_gradient else [1, 1, 1, 0, 0, 0])
            self.loss_scalings = calculate_loss_scalings(terms, training_fractions, cfg.train_gradient)

    # ---- RHS closures ---------------------------------------------------------------------------------
    def _split_p(self, p):
        p = np.asarray(p, dtype=np.float32)
        n = self.cfg.n_params
        if p.shape[-1] != n + 6:
            raise ValueError("p must be [weights(%d); uw_b, uw_t, vw_b, vw_t, wT_b, wT_t]" % n)
        return p[..., :n], p[..., n:]

    def NDE(self, x, p, t):
        """Out-of-place `NDE(x, p, t)`; x: [3Nz] (or [n, 3Nz] with p: [n_params+6] shared weights per row of BCs)."""
        w, bc = self._split_p(p)
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float32))
        bc2 = np.broadcast_to(np.atleast_2d(bc), (x2.shape[0], 6))
        dx = self.engine.rhs(x2, w if w.ndim == 1 else w[0], bc2, float(t))
        return dx[0] if np.ndim(x) == 1 else dx

    def NDE_inplace(self, dx, x, p, t):
        """`NDE!(dx, x, p, t)`: the evaluation RHS arithmetic (no ϵ in Ri; training_postprocessing.jl:105-153)."""
        if self._rhs_engine is None:
            self._rhs_engine = ColumnNDE(self.cfg.with_(inplace_variant=True), 1, device=self.engine.device)
        w, bc = self._split_p(p)
        x2 = np.atleast_2d(np.asarray(x, dtype=np.float32))
        bc2 = np.broadcast_to(np.atleast_2d(bc), (x2.shape[0], 6))
        out = self._rhs_engine.rhs(x2, w, bc2, float(t))
        dx[...] = out[0] if np.ndim(x) == 1 else out
        return None

    # ---- solves ---------------------------------------------------------------------------------------
    def solve_NDE_nonmutating(self, weights):
        """`[Array(solve(prob_NDEs[i], …; p=[weights; BCs[i]], saveat=t_train)) for i in 1:n_simulations]`
        (NDE_training.jl:403).  Returns [n_sims, 3Nz, Nt] — each `sols[i]` is the reference's 96×Nt array."""
        return np.transpose(self.engine.forward(weights), (0, 2, 1))

    # ---- losses ---------------------------------------------------------------------------------------
    def loss_NDE(self, weights, BCs=None):
        sc = self.loss_scalings.copy()
        sc[3:] = 0.0                      # loss_NDE zeroes the gradient terms (NDE_training.jl:298)
        total, terms = self.engine.loss(weights, sc)
        return total, dict(zip(LOSS_KEYS, [float(t) for t in terms])), dict(zip(LOSS_KEYS, sc))

    def loss_gradient_NDE(self, weights, BCs=None):
        total, terms = self.engine.loss(weights, self.loss_scalings)
        return total, dict(zip(LOSS_KEYS, [float(t) for t in terms])), dict(zip(LOSS_KEYS, self.loss_scalings))

    def grad_loss(self, weights):
        """∇loss: value and gradient of `first(loss(θ, BCs))` w.r.t. θ — what AutoZygote hands GalacticOptim."""
        sc = self.loss_scalings.copy()
        if not self.cfg.train_gradient:
            sc[3:] = 0.0
        total, terms, grad = self.engine.loss_grad(weights, sc)
        return total, dict(zip(LOSS_KEYS, [float(t) for t in terms])), grad

    def close(self):
        self.engine.close()
        if self._rhs_engine is not None:
            self._rhs_engine.close()


def train_NDE(problem: WindMixingNDE, weights, optimizers: Sequence[ADAM], epochs: int = 1, maxiters: int = 500,
              cb: Optional[Callable] = None, continue_state: bool = False, schedule=None) -> TrainResult:
    """The optimiser loop of `train_NDE` (NDE_training.jl:340-372): for each optimiser and epoch one
    `res = solve(prob_loss, opt, cb=cb, maxiters=maxiters); weights .= res.minimizer`.

    That `solve` is GalacticOptim 1.2.0's Flux-optimiser `__solve` (third-party, pinned in wind_mixing/Manifest.toml, absent from
    /root/reference; restated from its published source, `tests/test_training_loops.py` holds the literal restatement):
      * it optimises `θ = copy(prob.u0)`, and Flux's ADAM keeps its state in an IdDict keyed by that array, so every
        (optimizer, epoch) solve starts from zero moments and βᵗ = β (`continue_state=True` carries them over instead);
      * per iteration: loss and gradient at θ, `cb(θ, total, losses, loss_scalings)` (true = stop), `update!(opt, θ, g)`,
        then `save_best`: if this iteration's loss is the lowest so far, `min_θ = copy(θ)` — taken AFTER the update, i.e. the
        point one ADAM step past the best-loss point; at `i == maxiters` θ reverts to `min_θ` and `cb(min_θ, min_err...)` is called once
        more, so a solve that is not halted issues maxiters + 1 callbacks.
    The reference's OWN callback ignores that extra call: its body is guarded by `if iter <= maxiters` with `iter += 1` behind it
    (NDE_training.jl:343-368), so it prints and `write_data_NDE_training`s exactly `maxiters` records per solve.  A `cb` that logs must carry
    the same guard to produce a reference-shaped log: `reference_logging_callback` below is that closure.
    schedule: RK4 steps per save interval for the problem's engine (`ColumnNDE.set_schedule`; before its first gradient), None: cfg.substeps."""
    if schedule is not None:
        problem.engine.set_schedule(schedule)
    theta = np.array(weights, dtype=np.float32)
    history = []
    for opt in optimizers:
        for _ in range(epochs):
            if not continue_state:
                opt.reset()
            best, best_losses, best_theta = np.inf, None, theta.copy()
            halted = False
            for it in range(maxiters):
                total, losses, grad = problem.grad_loss(theta)
                history.append(dict(total=total, **losses))
                if cb is not None and cb(theta, total, losses, problem.loss_scalings):
                    halted = True
                    break
                opt.update(theta, grad.astype(np.float64))
                if total < best:
                    best, best_losses, best_theta = total, losses, theta.copy()
            theta = best_theta
            # `if i == maxiters ... θ = min_θ; cb(θ, x...); break` — GalacticOptim's extra callback on the reverted best point (its return value is
            # ignored).  The reference's cb does nothing on it (`if iter <= maxiters`, NDE_training.jl:344): see reference_logging_callback
            if cb is not None and not halted and maxiters > 0 and best_losses is not None:
                cb(theta, best, best_losses, problem.loss_scalings)
    return TrainResult(theta, history)


def reference_logging_callback(FILE_PATH, cfg: NDEConfig, stage, opt: ADAM, maxiters: int, log: Optional[Callable] = None):
    """The `cb(args...)` closure `train_NDE` builds per (optimizer, epoch) solve (NDE_training.jl:342-368): while `iter <= maxiters` it writes one
    record — losses, loss scalings, the three networks cut out of θ, the optimiser state — through `write_data_NDE_training`
    (wind_mixing/src/data_writing.jl:28-78), then `iter += 1` and returns false.  The guard is what makes the (maxiters + 1)-th call of
    GalacticOptim's solve (the reverted best point) a no-op, so a log holds exactly `maxiters` records per solve and `extract_NN`'s
    `N_data` / arg-min see what they see in a reference log.  `log(iter, total, losses)`: optional hook in place of the reference's `@info`."""
    from .checkpoint import network_record, write_data_NDE_training
    state = {"iter": 1}
    third = cfg.n_params // 3

    def cb(theta, total, losses, loss_scalings):
        if state["iter"] <= maxiters:
            if log is not None:
                log(state["iter"], total, losses)
            th = np.asarray(theta, dtype=np.float32)
            nets = [network_record(th[k * third:(k + 1) * third], cfg.layer_sizes, cfg.activations) for k in range(3)]
            sc = dict(zip(LOSS_KEYS, [float(s) for s in loss_scalings])) if not isinstance(loss_scalings, dict) else loss_scalings
            write_data_NDE_training(FILE_PATH, losses, sc, nets[0], nets[1], nets[2], stage, opt)
        state["iter"] += 1
        return False
    return cb


def _check_replicas(theta, comm, process_group, it):
    from .distributed import weights_in_sync
    if comm is not None:
        red = lambda t: comm.allreduce(t, "max")
    else:
        import torch.distributed as dist
        red = lambda t: dist.all_reduce(t, op=dist.ReduceOp.MAX, group=process_group)
    ok, spread = weights_in_sync(theta, red)
    if not ok:
        raise RuntimeError("train_NDE_device: the ranks' weight vectors differ at iteration %d (checksum spread %.3e): the replicas "
                           "no longer apply identical updates" % (it, spread))


def train_NDE_device(problem: WindMixingNDE, weights, optimizers: Sequence[ADAM], epochs: int = 1, maxiters: int = 500,
                     process_group=None, continue_state: bool = False, comm=None, sync_check_every: int = 0, schedule=None) -> TrainResult:
    """`train_NDE`'s optimiser loop (NDE_training.jl:340-372) with θ, the ADAM state and the best-loss copy resident on the
    GPU: per iteration one `colnde_loss_grad_dev`, [one SUM all-reduce of the gradient buffer when the columns are sharded
    over `process_group`], one fused `colnde_adam_step_dev`; nothing crosses PCIe until the end.  Same update rule, per-solve
    state reset and `save_best` selection as `train_NDE`; the per-iteration callback is not available here.
    sync_check_every = K > 0 (sharded runs): every K iterations, and before the first, the ranks compare checksums of their weight vectors
    with one 12-float MAX all-reduce (`distributed.weights_in_sync`) and raise if the replicas have drifted apart.
    schedule: RK4 steps per save interval (`ColumnNDE.set_schedule`; sharded runs: the same on every rank — `distributed.agree_schedule`), None: cfg.substeps."""
    import torch
    eng = problem.engine
    if schedule is not None:
        eng.set_schedule(schedule)
    dev = torch.device("cuda", eng.device)
    n = eng.n_params
    theta = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous()
    out = torch.empty(n + 8, dtype=torch.float32, device=dev)
    sc = problem.loss_scalings.copy()
    if not problem.cfg.train_gradient:
        sc[3:] = 0.0
    hist = []
    for opt in optimizers:
        for _ in range(epochs):
            if not continue_state:
                opt.reset()
            m = torch.zeros(n, dtype=torch.float32, device=dev)
            v = torch.zeros(n, dtype=torch.float32, device=dev)
            if opt.m is not None:            # continue_state: the moments of the previous solve
                m.copy_(torch.as_tensor(opt.m, dtype=torch.float32)); v.copy_(torch.as_tensor(opt.v, dtype=torch.float32))
            best = torch.full((), float("inf"), dtype=torch.float32, device=dev)
            best_theta = theta.clone()
            for it in range(maxiters):
                if sync_check_every > 0 and it % sync_check_every == 0 and (comm is not None or process_group is not None):
                    _check_replicas(theta, comm, process_group, it)
                eng.loss_grad(theta, sc, out=out)
                if comm is not None:                       # colnde.distributed.Comm: RCCL behind the C ABI
                    comm.allreduce_result(eng, out)
                elif process_group is not None:
                    import torch.distributed as dist
                    dist.all_reduce(out, op=dist.ReduceOp.SUM, group=process_group)
                total = out[n + 6]
                hist.append(out[n:n + 7].clone())
                eng.adam_step(theta, out, m, v, opt.eta, opt.beta, opt.eps, beta_t=tuple(opt.beta_t))
                opt.beta_t[0] *= opt.beta[0]
                opt.beta_t[1] *= opt.beta[1]
                better = total < best
                best = torch.where(better, total, best)
                best_theta = torch.where(better, theta, best_theta)      # min_θ = copy(θ) AFTER update! (GalacticOptim save_best)
            theta = best_theta.clone()
            opt.m, opt.v = m.double().cpu().numpy(), v.double().cpu().numpy()
    H = torch.stack(hist).cpu().numpy() if hist else np.zeros((0, 7), np.float32)
    history = [dict(total=float(r[6]), **{k: float(r[i]) for i, k in enumerate(LOSS_KEYS)}) for r in H]
    return TrainResult(theta.cpu().numpy(), history)


def member_column_weights(n_models: int, n_simulations: int, training_simulations) -> np.ndarray:
    """The 0/1 column weights [K, n_simulations] of `training_simulations`: a list of K index lists, member k trains on its own (no GPU needed)."""
    ts = list(training_simulations)
    if len(ts) != n_models:
        raise ValueError("training_simulations: expected %d index lists (one per member), got %d" % (n_models, len(ts)))
    cw = np.zeros((n_models, n_simulations), dtype=np.float32)
    for k, idx in enumerate(ts):
        idx = [int(i) for i in idx]
        if not idx:
            raise ValueError("training_simulations[%d] is empty: every member needs at least one simulation" % k)
        if min(idx) < 0 or max(idx) >= n_simulations or len(set(idx)) != len(idx):
            raise ValueError("training_simulations[%d]: distinct indices in 0..%d, got %r" % (k, n_simulations - 1, idx))
        cw[k, idx] = 1.0
    return cw


def member_fractions(n_models: int, training_fractions):
    """`training_fractions` as a list of K dicts: one dict for all members, or a list of K (no GPU needed)."""
    if isinstance(training_fractions, dict):
        return [training_fractions] * n_models
    fr = list(training_fractions)
    if len(fr) != n_models or not all(isinstance(f, dict) for f in fr):
        raise ValueError("training_fractions: a dict for all members or a list of %d dicts" % n_models)
    return fr


def train_NDE_ensemble(problem: WindMixingNDE, weights, physics, etas, epochs: int = 1, maxiters: int = 500, beta=(0.9, 0.999),
                       eps: float = 1e-8, schedule=None, training_fractions=None, training_simulations=None,
                       gradient_scaling=None, reltol=None) -> List[TrainResult]:
    """`train_NDE_device`'s loop (NDE_training.jl:340-372: ADAM, per-solve state reset, save_best) for K models at once — the sweep of
    wind_mixing/train_NDE_args.jl, which trains one model per process with its own ADAM rate (ARGS[2], :143) and Pacanowski-Philander constants
    (ARGS[3], :175).  weights [K, n_params], physics [K, 5] = (nu0, nu_minus, dRi, Ric, Pr) per model or None (the problem's constants), etas [K].
    One `colnde_ensemble_loss_grad_dev` and one `colnde_ensemble_adam_step_dev` per iteration for all models, on the problem's simulations and
    loss scalings; `save_best` per model (torch.where over rows).  Returns one TrainResult per model.
    schedule: RK4 steps per save interval shared by the K models (`ColumnNDEEnsemble.set_schedule`), None: cfg.substeps; "choose": chosen before the
    first gradient from the initial weights and every member's constants (`ColumnNDEEnsemble.choose_ensemble_schedule` at `reltol`, None:
    cfg.reltol) — every TrainResult then carries the counts (`schedule`) and its member's own estimate at them (`schedule_estimate`).
    The member loss (`ColumnNDEEnsemble.set_member_loss`) — with all three of the following None the function issues the calls above:
    training_fractions: dict(T, dTdz, profile) for all members or a list of K dicts — `determine_loss_scalings` per member (NDE_training.jl:256-288):
    one `member_loss` at the initial weights under unit scalings, then `calculate_loss_scalings` (loss.jl:11-31) on every row, so that each member
    trains under the scalings of its own first solve with its own constants.  training_simulations: a list of K index lists, member k trains on
    its own simulations (N_sims of train_NDE_args.jl; train_free_convection_nde.jl:60-66) and is still solved on all of them.  gradient_scaling:
    without fractions, the scalings are (1, 1, 1, g, g, g) for every member (None: the problem's loss scalings)."""
    from .nde import ColumnNDEEnsemble, TileNDEEnsemble, check_ensemble_arrays, is_net_split_shape
    # any other architecture trains on the tile engine's ensemble (`TileNDEEnsemble`), which has neither a member loss nor a step schedule
    net_split = is_net_split_shape(problem.cfg)
    if not net_split:
        for name, arg in (("training_fractions", training_fractions), ("training_simulations", training_simulations), ("schedule", schedule)):
            if arg is not None:
                raise ValueError("%s covers the net-split shape (Nz = 32, three 96-50-20-31 nets): this configuration trains on the tile engine's "
                                 "ensemble (TileNDEEnsemble), which has no member loss and no step schedule" % name)
    import torch
    W = np.ascontiguousarray(weights, dtype=np.float32)
    ph = None if physics is None else np.ascontiguousarray(physics, dtype=np.float32)
    et = np.ascontiguousarray(etas, dtype=np.float32)
    K = W.shape[0] if W.ndim == 2 else 0
    check_ensemble_arrays(K, problem.cfg.n_params, W, ph, et)
    eng = problem.engine
    ens = (ColumnNDEEnsemble if net_split else TileNDEEnsemble)(problem.cfg, problem.n_simulations, K, physics=ph, device=eng.device,
                                                                 matrix_arithmetic=eng.matrix_arithmetic)
    chosen, chosen_est = None, None
    try:
        if schedule is not None and not isinstance(schedule, str):
            ens.set_schedule(schedule)
        elif schedule is not None and schedule != "choose":
            raise ValueError("schedule: counts per save interval, None or \"choose\", got %r" % (schedule,))
        dev = torch.device("cuda", eng.device)
        t = lambda a: a if a is None or _is_torch_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))
        x0, bcs, truth = (t(a).to(dev).contiguous() for a in (problem.uvT0, problem.BCs, problem.uvT_trains))
        ens.set_problem(x0, bcs, truth)
        if isinstance(schedule, str):
            chosen, chosen_est = ens.choose_ensemble_schedule(W, 0.0 if reltol is None else float(reltol))
        n = ens.n_params
        theta = torch.as_tensor(W).to(dev).contiguous()
        eta_d = torch.as_tensor(et).to(dev).contiguous()
        out = torch.empty((K, n + 8), dtype=torch.float32, device=dev)
        sc = problem.loss_scalings.copy()
        if not problem.cfg.train_gradient:
            sc[3:] = 0.0
        member = not (training_fractions is None and training_simulations is None and gradient_scaling is None)
        if member and not net_split:         # gradient_scaling alone: one (1, 1, 1, g, g, g) for every member is the shared loss
            g = float(gradient_scaling) if problem.cfg.train_gradient else 0.0
            sc = np.array([1, 1, 1, g, g, g], dtype=np.float64)
            member = False
        if member:
            tg = problem.cfg.train_gradient
            cw = None if training_simulations is None else member_column_weights(K, problem.n_simulations, training_simulations)
            if gradient_scaling is not None:
                g = float(gradient_scaling) if tg else 0.0
                sc = np.array([1, 1, 1, g, g, g], dtype=np.float64)
            scs = np.tile(np.asarray(sc, np.float64), (K, 1))
            if training_fractions is not None:
                fr = member_fractions(K, training_fractions)
                ens.set_member_loss(np.tile(np.array([1, 1, 1, 1, 1, 1] if tg else [1, 1, 1, 0, 0, 0], np.float32), (K, 1)), cw)
                terms = ens.member_loss(theta).cpu().numpy()
                scs = np.stack([calculate_loss_scalings(terms[k, :6], fr[k], tg) for k in range(K)])
            ens.set_member_loss(scs.astype(np.float32), cw)
        hist = []
        for _ in range(epochs):
            m = torch.zeros((K, n), dtype=torch.float32, device=dev)
            v = torch.zeros((K, n), dtype=torch.float32, device=dev)
            bt = [beta[0], beta[1]]                                  # a fresh ADAM state per solve (ADAM.reset)
            best = torch.full((K,), float("inf"), dtype=torch.float32, device=dev)
            best_theta = theta.clone()
            for _ in range(maxiters):
                if member:
                    ens.member_loss_grad(theta, out=out)
                else:
                    ens.loss_grad(theta, sc, out=out)
                total = out[:, n + 6]
                hist.append(out[:, n:n + 7].clone())
                ens.adam_step(theta, out, m, v, eta_d, beta, eps, beta_t=tuple(bt))
                bt[0] *= beta[0]
                bt[1] *= beta[1]
                better = total < best
                best = torch.where(better, total, best)
                best_theta = torch.where(better[:, None], theta, best_theta)      # min_θ = copy(θ) AFTER update, per model
            theta = best_theta.clone()
        H = torch.stack(hist).cpu().numpy() if hist else np.zeros((0, K, 7), np.float32)
        th = theta.cpu().numpy()
    finally:
        ens.close()
    return [TrainResult(th[k], [dict(total=float(r[k, 6]), **{q: float(r[k, i]) for i, q in enumerate(LOSS_KEYS)}) for r in H], chosen,
                        None if chosen_est is None else float(chosen_est[k])) for k in range(K)]


def _is_torch_tensor(x):
    return type(x).__module__.startswith("torch")


# ---- NDE_profile (wind_mixing/src/training_postprocessing.jl:250-632) --------------------------------------------------------------------------
PROFILE_LOSS_KEYS = ("u", "v", "T", "∂u∂z", "∂v∂z", "∂T∂z")      # the reference's output keys are `<name>_losses`
_MPP = "_modified_pacanowski_philander"


def _local_richardson(cfg: NDEConfig, sol):
    """`local_richardson` on `D_face * u, v, T` WITHOUT ε (training_postprocessing.jl:429-430), Float32: [.., 3 Nz] -> [.., Nz + 1]; the two boundary
    faces are 0 / 0 = NaN, as in the reference."""
    f = np.float32
    Nz = cfg.Nz
    x = np.asarray(sol, f)
    g = []
    for q in range(3):
        d = np.zeros(x.shape[:-1] + (Nz + 1,), f)
        d[..., 1:Nz] = (x[..., q * Nz + 1:(q + 1) * Nz] - x[..., q * Nz:(q + 1) * Nz - 1]) * f(Nz)
        g.append(d)
    B = f(f(f(cfg.H) * f(cfg.g)) * f(cfg.alpha)) * f(cfg.sigma[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (B * g[2]) / ((f(cfg.sigma[0]) * g[0]) ** 2 + (f(cfg.sigma[1]) * g[1]) ** 2)


def _profile_block(cfg: NDEConfig, a, loss_scalings, suffix: str, flux_suffix=None):
    """The keys one solve contributes (:400-423, :310-322, :515-517): a = dict(sol [n_sim, n_save, 3 Nz], uw, vw, wT, Ri [n_sim, n_save, Nz + 1],
    losses [n_sim, 6, n_save]); every profile array comes out as the reference's Nz x Nt (faces: Nz + 1 x Nt) per simulation."""
    f = np.float32
    Nz = cfg.Nz
    out = {}
    T = lambda x: np.ascontiguousarray(np.swapaxes(np.asarray(x, f), -1, -2))
    sol = np.asarray(a["sol"], f)
    for q, name in enumerate(("u", "v", "T")):
        out["test_%s%s" % (name, suffix)] = T(f(cfg.sigma[q]) * sol[..., q * Nz:(q + 1) * Nz] + f(cfg.mu[q]))
    for q, name in enumerate(("uw", "vw", "wT")):
        un = T(f(cfg.sigma[3 + q]) * np.asarray(a[name], f) + f(cfg.mu[3 + q]))          # inv(scalings.uw).(test_uw)
        out["test_%s%s" % (name, flux_suffix if flux_suffix is not None else suffix)] = un - un[..., :1, :1]     # test_uw .- test_uw[1, 1]
    out["test_Ri%s" % suffix] = T(a["Ri"])
    ls = np.asarray(a["losses"], f)
    sc = [f(s) for s in loss_scalings]
    scaled = [sc[q] * ls[..., q, :] for q in range(6)]                                     # apply_loss_scalings, per time step
    for q, name in enumerate(PROFILE_LOSS_KEYS):
        out["%s_losses%s" % (name, suffix)] = scaled[q]
    prof, grad = scaled[0] + scaled[1] + scaled[2], scaled[3] + scaled[4] + scaled[5]
    out["losses%s" % suffix] = prof
    out["loss%s" % suffix] = prof.mean(axis=-1)
    out["losses%s_gradient" % suffix] = grad
    out["loss%s_gradient" % suffix] = grad.mean(axis=-1)
    return out


def _assemble_NDE_profile(cfg: NDEConfig, arrays, truth, loss_scalings, arrays_mpp=None, NN_only=None, train_parameters=None, truth_fluxes=None):
    """Everything `NDE_profile` does after its solves and flux evaluations (training_postprocessing.jl:392-599), for ONE member, on host arrays,
    in Float32 as the reference: the unscaling, `test_uw .- test_uw[1, 1]` on the unscaled fluxes (:515-526), `apply_loss_scalings`, the sums and
    the means.  arrays = dict(sol, uw, vw, wT, Ri, losses) of the member (scaled units; `ColumnNDEEnsemble.profile`'s rows plus the solution);
    truth [n_sim, n_save, 3 Nz], scaled.  With the closure: arrays_mpp, the same of the closure-only solve (all-zero networks), NN_only = (uw, vw,
    wT) evaluated with ν₀ = ν₋ = 0 on the member's solution, and train_parameters.  Every array carries a leading simulation axis in front of the
    reference's layout (`NDE_profile` judges one simulation): test_u [n_sim, Nz, Nt], test_uw [n_sim, Nz + 1, Nt], u_losses [n_sim, Nt],
    loss [n_sim].  The KPP keys are left out (OceanTurb is out of scope)."""
    f = np.float32
    Nz = cfg.Nz
    truth = np.asarray(truth, f)
    T = lambda x: np.ascontiguousarray(np.swapaxes(np.asarray(x, f), -1, -2))
    dz = f(cfg.H) / f(Nz)
    out = {"depth_profile": (-f(cfg.H) + dz * (np.arange(Nz, dtype=f) + f(0.5))),
           "depth_flux": (-f(cfg.H) + dz * np.arange(Nz + 1, dtype=f)),
           "t": np.asarray(cfg.save_times, f) * f(cfg.tau)}
    for q, name in enumerate(("u", "v", "T")):
        out["truth_" + name] = T(f(cfg.sigma[q]) * truth[..., q * Nz:(q + 1) * Nz] + f(cfg.mu[q]))
    for q, name in enumerate(("uw", "vw", "wT")):
        out["truth_" + name] = None if truth_fluxes is None else np.asarray(truth_fluxes[q], f)
    out["truth_Ri"] = T(_local_richardson(cfg, truth))
    out.update(_profile_block(cfg, arrays, loss_scalings, ""))
    if cfg.modified_pacanowski_philander:
        if arrays_mpp is None or NN_only is None:
            raise ValueError("with the closure on, NDE_profile needs the closure-only arrays (arrays_mpp) and the NN-only fluxes (NN_only)")
        out["train_parameters"] = dict(train_parameters or {}, loss_scalings=tuple(float(s) for s in loss_scalings))
        out.update(_profile_block(cfg, arrays_mpp, loss_scalings, _MPP))
        nn = _profile_block(cfg, dict(arrays, uw=NN_only[0], vw=NN_only[1], wT=NN_only[2]), loss_scalings, "", flux_suffix="_NN_only")
        out.update({k: v for k, v in nn.items() if k.endswith("_NN_only")})
    return out


def ensemble_NDE_profile(problem: WindMixingNDE, weights, physics=None, loss_scalings=(1.0, 1.0, 1.0, 5e-3, 5e-3, 5e-3), solve: str = "ensemble",
                         truth_fluxes=None) -> List[dict]:
    """`NDE_profile` (wind_mixing/src/training_postprocessing.jl:250-632) for the K members of a sweep at once: one dict per member with the
    reference's keys (see `_assemble_NDE_profile` for the layout; the KPP keys are left out).  weights [K, n_params]; physics [K, 5] = (nu0,
    nu_minus, dRi, Ric, Pr) per member or None (the problem's constants); the problem's simulations are the test simulations and need truth.
    Every flux, Richardson number and per-time-step loss comes from `colnde_ensemble_profile`: one call for the members, and with the closure one
    with ν₀ = ν₋ = 0 (`*_NN_only`) and one with all-zero networks on the closure-only solve (`*_modified_pacanowski_philander`).
    solve = "ensemble": the members are solved by `ColumnNDEEnsemble.forward`, the TRAINING right-hand side (`NDE`), all in one launch.
    solve = "mutating": each member is solved on a single `inplace_variant` handle — `NDE!`, what the reference's `solve_NDE_mutating` (:302) runs —
    and the result uploaded.  The two differ as `NDE` and `NDE!` do: `NDE!` has no ε in the Richardson number of the closure, and it carries the two
    documented in-place quirks (ν_T switched on ∂u∂z under convective adjustment, the diurnal top flux without −scaling(0)); without diurnal forcing
    and convective adjustment ε is the only difference.  The fluxes are `predict_flux`'s (the training conventions) in both modes, as in the reference."""
    from .nde import ColumnNDEEnsemble, check_ensemble_arrays
    if solve not in ("ensemble", "mutating"):
        raise ValueError("solve must be 'ensemble' or 'mutating', got %r" % (solve,))
    if problem.uvT_trains is None:
        raise ValueError("NDE_profile compares with the truth trajectories: the problem has none")
    cfg = problem.cfg
    if solve == "mutating" and not cfg.modified_pacanowski_philander:
        raise ValueError("solve='mutating' runs NDE!, which hard-wires the Pacanowski-Philander closure (training_postprocessing.jl:105-153): "
                         "a configuration without the closure is solved with solve='ensemble'")
    W = np.ascontiguousarray(weights, dtype=np.float32)
    ph = None if physics is None else np.ascontiguousarray(physics, dtype=np.float32)
    K = W.shape[0] if W.ndim == 2 else 0
    check_ensemble_arrays(K, cfg.n_params, W, ph)
    mpp = bool(cfg.modified_pacanowski_philander)
    eng = problem.engine
    x0, bcs, truth = problem.uvT0, problem.BCs, np.ascontiguousarray(problem.uvT_trains, dtype=np.float32)
    rows = ph if ph is not None else np.tile(np.array([[cfg.nu0, cfg.nu_minus, cfg.dRi, cfg.Ric, cfg.Pr]], np.float32), (K, 1))
    Z = np.zeros_like(W)

    def solve_mutating(Wm):
        sols = []
        for k in range(K):
            c = cfg.with_(inplace_variant=True, nu0=float(rows[k, 0]), nu_minus=float(rows[k, 1]), dRi=float(rows[k, 2]), Ric=float(rows[k, 3]),
                          Pr=float(rows[k, 4]))
            with ColumnNDE(c, problem.n_simulations, device=eng.device, matrix_arithmetic=eng.matrix_arithmetic) as one:
                one.set_problem(x0, bcs, truth)
                sols.append(one.forward(Wm[k]))
        return np.stack(sols)

    with ColumnNDEEnsemble(cfg, problem.n_simulations, K, physics=ph if mpp else None, device=eng.device, matrix_arithmetic=eng.matrix_arithmetic) as ens:
        ens.set_problem(x0, bcs, truth)
        run = (lambda Wm: ens.forward(Wm)) if solve == "ensemble" else solve_mutating
        sol = run(W)
        main = ens.profile(W, sol)
        if mpp:
            nn_rows = rows.copy()
            nn_rows[:, :2] = 0.0                                          # constants_NN_only (:286)
            nn = ens.profile(W, sol, physics=nn_rows, Ri=False, losses=False)
            sol0 = run(Z)
            zero = ens.profile(Z, sol0)
    out = []
    for k in range(K):
        a = dict(sol=sol[k], uw=main.uw[k], vw=main.vw[k], wT=main.wT[k], Ri=main.Ri[k], losses=main.losses[k])
        if mpp:
            a0 = dict(sol=sol0[k], uw=zero.uw[k], vw=zero.vw[k], wT=zero.wT[k], Ri=zero.Ri[k], losses=zero.losses[k])
            tp = dict(zip(MPP_KEYS, (float(x) for x in rows[k])))
            out.append(_assemble_NDE_profile(cfg, a, truth, loss_scalings, a0, (nn.uw[k], nn.vw[k], nn.wT[k]), tp, truth_fluxes))
        else:
            out.append(_assemble_NDE_profile(cfg, a, truth, loss_scalings, truth_fluxes=truth_fluxes))
    return out


def NDE_profile(problem: WindMixingNDE, weights, loss_scalings=(1.0, 1.0, 1.0, 5e-3, 5e-3, 5e-3), truth_fluxes=None) -> dict:
    """`NDE_profile` of one network triple: `ensemble_NDE_profile` with K = 1 and the reference's own solve (`solve_NDE_mutating`, which needs the
    closure: `NDE!` hard-wires it)."""
    return ensemble_NDE_profile(problem, np.asarray(weights, np.float32)[None, :], None, loss_scalings, solve="mutating", truth_fluxes=truth_fluxes)[0]


def train_NN(engine: ColumnNDE, NN_type: str, weights, profiles, BCs, fluxes, optimizers: Sequence[ADAM], train_epochs: Sequence[int],
             gradient_scaling: float = 1e-4, order=None, cb: Optional[Callable] = None):
    """`train_NN(NN, 𝒟train, optimizers, train_epochs, FILE_PATH, NN_type; …)` — wind_mixing/src/NN_training.jl:207-249: for each
    optimiser and epoch one `Flux.train!(NN_loss, Flux.params(NN), training_data, opt)` (ONE ADAM update per shuffled sample) followed by
    `total_loss(training_data)`, which `cb(total_loss, weights)` receives where the reference calls `write_data_NN_training`.
    The whole pass runs on the GPU (`colnde_pretrain_flux_dev`); `profiles` [n, 3Nz] = columns of 𝒟.uvT_scaled, `BCs` [n, 6],
    `fluxes` [n, Nz+1] = columns of 𝒟.<NN_type>.scaled, `order` = the shuffled sample order (default: as given).
    `weights`: the full [uw; vw; wT] vector — only the net being trained changes.  Returns (weights, [total loss per epoch])."""
    import torch
    k = {"uw": 0, "vw": 1, "wT": 2}[NN_type]
    dev = torch.device("cuda", engine.device)
    t = lambda a, dt=np.float32: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    theta, X, B, Y = t(weights), t(profiles), t(BCs), t(fluxes)
    od = None if order is None else t(order, np.int32)
    hist = []
    for opt, n_ep in zip(optimizers, train_epochs):
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        if opt.m is not None:
            m.copy_(t(opt.m)); v.copy_(t(opt.v))
        for _ in range(n_ep):
            engine.pretrain_flux(k, theta, m, v, X, B, Y, od, gradient_scaling, opt, update=True)
            total = engine.pretrain_flux(k, theta, None, None, X, B, Y, od, gradient_scaling, opt, update=False)
            hist.append(total)
            if cb is not None:
                cb(total, theta)
        opt.m, opt.v = m.double().cpu().numpy(), v.double().cpu().numpy()
    return theta.cpu().numpy(), hist


def train_NN_ensemble(ens, weights, profiles, BCs, fluxes, optimizers: Sequence[ADAM], train_epochs: Sequence[int], etas=None,
                      gradient_scaling: float = 1e-4, seeds=None, nets=("uw", "vw", "wT"), cb: Optional[Callable] = None):
    """The loop of `train_NN` (wind_mixing/src/NN_training.jl:207-249) for the chosen flux nets of all K models of `ens` (a `ColumnNDEEnsemble` — the
    handle that then trains the NDE sweep) at once: per optimiser and epoch ONE `pretrain_fluxes` launch (one ADAM update per sample and chain, model
    k's nets fitted under model k's closure constants) and one update=False launch for `total_loss(training_data)`, which `cb(total_loss [K, 3],
    weights)` receives.  Each (model, net) walks its own fresh permutation per pass (`free_convection.pretrain_orders`, one seed per chain; seeds
    None: 0..3K-1, else [K, 3]); the loss over the data is summed in that pass's order, as `train_NN` does.
    weights [K, n_params]; profiles [n, 3Nz], BCs [n, 6], fluxes [3, n, Nz + 1] = 𝒟.uw / vw / wT.scaled.  optimizers: flux_compat.ADAMs, read for
    rate, beta and eps only — moments and running powers start afresh with each and carry across its epochs.  etas: None (every chain takes each
    optimiser's rate), [S, K] per-model or [S, K, 3] per-chain rates for the S optimisers.
    Returns (weights [K, n_params], history [passes, K, 3]): after each pass the loss over the training set at the weights it left (0: net not chosen)."""
    import torch
    from .free_convection import pretrain_orders
    from .nde import check_wm_pretrain_arrays, wm_pretrain_nets_mask
    K, S = ens.n_models, len(optimizers)
    mask = wm_pretrain_nets_mask(nets)
    Wn = np.ascontiguousarray(weights, dtype=np.float32)
    Xn, Bn, Yn = (np.ascontiguousarray(a, dtype=np.float32) for a in (profiles, BCs, fluxes))
    if len(train_epochs) != S or any(int(e) < 0 for e in train_epochs):
        raise ValueError("train_epochs: expected %d counts >= 0 (one per optimiser), got %r" % (S, list(train_epochs)))
    if etas is None:
        et = np.array([opt.eta for opt in optimizers], dtype=np.float32).reshape(S, 1, 1) * np.ones((1, K, 3), np.float32)
    else:
        et = np.asarray(etas, dtype=np.float32)
        if et.shape == (S, K):
            et = np.repeat(et[:, :, None], 3, axis=2)
        if et.shape != (S, K, 3):
            raise ValueError("etas: expected shape %s or %s (per-model or per-chain rates, one row per optimiser), got %s" % ((S, K), (S, K, 3), np.shape(etas)))
    et = np.ascontiguousarray(et, dtype=np.float32)
    seeds = np.arange(3 * K) if seeds is None else np.asarray(seeds)
    if seeds.shape != (K, 3) and not (seeds.ndim == 1 and seeds.size == 3 * K):
        raise ValueError("seeds: expected shape %s (one per model and net), got %s" % ((K, 3), seeds.shape))
    n_passes = int(sum(int(e) for e in train_epochs))
    n = check_wm_pretrain_arrays(ens.cfg, K, Wn, Xn, Bn, Yn, etas=et[0] if S else None)
    orders = pretrain_orders(seeds.reshape(-1), n, n_passes).reshape(n_passes, K, 3, n)
    dev = torch.device("cuda", ens.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev).contiguous()
    theta, Xd, Bd, Yd = up(Wn.copy()), up(Xn), up(Bn), up(Yn)
    history = np.zeros((n_passes, K, 3), np.float32)
    p = 0
    for i, (opt, n_ep) in enumerate(zip(optimizers, train_epochs)):
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        bt = [float(opt.beta[0]), float(opt.beta[1])]
        eta_d = up(et[i])
        for _ in range(int(n_ep)):
            od = up(orders[p])
            ens.pretrain_fluxes(theta, m, v, Xd, Bd, Yd, od, gradient_scaling, eta_d, mask, opt.beta, opt.eps, bt, update=True)
            history[p] = ens.pretrain_fluxes(theta, None, None, Xd, Bd, Yd, od, gradient_scaling, None, mask, opt.beta, opt.eps, bt, update=False)
            if cb is not None:
                cb(history[p], theta)
            p += 1
    return theta.cpu().numpy(), history


def _named(d, *names):
    for nm in names:
        if isinstance(d, dict) and nm in d:
            return float(d[nm])
        if not isinstance(d, dict) and hasattr(d, nm):
            return float(getattr(d, nm))
    raise KeyError(names[0])


WM_FIXED_SHAPE = (96, 50, 20, 31)        # the one architecture the four single-model embedding calls cover (Nz = 32, identity output layer)


def _wm_fixed_shape(engine: ColumnNDE) -> bool:
    """whether the four single-model calls serve the engine (one that states no configuration is taken at its word: it has those calls)"""
    c = getattr(engine, "cfg", None)
    return c is None or c.Nz == 32 and tuple(c.layer_sizes) == WM_FIXED_SHAPE and c.activations[-1] == "identity"


def _wm_embedded_single(engine: ColumnNDE, weights, u2, v2, T2, top, Lz, dt=None, params=None, ca=False, hb=None, ht=None, step=False, flux=False):
    """Any other architecture: `ColumnNDE.wm_embedded` with the single handle as K = 1 (`colnde_ensemble_wm_embedded`); the leading axis taken off."""
    one = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32))[None]
    r = engine.wm_embedded(np.asarray(weights, np.float32).reshape(1, -1), one(u2), one(v2), one(T2), top, Lz, dt,
                           None if params is None else np.asarray(params, np.float64).reshape(1, 7), ca, one(hb), one(ht), step=step, flux=flux)
    return tuple(None if g is None else tuple(a[0] for a in g) for g in r)


def NN_forcings(engine: ColumnNDE, weights, u, v, T, top_fluxes, Lz: float):
    """`NN_uw_forcing`, `NN_vw_forcing`, `NN_wT_forcing` (wind_mixing/src/NDE_oceananigans.jl:288-329) as the ocean model applies them
    (`- p.∂z_uw_NN[k]`, :333, :338, :343): the three forcings [n, Nz] (or [Nz]) of `interior(u)`, `interior(v)`, `interior(T)` in the
    model's units.  top_fluxes = (uw_flux, vw_flux, wT_flux) at the top face: scalars or [n] arrays ([3, n]); a diurnal wT_flux(t) is
    passed as its value at t."""
    u, v, T = (np.asarray(a, dtype=np.float32) for a in (u, v, T))
    shape = T.shape
    u2, v2, T2 = (a.reshape(-1, shape[-1]) for a in (u, v, T))
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_fluxes, np.float32).reshape(3, -1), (3, T2.shape[0])))
    if not _wm_fixed_shape(engine):
        return tuple(-d.reshape(shape) for d in _wm_embedded_single(engine, weights, u2, v2, T2, top, Lz)[0])
    return tuple(-d.reshape(shape) for d in engine.wm_infer_dz_flux(weights, u2, v2, T2, top, Lz))


def progress_neural_network(engine: ColumnNDE, weights, u, v, T, top_fluxes, Lz: float, dt: float, p: dict, constants,
                            convective_adjustment: bool = False, halo_bottom=None):
    """One iteration of `progress_neural_network` (wind_mixing/src/NDE_oceananigans.jl:380-405): the stored `∂z_uw_NN`, `∂z_vw_NN`,
    `∂z_wT_NN` of the state as given, then `modified_pacanowski_philander!` on it.  `p`, `constants`, halo_bottom as
    `modified_pacanowski_philander_step`; top_fluxes as `NN_forcings`.  Returns ((∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), (u′, v′, T′))."""
    params = (_named(p, "ν₀", "nu0"), _named(p, "ν₋", "nu_minus"), _named(p, "ΔRi", "dRi"), _named(p, "Riᶜ", "Ric"), _named(p, "Pr"),
              _named(constants, "α", "alpha"), _named(constants, "g"))
    u, v, T = (np.asarray(a, dtype=np.float32) for a in (u, v, T))
    shape = T.shape
    u2, v2, T2 = (a.reshape(-1, shape[-1]) for a in (u, v, T))
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_fluxes, np.float32).reshape(3, -1), (3, T2.shape[0])))
    hb = None if halo_bottom is None else np.asarray(halo_bottom, np.float32).reshape(3, -1)
    if not _wm_fixed_shape(engine):
        dz, st, _ = _wm_embedded_single(engine, weights, u2, v2, T2, top, Lz, dt, params, convective_adjustment, hb, step=True)
    else:
        dz, st = engine.wm_embedded_step(weights, u2, v2, T2, top, Lz, dt, params, convective_adjustment, hb)
    return tuple(d.reshape(shape) for d in dz), tuple(a.reshape(shape) for a in st)


def ensemble_progress_neural_network(ens, weights, state, top_fluxes, Lz: float, dt: float, p=None, constants=None, convective_adjustment: bool = False,
                                     halo_bottom=None, halo_top=None, flux: bool = False):
    """`progress_neural_network` for the K models of a `ColumnNDEEnsemble` in one launch: state = (u, v, T), each [K, n, Nz] (or [K, Nz] for one
    column per model), every model on its own state; top_fluxes [3] or [3, n], shared by the models.  `p`: a sequence of K parameter dicts (as
    `progress_neural_network`'s `p`) with `constants` one dict for all, or None: the ensemble's own physics.  halo_bottom / halo_top [K, 3, n]
    or None.  Returns ((∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), (u′, v′, T′)) shaped like the state — and, with flux=True, also (uw, vw, wT) of the state
    as given ([.., Nz + 1]).  Row k is `progress_neural_network` of model k, bit for bit."""
    K = ens.n_models
    u, v, T = (np.asarray(a, dtype=np.float32) for a in state)
    shape = T.shape
    u3, v3, T3 = (np.ascontiguousarray(a.reshape(K, -1, shape[-1])) for a in (u, v, T))
    n = T3.shape[1]
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_fluxes, np.float32).reshape(3, -1), (3, n)))
    halos = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(K, 3, -1)) for a in (halo_bottom, halo_top)]
    params = None
    if p is not None:
        if len(p) != K or constants is None:
            raise ValueError("p must hold one parameter dict per model (%d) and constants must be given with it" % K)
        params = np.array([_mpp_tuple(pk, constants) for pk in p], dtype=np.float32)
    r = ens.wm_embedded(weights, u3, v3, T3, top, Lz, dt, params, convective_adjustment, halos[0], halos[1], step=True, flux=flux)
    out = tuple(d.reshape(shape) for d in r.dz), tuple(a.reshape(shape) for a in r.state)
    if flux:
        out += (tuple(f.reshape(shape[:-1] + (shape[-1] + 1,)) for f in r.faces),)
    return out


def _mpp_tuple(p, constants):
    return (_named(p, "ν₀", "nu0"), _named(p, "ν₋", "nu_minus"), _named(p, "ΔRi", "dRi"), _named(p, "Riᶜ", "Ric"), _named(p, "Pr"),
            _named(constants, "α", "alpha"), _named(constants, "g"))


def _diag_args(u, v, T, top_fluxes, halos):
    u, v, T = (np.asarray(a, dtype=np.float32) for a in (u, v, T))
    shape = T.shape
    u2, v2, T2 = (np.ascontiguousarray(a.reshape(-1, shape[-1])) for a in (u, v, T))
    n = T2.shape[0]
    top = np.ascontiguousarray(np.broadcast_to(np.asarray(top_fluxes, np.float32).reshape(3, -1), (3, n)))
    if halos is not None:
        if len(halos) != 2:
            raise ValueError("halos must be (halo_bottom, halo_top); either may be None")
        halos = tuple(None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32).reshape(3, -1), (3, n))) for a in halos)
    return shape[:-1] + (shape[-1] + 1,), u2, v2, T2, top, halos


def diagnose_NN_flux(engine: ColumnNDE, weights, u, v, T, top_fluxes, Lz: float, p: dict, constants, convective_adjustment: bool = False, halos=None):
    """`diagnose_NN_flux_uw`, `diagnose_NN_flux_vw`, `diagnose_NN_flux_wT` (wind_mixing/src/NDE_oceananigans.jl:226-286): the total fluxes
    (uw, vw, wT) on the Nz + 1 faces ([n, Nz + 1], or [Nz + 1] for one column) that the embedding saves with a state.  `p`, `constants` as
    `modified_pacanowski_philander_step`; top_fluxes as `NN_forcings`; halos = None or (halo_bottom, halo_top): the u, v, T halo cells
    below and above the column, each [3, n] (or [3]) or None (zero-gradient fill)."""
    shape, u2, v2, T2, top, halos = _diag_args(u, v, T, top_fluxes, halos)
    if not _wm_fixed_shape(engine):
        hb, ht = halos if halos is not None else (None, None)
        faces = _wm_embedded_single(engine, weights, u2, v2, T2, top, Lz, None, _mpp_tuple(p, constants), convective_adjustment, hb, ht, flux=True)[2]
    else:
        faces = engine.wm_diagnose_flux(weights, u2, v2, T2, top, Lz, _mpp_tuple(p, constants), convective_adjustment, halos)
    return tuple(f.reshape(shape) for f in faces)


def diagnose_baseline_flux(engine: ColumnNDE, u, v, T, top_fluxes, Lz: float, p: dict, constants, convective_adjustment: bool = False, halos=None):
    """`diagnose_baseline_flux_uw`, `_vw`, `_wT` (wind_mixing/src/NDE_oceananigans.jl:157-191): the same for the diffusivity-only model,
    (uw, vw, wT) = (−ν ∂z u, −ν ∂z v, −νT ∂z T) with the top face replaced by the top flux.  Arguments as `diagnose_NN_flux` without the
    weights; of halos only halo_bottom is read (the one face that would see halo_top is replaced)."""
    shape, u2, v2, T2, top, halos = _diag_args(u, v, T, top_fluxes, halos)
    faces = engine.mpp_diagnose_flux(u2, v2, T2, top, float(Lz) / T2.shape[1], _mpp_tuple(p, constants), convective_adjustment,
                                     None if halos is None else halos[0])
    return tuple(f.reshape(shape) for f in faces)


def modified_pacanowski_philander_step(engine: ColumnNDE, u, v, T, dt: float, dz: float, p: dict, constants, convective_adjustment: bool = False,
                                       halo_bottom=None):
    """`modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment)` (wind_mixing/src/NDE_oceananigans.jl:61-101;
    diffusivities :17-58) on `interior(u)`, `interior(v)`, `interior(T)` as [n, Nz] (or [Nz]) arrays: returns (u′, v′, T′).
    `p` is the reference's diffusivity dictionary (keys "ν₀", "ν₋", "ΔRi", "Riᶜ", "Pr"; ASCII "nu0", "nu_minus", "dRi", "Ric" accepted),
    `constants` carries α and g (attributes or keys `alpha`/`α`, `g`).  halo_bottom [3, n]: the u, v, T halo cells below the deepest
    cell (None: zero-gradient fill)."""
    def get(d, *names):
        for nm in names:
            if isinstance(d, dict) and nm in d:
                return float(d[nm])
            if not isinstance(d, dict) and hasattr(d, nm):
                return float(getattr(d, nm))
        raise KeyError(names[0])
    params = (get(p, "ν₀", "nu0"), get(p, "ν₋", "nu_minus"), get(p, "ΔRi", "dRi"), get(p, "Riᶜ", "Ric"), get(p, "Pr"),
              get(constants, "α", "alpha"), get(constants, "g"))
    u, v, T = (np.asarray(a, dtype=np.float32) for a in (u, v, T))
    shape = T.shape
    u2, v2, T2 = (a.reshape(-1, shape[-1]) for a in (u, v, T))
    hb = None if halo_bottom is None else np.asarray(halo_bottom, np.float32).reshape(3, -1)
    uo, vo, To = engine.implicit_diffusion(u2, v2, T2, dt, dz, params, convective_adjustment, hb)
    return uo.reshape(shape), vo.reshape(shape), To.reshape(shape)


# ---- calibrating the closure itself (wind_mixing/src/diffusivity_parameter_optimisation.jl) ---------------------------------------------------
MPP_KEYS = ("nu0", "nu_minus", "dRi", "Ric", "Pr")


@dataclass
class MPPOptimisationResult:
    parameters: np.ndarray        # [K, 5] fitted constants per start (MPP_KEYS order)
    losses: np.ndarray            # [n_iterations, K]: total loss BEFORE each update
    terms: np.ndarray             # [n_iterations, K, 6]: the scaled terms (LOSS_KEYS order)
    best: int                     # the start whose final loss is least
    loss_scalings: np.ndarray
    final_losses: np.ndarray      # [K]: total loss at the returned parameters


def _problem_arrays(problem):
    """(cfg, x0, bcs, truth) of a synthetic.ColumnProblem-like object or of a WindMixingNDE."""
    get = lambda *names: next((getattr(problem, n) for n in names if getattr(problem, n, None) is not None), None)
    x0, bcs, truth = get("x0", "uvT0"), get("bcs", "BCs"), get("truth", "uvT_trains")
    if x0 is None or bcs is None or truth is None:
        raise ValueError("the problem needs initial profiles, boundary conditions and training trajectories (x0 / bcs / truth)")
    return problem.cfg, x0, bcs, truth


def optimise_modified_pacanowski_philander(problem, optimizers: Sequence[ADAM], maxiters: int, nu0: float = 1e-4, nu_minus: float = 1e-1,
                                           dRi: float = 0.1, Ric: float = 0.25, Pr: float = 1.0, train_gradient: bool = True,
                                           gradient_scaling: float = 5e-3, training_fractions: Optional[dict] = None, starts=None,
                                           cb: Optional[Callable] = None, s_min: float = 1e-3, device: int = 0) -> MPPOptimisationResult:
    """`optimise_modified_pacanowski_philander` (diffusivity_parameter_optimisation.jl:35-231) on the closure engine: fits (nu0, nu_minus, dRi, Ric, Pr)
    to the problem's trajectories by ADAM on the exact discrete gradient.

    As in the reference the optimiser works on the SCALED parameters s = p / p_initial, starting from ones (:44-48, :72-73); dL/ds = p_initial * dL/dp is
    one elementwise op on the result rows, and the update is Flux ADAM (`colnde_adam_step_dev`) on the 5 K vector, one optimiser after the other (:205-227),
    each with a fresh state.  Loss scalings: (1, 1, 1, g, g, g) with g = gradient_scaling, or from `training_fractions` through `calculate_loss_scalings`
    after one forward solve at the initial constants (:114-148; with several starts: the first start's solve).  train_gradient=False zeroes the three
    gradient terms (loss_mpp, :150-163).

    The reference hands the box lb = 0, ub = 10 in scaled units to the optimisation problem (:197).  Here the scaled parameters are clamped to [s_min, 10]
    after every update.  The lower edge s_min = 1e-3 is THIS PROJECT'S, not the reference's: dRi = 0 and Pr = 0 are singular (y = (Ri - Ric) / dRi, nu / Pr),
    so the box cannot be closed at 0.

    starts: [K, 5] initial constant sets fitted side by side (multi-start), every kernel launched once for all K; default: the single set of the keywords.
    The handle's sub-step count is cfg.substeps raised, if need be, to `colnde_closure_min_substeps` of every initial set with nu0 and nu_minus doubled and
    Pr no larger than 1 (room for the fit to move; the far corner of the box, 10 x the diffusivities at Pr -> 0, would be needlessly pessimistic).  A set that
    still leaves the stable regime shows up as a non-finite loss in its own row only.

    cb(parameters [K, 5], total [K], terms [K, 6], optimizer_index, iteration): what the reference's callback logs (:209-223).  Returns MPPOptimisationResult."""
    import torch
    from .nde import ClosureColumns, closure_min_substeps
    cfg, x0, bcs, truth = _problem_arrays(problem)
    p0 = np.array([[nu0, nu_minus, dRi, Ric, Pr]] if starts is None else starts, dtype=np.float64)
    if p0.ndim != 2 or p0.shape[1] != 5:
        raise ValueError("starts: expected shape [K, 5] = (nu0, nu_minus, dRi, Ric, Pr) per start, got %s" % (p0.shape,))
    if not (p0 > 0).all():
        raise ValueError("the initial constants must be positive (they scale the optimised parameters)")
    K = p0.shape[0]
    need = max(closure_min_substeps(cfg, (2 * r[0], 2 * r[1], r[2], r[3], min(r[4], 1.0))) for r in p0)
    if need > cfg.substeps:
        cfg = cfg.with_(substeps=need)
    eng = ClosureColumns(cfg, len(x0), K, device=device)
    try:
        dev = torch.device("cuda", device)
        t = lambda a: (a if _is_torch_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))).to(dev).contiguous()
        eng.set_problem(t(x0), t(bcs), t(truth))
        p_init = torch.as_tensor(p0.astype(np.float32)).to(dev).contiguous()
        if training_fractions is None:
            g = gradient_scaling if train_gradient else 0.0
            sc = np.array([1, 1, 1, g, g, g], dtype=np.float64)
        else:
            terms0 = eng.loss(p_init, [1, 1, 1, 1, 1, 1] if train_gradient else [1, 1, 1, 0, 0, 0])[0, :6].cpu().numpy()
            sc = calculate_loss_scalings(terms0, training_fractions, train_gradient)
        if not train_gradient:
            sc[3:] = 0.0
        s = torch.ones((K, 5), dtype=torch.float32, device=dev)
        out = torch.empty((K, 13), dtype=torch.float32, device=dev)
        hist = []
        for oi, opt in enumerate(optimizers):
            m, v = torch.zeros_like(s), torch.zeros_like(s)
            bt = [opt.beta[0], opt.beta[1]]
            for it in range(maxiters):
                p = (s * p_init).contiguous()
                eng.loss_grad(p, sc, out=out)
                hist.append(out[:, 5:12].clone())
                if cb is not None:
                    o = out.cpu().numpy()
                    cb(p.cpu().numpy(), o[:, 11], o[:, 5:11], oi, it)
                gs = (out[:, :5] * p_init).contiguous()                    # dL/ds = p_initial * dL/dp
                eng.adam_step(s.view(-1), gs.view(-1), m.view(-1), v.view(-1), opt.eta, opt.beta, opt.eps, beta_t=tuple(bt))
                bt[0] *= opt.beta[0]
                bt[1] *= opt.beta[1]
                s.clamp_(float(s_min), 10.0)
        p = (s * p_init).contiguous()
        final = eng.loss(p, sc)[:, 6].cpu().numpy()
        H = torch.stack(hist).cpu().numpy() if hist else np.zeros((0, K, 7), np.float32)
        params = p.cpu().numpy()
    finally:
        eng.close()
    best = int(np.nanargmin(final)) if np.isfinite(final).any() else 0
    return MPPOptimisationResult(params, H[:, :, 6], H[:, :, :6], best, sc, final)
