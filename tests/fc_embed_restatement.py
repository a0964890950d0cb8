"""NumPy restatement (float64 unless told otherwise) of what the free-convection embedding does per iteration and writes out per saved
state — free_convection/src/oceananigans_nn.jl: `progress_neural_network` (:153-165), `convective_adjustment!` (:13-40) and
`diagnose_wT_NN` (:100-118) — for a batch of columns.  A helper, not a test: shared by tests/test_fc_embed_host.py and
tests/test_gpu_fc_embed.py, and by them alone.

Conventions (include/colnde.h, colnde_fc_embedded_step): T [n, Nz], k = 0 deepest, in the units `colnde_infer_dz_wT` takes; top_flux [n];
dz = Lz/Nz; c = dt/dz²; halo cells as given or, None, the nearest interior value (zero-gradient fill)."""
import numpy as np

from oracle import nde_oracle as O


def faces(cfg, weights, T, top_flux, dtype=np.float64):
    """F = [0; σ_wT y + μ_wT; top_flux] (enforce_fluxes, :95), y = NN(T_scaling(T̃)) (:101-105, :120-124) with the oracle's own network and
    its T̃ = 19.65 + T/20 (double_gyre_nn.jl:156, what O.infer_forcing evaluates).  [n, Nz + 1]."""
    m = O.Model(cfg, dtype)
    nets = m.unpack(np.asarray(weights, dtype))
    T = np.asarray(T, dtype)
    Tt = dtype(19.65) + T / dtype(20.0)
    y, _ = O.mlp_forward(nets[0], m.acts, (Tt - dtype(m.mu_T)) / dtype(m.s_T))
    F = np.zeros((T.shape[0], cfg.Nz + 1), dtype)
    F[:, 1:cfg.Nz] = dtype(m.s_wT) * y + dtype(m.mu_wT)
    F[:, cfg.Nz] = np.asarray(top_flux, dtype)
    return F


def dz_wT(cfg, weights, T, top_flux, Lz, dtype=np.float64):
    """The stored ∂z_wT_NN (:159-160): +∂z wT — the negative of the oracle's `compute_neural_network_forcing!` restatement."""
    return -O.infer_forcing(cfg, np.asarray(T, dtype), np.asarray(top_flux, dtype), np.asarray(weights, dtype), dtype(Lz), dtype=dtype)


def _halos(T, halos):
    hb, ht = halos if halos is not None else (None, None)
    hb = T[:, 0] if hb is None else np.asarray(hb, T.dtype)
    ht = T[:, -1] if ht is None else np.asarray(ht, T.dtype)
    return hb, ht


def centred_switch(T, halos=None):
    """κ_k ≠ 0 pattern of convective_adjustment! (:17-23): the centred ∂T/∂z of cell k is negative.  bool [n, Nz]."""
    hb, ht = _halos(T, halos)
    ext = np.concatenate([hb[:, None], T, ht[:, None]], axis=1)
    return (ext[:, 2:] - ext[:, :-2]) < 0


def face_switch(T, halos=None):
    """κ_f ≠ 0 pattern of diagnose_wT_NN (:107-113): ∂T/∂z on face f is negative.  bool [n, Nz + 1]."""
    hb, ht = _halos(T, halos)
    ext = np.concatenate([hb[:, None], T, ht[:, None]], axis=1)
    return (ext[:, 1:] - ext[:, :-1]) < 0


def convective_adjustment(T, dt, dz, K, halos=None, dtype=np.float64):
    """convective_adjustment!(model, Δt, K) (:13-40): κ (:20-23), ld, ud, d (:25-32) assembled DENSE, T′ = 𝓛 \\ T (:34-36) by numpy.linalg.solve."""
    T = np.asarray(T, dtype)
    n, Nz = T.shape
    kappa = np.where(centred_switch(T, halos), dtype(K), dtype(0))                  # κ[i] = ∂T∂z[i] < 0 ? K : 0
    c = dtype(dt) / (dtype(dz) * dtype(dz))
    out = np.empty_like(T)
    for i in range(n):
        k = kappa[i]
        L = np.zeros((Nz, Nz), dtype)
        for r in range(Nz):
            if r >= 1:
                L[r, r - 1] = -c * k[r]                                              # ld
            if r < Nz - 1:
                L[r, r + 1] = -c * k[r + 1]                                          # ud
                L[r, r] = 1 + c * (k[r] + k[r + 1])                                  # d[i], i < Nz
            else:
                L[r, r] = 1 + c * k[r]                                               # d[Nz]
        out[i] = np.linalg.solve(L, T[i])
    return out


def diagnose_wT(F, T, Lz, K, halos=None, dtype=np.float64):
    """diagnose_wT_NN (:100-118) given the NN faces F: wT_NN .- κ .* ∂T∂z on the Nz + 1 faces.  NaN < 0 is false, as in Julia."""
    T = np.asarray(T, dtype)
    hb, ht = _halos(T, halos)
    ext = np.concatenate([hb[:, None], T, ht[:, None]], axis=1)
    g = (ext[:, 1:] - ext[:, :-1]) / (dtype(Lz) / dtype(T.shape[1]))                 # ∂z(T) at (Center, Center, Face)
    kappa = np.where(g < 0, dtype(K), dtype(0))
    return np.asarray(F, dtype) - kappa * g


def embedded_step(cfg, weights, T, top_flux, Lz, dt, K, halos=None, dtype=np.float64):
    """progress_neural_network (:153-165) + diagnose_wT_NN of the state as given: (∂z_wT_NN, T′, wT_faces).  The forcing is evaluated on T
    BEFORE the adjustment (:159-162)."""
    F = faces(cfg, weights, T, top_flux, dtype)
    dz = dtype(Lz) / dtype(cfg.Nz)
    return dz_wT(cfg, weights, T, top_flux, Lz, dtype), convective_adjustment(T, dt, dz, K, halos, dtype), diagnose_wT(F, T, Lz, K, halos, dtype)


def switch_robust_case(Nz, n, seed=20261018):
    """Inputs on which float32 and float64 take the same switches: the level increments alternate between a small class (0.2 … 0.3) and a
    large one (0.6 … 0.9, both x 32/Nz), so every face gradient is at least 0.2 and every centred one (the sum of a small and a large
    increment) at least 0.3 away from zero, whatever the signs.  Column c has sign pattern c % 4: all stable, all unstable, alternating,
    random.  Returns float32 (T [n, Nz], top_flux [n], halo_bottom [n], halo_top [n]); the halos continue the pattern."""
    r = np.random.default_rng(seed + 1000 * Nz)
    f = np.arange(Nz + 1)
    mag = np.where(f % 2 == 0, r.uniform(0.2, 0.3, (n, Nz + 1)), r.uniform(0.6, 0.9, (n, Nz + 1))) * (32.0 / Nz)
    sign = np.empty((n, Nz + 1))
    c = np.arange(n) % 4
    sign[c == 0] = 1.0
    sign[c == 1] = -1.0
    sign[c == 2] = np.where(f % 2 == 0, 1.0, -1.0)
    sign[c == 3] = r.choice([-1.0, 1.0], size=(int((c == 3).sum()), Nz + 1))
    d = sign * mag                                                                   # d[:, f] = T[f] − T[f−1] across face f (halos at the ends)
    T = np.cumsum(d[:, 1:Nz], axis=1)
    T = np.concatenate([np.zeros((n, 1)), T], axis=1)
    T += 15.0 - T.mean(axis=1, keepdims=True)
    hb, ht = T[:, 0] - d[:, 0], T[:, -1] + d[:, Nz]
    top = 1e-5 * r.standard_normal(n)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (T, top, hb, ht))
