"""float64 NumPy restatement of the embedding's forcing chains — `NN_uw_forcing`, `NN_vw_forcing`, `NN_wT_forcing`
(wind_mixing/src/NDE_oceananigans.jl:288-329) with `enforce_fluxes_*` (:220-224) and `∂z_*` (:193-218) — on the oracle's own
`Model.unpack` / `mlp_forward`, for a batch of columns.  Shared by tests/test_wm_embed_host.py and tests/test_gpu_wm_embed.py."""
import numpy as np

from oracle import nde_oracle as O

LZ = 256.0
MPP = dict(nu0=1e-4, nu_minus=1e-1, dRi=1.0, Ric=0.25, Pr=1.0, alpha=1.67e-4, g=9.81)        # as tests/test_column_ops.py


def mpp_params():
    return (MPP["nu0"], MPP["nu_minus"], MPP["dRi"], MPP["Ric"], MPP["Pr"], MPP["alpha"], MPP["g"])


def dz_fluxes(cfg, weights, u, v, T, top_flux, Lz, dtype=np.float64):
    """(∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), each [n, Nz], as `progress_neural_network` stores them (:393-400): u, v, T [n, Nz] in the ocean
    model's units (k = 0 deepest), top_flux [3, n] physical.  No smoothing filter, none of the training conditions."""
    m = O.Model(cfg, dtype)
    nets = m.unpack(np.asarray(weights, dtype))
    u, v, T = (np.asarray(a, dtype) for a in (u, v, T))
    top = np.asarray(top_flux, dtype)
    n, Nz = T.shape
    mu = [dtype(x) for x in cfg.mu]
    sg = [dtype(x) for x in cfg.sigma]
    x = np.concatenate([(u - mu[0]) / sg[0], (v - mu[1]) / sg[1], (T - mu[2]) / sg[2]], axis=1)      # :289, :298, :316
    dz = dtype(Lz) / dtype(Nz)
    out = []
    for k in range(3):
        y, _ = O.mlp_forward(nets[k], m.acts, x)                                                     # [n, Nz - 1]
        if k < 2:
            a = sg[3 + k] * y + mu[3 + k]                                                            # inv(scaling).(uw)        :291
            interior = a - (sg[3 + k] * a[:, :1] + mu[3 + k])                                        # uw .- inv(scaling).(uw[1]) :292 (sic)
        else:
            interior = (sg[5] * y + mu[5]) - (sg[5] * y[:, :1] + mu[5])                              # :318
        F = np.concatenate([np.zeros((n, 1), dtype), interior, top[k][:, None]], axis=1)             # cat(0, uw, uw_flux)      :220-224
        out.append((F[:, 1:] - F[:, :-1]) / dz)                                                      # ∂z on (Center, Center, Center) :193-218
    return tuple(out)


def embed_inputs(p):
    """Ocean-unit state and top fluxes of a synthetic.wind_mixing_problem: u = σ_u x0[:, :Nz] + μ_u (likewise v, T), tops from
    bcs[:, 1], bcs[:, 3], bcs[:, 5] unscaled."""
    Nz, mu, sg = p.cfg.Nz, p.cfg.mu, p.cfg.sigma
    x0 = p.x0.astype(np.float64)
    u, v, T = (np.ascontiguousarray((sg[f] * x0[:, f * Nz:(f + 1) * Nz] + mu[f]).astype(np.float32)) for f in range(3))
    top = np.stack([sg[3 + k] * p.bcs[:, 1 + 2 * k].astype(np.float64) + mu[3 + k] for k in range(3)]).astype(np.float32)
    return u, v, T, np.ascontiguousarray(top)
