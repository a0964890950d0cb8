"""NumPy restatement (float64 unless told otherwise) of what the wind-mixing embedding saves with every state — the six diagnosis functions of
wind_mixing/src/NDE_oceananigans.jl: `diagnose_baseline_flux_uw / _vw / _wT` (:157-191) and `diagnose_NN_flux_uw / _vw / _wT` (:226-286), with
`modified_pacanowski_philander_diffusivity` (:17-58) and `enforce_fluxes_*` (:220-224) — written the way the Julia is written, for a batch of
columns, on the oracle's own `Model.unpack` / `mlp_forward`.  A helper, not a test: shared by tests/test_wm_diag_host.py and
tests/test_gpu_wm_diag.py.

Conventions (include/colnde.h, colnde_wm_diagnose_flux): u, v, T [n, Nz], k = 0 deepest, ocean units; top_flux [3, n]; dz = Lz/Nz; faces
[n, Nz + 1], face 0 the bottom; halos = None or (halo_bottom, halo_top), each [3, n] or None = the nearest interior value (zero-gradient fill).
mpp = dict(nu0, nu_minus, dRi, Ric, Pr, alpha, g) as tests/wm_embed_common.MPP."""
import numpy as np

from oracle import nde_oracle as O


def _fill_halo_regions(a, halo_b, halo_t):
    """[halo below; interior; halo above] of one field: [n, Nz + 2]."""
    hb = a[:, 0] if halo_b is None else np.asarray(halo_b, a.dtype)
    ht = a[:, -1] if halo_t is None else np.asarray(halo_t, a.dtype)
    return np.concatenate([hb[:, None], a, ht[:, None]], axis=1)


def _fields(u, v, T, halos, dtype):
    hb, ht = halos if halos is not None else (None, None)
    out = []
    for f, a in enumerate((u, v, T)):
        a = np.asarray(a, dtype)
        out.append(_fill_halo_regions(a, None if hb is None else np.asarray(hb, dtype)[f], None if ht is None else np.asarray(ht, dtype)[f]))
    return out


def dz_face(ext, dz):
    """ComputedField(@at (Center, Center, Face) ∂z(φ)) (:159, :232): (φ[f] − φ[f−1])/Δz on the Nz + 1 faces."""
    return (ext[:, 1:] - ext[:, :-1]) / dz


def richardson_number(u, v, T, dz, mpp, halos=None, dtype=np.float64):
    """richardson_number_ccf! on (Center, Center, Face) (:34-36): ∂z b / ((∂z u)² + (∂z v)²), b = gαT.  [n, Nz + 1]; 0/0 = NaN."""
    ue, ve, Te = _fields(u, v, T, halos, dtype)
    dz = dtype(dz)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dtype(mpp["g"]) * dtype(mpp["alpha"]) * dz_face(Te, dz) / (dz_face(ue, dz) ** 2 + dz_face(ve, dz) ** 2)


def tanh_step(x):
    return (1 - np.tanh(x)) / 2


def modified_pacanowski_philander_diffusivity(u, v, T, dz, mpp, convective_adjustment, halos=None, dtype=np.float64):
    """:17-58: (ν, ν_T), each [n, Nz + 1]."""
    Ri = richardson_number(u, v, T, dz, mpp, halos, dtype)
    n, Nf = Ri.shape
    Nz = Nf - 1
    nu = np.zeros((n, Nz + 1), dtype)                                                                 # ν = zeros(Float32, Nz+1)        :38
    with np.errstate(invalid="ignore"):
        for i in range(1, Nz):                                                                        # for i in 2:Nz                   :45
            nu[:, i] = dtype(mpp["nu0"]) + dtype(mpp["nu_minus"]) * tanh_step((Ri[:, i] - dtype(mpp["Ric"])) / dtype(mpp["dRi"]))
        if convective_adjustment:
            nu_T = np.where(Ri > 0, nu / dtype(mpp["Pr"]), dtype(1))                                  # Ri > 0 ? ν/Pr : 1f0            :51
        else:
            nu_T = nu / dtype(mpp["Pr"])                                                              # ν_T .= ν ./ Pr                  :54
    return nu, nu_T


def diagnose_baseline_flux(u, v, T, top_flux, dz, mpp, convective_adjustment=False, halos=None, dtype=np.float64):
    """diagnose_baseline_flux_uw / _vw / _wT (:157-191): (uw, vw, wT), each [n, Nz + 1]."""
    nu, nu_T = modified_pacanowski_philander_diffusivity(u, v, T, dz, mpp, convective_adjustment, halos, dtype)
    ue, ve, Te = _fields(u, v, T, halos, dtype)
    top = np.asarray(top_flux, dtype)
    out = []
    with np.errstate(invalid="ignore"):
        for k, (ext, d) in enumerate(((ue, nu), (ve, nu), (Te, nu_T))):
            flux = -d * dz_face(ext, dtype(dz))                                                       # uw = -ν .* ∂u∂z                 :162
            flux[:, -1] = top[k]                                                                      # uw[end] = uw_flux               :163
            out.append(flux)
    return tuple(out)


def nn_faces(cfg, weights, u, v, T, top_flux, dtype=np.float64):
    """enforce_fluxes(inv(scaling).(NN(uvT)) .- inv(scaling)(0)) (:235, :253, :274-276; :220-224) of the three nets: each [n, Nz + 1]; also the raw
    network outputs y (three [n, Nz − 1])."""
    m = O.Model(cfg, dtype)
    nets = m.unpack(np.asarray(weights, dtype))
    u, v, T = (np.asarray(a, dtype) for a in (u, v, T))
    top = np.asarray(top_flux, dtype)
    n = T.shape[0]
    mu = [dtype(x) for x in cfg.mu]
    sg = [dtype(x) for x in cfg.sigma]
    uvT = np.concatenate([(u - mu[0]) / sg[0], (v - mu[1]) / sg[1], (T - mu[2]) / sg[2]], axis=1)     # [u; v; T]                       :227-230
    F, ys = [], []
    for k in range(3):
        y, _ = O.mlp_forward(nets[k], m.acts, uvT)
        inv0 = sg[3 + k] * dtype(0) + mu[3 + k]                                                       # inv(uw_scaling)(0)
        interior = (sg[3 + k] * y + mu[3 + k]) - inv0                                                 # inv(uw_scaling).(uw_NN(uvT)) .- inv(uw_scaling)(0)
        F.append(np.concatenate([np.zeros((n, 1), dtype), interior, top[k][:, None]], axis=1))        # cat(0, uw, uw_flux, dims=1)     :220
        ys.append(y)
    return tuple(F), tuple(ys)


def diagnose_NN_flux(cfg, weights, u, v, T, top_flux, Lz, mpp, convective_adjustment=False, halos=None, dtype=np.float64):
    """diagnose_NN_flux_uw / _vw / _wT (:226-286): (uw, vw, wT), each [n, Nz + 1]."""
    dz = dtype(Lz) / dtype(cfg.Nz)
    F, _ = nn_faces(cfg, weights, u, v, T, top_flux, dtype)
    nu, nu_T = modified_pacanowski_philander_diffusivity(u, v, T, dz, mpp, convective_adjustment, halos, dtype)
    ue, ve, Te = _fields(u, v, T, halos, dtype)
    out = []
    with np.errstate(invalid="ignore"):
        for Fk, ext, d in ((F[0], ue, nu), (F[1], ve, nu), (F[2], Te, nu_T)):
            nu_dz = d * dz_face(ext, dz)                                                              # ν∂u∂z = ν .* interior(∂u∂z)[:]  :239
            out.append(Fk - nu_dz)                                                                    # uw = uw .- ν∂u∂z                :240
    return tuple(out)


def diag_inputs(p_inputs, n_all):
    """The GPU tests' state: embed_inputs' u, v, T, top with T perturbed by a FIXED profile so that float32 and float64 take the same `Ri > 0`
    branch on every face and both branches occur — T += 0.02 s_c k with s_c = +1, −1 alternating over blocks of three columns (a stable and an
    unstable stratification of 0.02 K per level on top of the synthetic one, far from Ri = 0) —, and the halo cells of test_fused_step's pattern
    continued to the top: both signs of the bottom and of the top T difference across columns.  float32 (u, v, T, top, halo_bottom, halo_top)."""
    u, v, T, top = p_inputs
    n, Nz = T.shape
    assert n == n_all
    s = np.where((np.arange(n) // 3) % 2 == 0, 1.0, -1.0)
    T = np.ascontiguousarray((T.astype(np.float64) + 0.02 * s[:, None] * np.arange(Nz)[None, :]).astype(np.float32))
    c = np.arange(n)
    hb = np.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] + np.where(c % 2, 0.01, -0.01)]).astype(np.float32)
    ht = np.stack([u[:, -1] + 2e-3, v[:, -1] - 1e-3, T[:, -1] + np.where((c // 2) % 2, 0.01, -0.01)]).astype(np.float32)
    return u, v, T, top, np.ascontiguousarray(hb), np.ascontiguousarray(ht)
