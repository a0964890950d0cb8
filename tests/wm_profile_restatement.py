"""NumPy restatement of what `NDE_profile` (wind_mixing/src/training_postprocessing.jl:250-632) diagnoses on the saved states of a solve — TEST
INFRASTRUCTURE, float64 or float32:

    fluxes            `predict_flux` per frame through the oracle (`O.predict_flux(cfg_k, x, bcs, θ_k, t_n)`, :404-423), scaled units
    local_richardson  on `D_face * u, v, T` WITHOUT ε (:425-431): the two boundary faces are 0 / 0 = NaN
    losses            `O.loss_per_tstep` (:310-317)
    postprocess       :392-599: the unscaling, `test_uw .- test_uw[1, 1]`, `apply_loss_scalings`, the sums and the means

Arrays carry a leading simulation axis in front of the reference's layout (NDE_profile judges one simulation)."""
import numpy as np

from oracle import nde_oracle as O

PHYSICS_KEYS = ("nu0", "nu_minus", "dRi", "Ric", "Pr")
LOSS_NAMES = ("u", "v", "T", "∂u∂z", "∂v∂z", "∂T∂z")
MPP = "_modified_pacanowski_philander"


def member_cfg(cfg, row):
    return cfg if row is None else cfg.with_(**dict(zip(PHYSICS_KEYS, [float(x) for x in row])))


def fluxes(cfg, theta, sol, bcs, dtype=np.float64):
    """[n_col, n_save, 3 Nz] -> uw, vw, wT, each [n_col, n_save, Nz + 1]; the time of frame n is the float32 the library holds"""
    out = np.empty((sol.shape[0], sol.shape[1], 3, cfg.Nz + 1), dtype)
    for n in range(sol.shape[1]):
        t = float(np.float32(cfg.save_times[n]))
        out[:, n] = O.predict_flux(cfg, sol[:, n], bcs, theta, t, dtype=dtype)
    return out[:, :, 0], out[:, :, 1], out[:, :, 2]


def local_richardson(cfg, sol, dtype=np.float64):
    """`local_richardson(∂u∂z, ∂v∂z, ∂T∂z, H, g, α, σ_u, σ_v, σ_T)` (NDE_training.jl:46-52) on D_face's gradients, no ε: [.., 3 Nz] -> [.., Nz + 1]"""
    Nz = cfg.Nz
    x = np.asarray(sol, dtype)
    g = [O._face_grad(x[..., q * Nz:(q + 1) * Nz], Nz) for q in range(3)]
    su, sv, sT = (dtype(s) for s in cfg.sigma[:3])
    Bz = dtype(cfg.H) * dtype(cfg.g) * dtype(cfg.alpha) * sT * g[2]
    S2 = (su * g[0]) ** 2 + (sv * g[1]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return Bz / S2


def diagnose(cfg, theta, sol, bcs, truth=None, dtype=np.float64):
    """dict(sol, uw, vw, wT, Ri[, losses]) of one member: what ColumnNDEEnsemble.profile returns for it, plus the solution"""
    uw, vw, wT = fluxes(cfg, theta, sol, bcs, dtype)
    a = dict(sol=np.asarray(sol, dtype), uw=uw, vw=vw, wT=wT, Ri=local_richardson(cfg, sol, dtype))
    if truth is not None:
        a["losses"] = O.loss_per_tstep(cfg, sol, truth).astype(dtype)
    return a


def _block(cfg, a, sc, suffix, dtype, flux_suffix=None):
    Nz = cfg.Nz
    tr = lambda x: np.swapaxes(np.asarray(x, dtype), -1, -2)
    out = {}
    for q, nm in enumerate(("u", "v", "T")):
        out["test_%s%s" % (nm, suffix)] = tr(dtype(cfg.sigma[q]) * np.asarray(a["sol"], dtype)[..., q * Nz:(q + 1) * Nz] + dtype(cfg.mu[q]))
    for q, nm in enumerate(("uw", "vw", "wT")):
        un = tr(dtype(cfg.sigma[3 + q]) * np.asarray(a[nm], dtype) + dtype(cfg.mu[3 + q]))
        first = un[..., 0, 0]                                        # test_uw[1, 1]: the bottom face of the first frame
        out["test_%s%s" % (nm, suffix if flux_suffix is None else flux_suffix)] = un - first[..., None, None]
    out["test_Ri" + suffix] = tr(a["Ri"])
    scaled = [dtype(sc[q]) * np.asarray(a["losses"], dtype)[..., q, :] for q in range(6)]
    for q, nm in enumerate(LOSS_NAMES):
        out["%s_losses%s" % (nm, suffix)] = scaled[q]
    out["losses" + suffix] = scaled[0] + scaled[1] + scaled[2]
    out["loss" + suffix] = out["losses" + suffix].mean(axis=-1)
    out["losses%s_gradient" % suffix] = scaled[3] + scaled[4] + scaled[5]
    out["loss%s_gradient" % suffix] = out["losses%s_gradient" % suffix].mean(axis=-1)
    return out


def postprocess(cfg, a, truth, loss_scalings, a_mpp=None, nn_only=None, train_parameters=None, dtype=np.float64):
    """:392-599 for one member (KPP keys left out)"""
    Nz = cfg.Nz
    tr = lambda x: np.swapaxes(np.asarray(x, dtype), -1, -2)
    dz = dtype(cfg.H) / dtype(Nz)
    out = dict(depth_profile=-dtype(cfg.H) + dz * (np.arange(Nz).astype(dtype) + dtype(0.5)), depth_flux=-dtype(cfg.H) + dz * np.arange(Nz + 1).astype(dtype),
               t=np.asarray(cfg.save_times, dtype) * dtype(cfg.tau))
    for q, nm in enumerate(("u", "v", "T")):
        out["truth_" + nm] = tr(dtype(cfg.sigma[q]) * np.asarray(truth, dtype)[..., q * Nz:(q + 1) * Nz] + dtype(cfg.mu[q]))
    for nm in ("uw", "vw", "wT"):
        out["truth_" + nm] = None
    out["truth_Ri"] = tr(local_richardson(cfg, truth, dtype))
    out.update(_block(cfg, a, loss_scalings, "", dtype))
    if cfg.modified_pacanowski_philander:
        out["train_parameters"] = dict(train_parameters or {}, loss_scalings=tuple(float(s) for s in loss_scalings))
        out.update(_block(cfg, a_mpp, loss_scalings, MPP, dtype))
        b = _block(cfg, dict(a, uw=nn_only[0], vw=nn_only[1], wT=nn_only[2]), loss_scalings, "", dtype, flux_suffix="_NN_only")
        out.update({k: v for k, v in b.items() if k.endswith("_NN_only")})
    return out


def nde_profile(cfg, theta, row, sol, sol0, bcs, truth, loss_scalings, dtype=np.float64):
    """The whole of NDE_profile after its solves, for one member with closure constants `row` (None: cfg's): sol the member's solution, sol0 the
    closure-only one (all-zero networks; unused without the closure)."""
    c = member_cfg(cfg, row)
    a = diagnose(c, theta, sol, bcs, truth, dtype)
    if not cfg.modified_pacanowski_philander:
        return postprocess(c, a, truth, loss_scalings, dtype=dtype)
    a0 = diagnose(c, np.zeros_like(theta), sol0, bcs, truth, dtype)
    nn = fluxes(c.with_(nu0=0.0, nu_minus=0.0), theta, sol, bcs, dtype)
    r = [getattr(c, k) for k in PHYSICS_KEYS]
    return postprocess(c, a, truth, loss_scalings, a0, nn, dict(zip(PHYSICS_KEYS, (float(np.float32(x)) for x in r))), dtype)


def compare(got, ref, rtol, atol):
    """every key of ref is in got and agrees: arrays within atol max|ref| + rtol |ref| (atol relative to the key's scale: the keys span 1e-11 .. 1e5)
    with the same non-finite pattern; returns the worst excess ratio"""
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref)))
    worst = 0.0
    for k, r in ref.items():
        g = got[k]
        if r is None or isinstance(r, dict):
            assert g == r or (isinstance(r, dict) and set(g) == set(r)), k
            if isinstance(r, dict):
                for q in r:
                    assert np.allclose(np.asarray(g[q], np.float64), np.asarray(r[q], np.float64), rtol=1e-6), (k, q)
            continue
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin), k
        if fin.any():
            ex = np.abs(g - r)[fin] / (atol * np.abs(r[fin]).max() + rtol * np.abs(r[fin]) + 1e-300)
            worst = max(worst, float(ex.max()))
            assert ex.max() <= 1.0, (k, float(ex.max()))
    return worst
