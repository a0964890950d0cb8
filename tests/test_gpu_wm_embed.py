"""Wind-mixing embedded inference on the GPU: `colnde_wm_infer_dz_flux` (NN_uw_forcing / NN_vw_forcing / NN_wT_forcing,
wind_mixing/src/NDE_oceananigans.jl:288-329) and `colnde_wm_embedded_step` (progress_neural_network, :380-405) against the float64
restatement of tests/wm_embed_common.py and the oracle's modified_pacanowski_philander_step.

Inputs: synthetic.wind_mixing_problem(200, n_frames=3, weight_divisor=1.0), its first n columns per case; weights_truth; Lz = 256.
Forcing bound: max|gpu − f64| / max|f64| <= 5e-6 per net — about 12x the distance of a float32 NumPy restatement from float64 on these
inputs (2.7e-7 / 4.0e-7 / 4.1e-7 for uw / vw / wT at 77 columns), the project's 10x convention; the kernel sums in another order than
NumPy and gets that margin, no more."""
import ctypes
import functools

import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as O
from tests import wm_embed_common as W
from tests.test_gpu_parity import _record      # COLNDE_RECORD_ERRORS=1: the measured errors join the other parity records

pytestmark = pytest.mark.gpu

N_ALL = 200
DZ_BOUND = 5e-6
NETS = ("uw", "vw", "wT")
DT = 60.0


@functools.lru_cache(maxsize=None)
def _problem():
    p = synthetic.wind_mixing_problem(N_ALL, n_frames=3, weight_divisor=1.0)
    u, v, T, top = W.embed_inputs(p)
    ref = W.dz_fluxes(p.cfg, p.weights_truth, u, v, T, top, W.LZ)
    for a in (u, v, T, top) + ref:
        a.setflags(write=False)
    return p, (u, v, T, top), ref


def _case(n):
    p, (u, v, T, top), ref = _problem()
    c = lambda a: np.ascontiguousarray(a[:n])
    return p, (c(u), c(v), c(T), np.ascontiguousarray(top[:, :n])), tuple(r[:n] for r in ref)


def _dz_errors(got, ref):
    return [float(np.abs(g.astype(np.float64) - r).max() / np.abs(r).max()) for g, r in zip(got, ref)]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 77, 200])
def test_forcing_parity_host_and_device_twins(n):
    """One pipe is built (colnde_describe: wm_infer=f32), so both matrix arithmetics of the handle must give the same bits."""
    import torch
    import colnde
    p, (u, v, T, top), ref = _case(n)
    outs = []
    for ma in ("bf16x3_exact", "f32_mfma"):
        with colnde.ColumnNDE(p.cfg, 4, matrix_arithmetic=ma) as nde:      # the handle's own column count is unrelated to n
            assert "wm_infer=f32" in nde.describe()
            host = nde.wm_infer_dz_flux(p.weights_truth, u, v, T, top, W.LZ)
            wd, ud, vd, Td, td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p.weights_truth, u, v, T, top))
            dev = nde.wm_infer_dz_flux(wd, ud, vd, Td, td, W.LZ)
            torch.cuda.synchronize()
            dev = tuple(d.cpu().numpy() for d in dev)
        errs = _dz_errors(host, ref)
        print("wm_infer n=%d %s: rel err uw %.3e vw %.3e wT %.3e" % ((n, ma) + tuple(errs)))
        _record("wm_infer/%d/%s" % (n, ma), **dict(zip(NETS, errs)))
        for h_, d_ in zip(host, dev):
            assert np.isfinite(h_).all() and np.array_equal(h_, d_)                                  # twins: bit for bit
        for nm, e in zip(NETS, errs):
            assert e <= DZ_BOUND, (nm, e)
        outs.append(host)
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_exact_properties():
    import colnde
    n = 77
    p, (u, v, T, top), ref = _case(n)
    dz = np.float32(W.LZ / 32)
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        a = nde.wm_infer_dz_flux(p.weights_truth, u, v, T, top, W.LZ)
        b = nde.wm_infer_dz_flux(p.weights_truth, u, v, T, top, W.LZ)
        c = nde.wm_infer_dz_flux(p.weights_truth, u, v, T, 2 * top, W.LZ)
        f = colnde.wind_mixing.NN_forcings(nde, p.weights_truth, u[3], v[3], T[3], top[:, 3], W.LZ)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                                           # two launches, equal bits
    assert np.array_equal(a[2][:, 0], np.zeros(n, np.float32))                                       # first interior wT face is exactly 0
    for k in range(3):
        assert np.array_equal(a[k][:, :-1], c[k][:, :-1])                                            # the top flux enters the top cell only ...
        # ... as top/Δz: c − a is the difference of two float32 roundings of (top-ish)/Δz, each within half an ulp of its own value
        want = top[k].astype(np.float64) / float(dz)
        tol = 2.0 ** -23 * (np.abs(a[k][:, -1]) + np.abs(c[k][:, -1])) + 1e-30
        assert (np.abs((c[k][:, -1].astype(np.float64) - a[k][:, -1]) - want) <= tol).all()
        # telescoping: Σ_k Δz ∂z F = F[Nz] − F[0] = top.  rtol 2e-4 of the top flux; where that is (nearly) zero — vw here — the rounding of the
        # 32 float32 terms still scales with the TERMS, so the same 2e-4 is also granted on the largest |Δz ∂z F| of the column
        terms = a[k].astype(np.float64) * float(dz)
        assert (np.abs(terms.sum(1) - top[k]) <= 2e-4 * np.maximum(np.abs(top[k]), np.abs(terms).max(1))).all()
        assert f[k].shape == (32,) and np.array_equal(f[k], -a[k][3])                                # the reference-named mirror: the negatives


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
@pytest.mark.parametrize("n", [1, 33, 77])
def test_fused_step(n, ca, halo):
    import torch
    import colnde
    p, (u, v, T, top), ref = _case(n)
    hb = np.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] + np.where(np.arange(n) % 2, 0.01, -0.01)]).astype(np.float32) if halo else None
    dzc = W.LZ / 32
    want = O.modified_pacanowski_philander_step(u, v, T, DT, dzc, convective_adjustment=bool(ca), halo_bottom=hb, **W.MPP)
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        wd, td = torch.from_numpy(p.weights_truth).cuda(), torch.from_numpy(top).cuda()
        hd = torch.from_numpy(hb).cuda() if halo else None
        ud, vd, Td = (torch.from_numpy(a).cuda() for a in (u, v, T))
        dz_a, st_a = nde.wm_embedded_step(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, hd, out=(ud, vd, Td))       # in place
        torch.cuda.synchronize()
        dz_a, st_a = tuple(d.cpu().numpy() for d in dz_a), tuple(d.cpu().numpy() for d in st_a)
        # not in place: the inputs survive and the ∂z arrays are the same bits — those of the PRE-diffusion state (`post` below: the
        # networks on the diffused state, what the wrong order would store, must differ)
        ud, vd, Td = (torch.from_numpy(a).cuda() for a in (u, v, T))
        dz_b, st_b = nde.wm_embedded_step(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, hd)
        torch.cuda.synchronize()
        assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((ud, vd, Td), (u, v, T)))     # inputs untouched
        dz_b, st_b = tuple(d.cpu().numpy() for d in dz_b), tuple(d.cpu().numpy() for d in st_b)
        host_dz, host_st = nde.wm_embedded_step(p.weights_truth, u, v, T, top, W.LZ, DT, W.mpp_params(), ca, hb)
        post = nde.wm_infer_dz_flux(p.weights_truth, st_b[0], st_b[1], st_b[2], top, W.LZ)           # what the WRONG order would store
        alone = nde.wm_infer_dz_flux(p.weights_truth, u, v, T, top, W.LZ)
    for x, y, z in zip(dz_a + st_a, dz_b + st_b, host_dz + host_st):
        assert np.isfinite(x).all() and np.array_equal(x, y) and np.array_equal(x, z)
    errs = _dz_errors(dz_a, ref)
    print("wm_embedded_step n=%d ca=%d halo=%d: dz rel err uw %.3e vw %.3e wT %.3e" % ((n, ca, halo) + tuple(errs)))
    _record("wm_embedded_step/%d/%d/%d" % (n, ca, halo), **dict(zip(NETS, errs)))
    for nm, e in zip(NETS, errs):
        assert e <= DZ_BOUND, (nm, e)
    assert all(np.array_equal(x, y) for x, y in zip(dz_a, alone))                                    # the forcing-only kernel's bits
    assert any(not np.array_equal(x, y) for x, y in zip(dz_a, post))                                 # ... and not those of the diffused state
    # u′, v′, T′: the tolerances tests/test_column_ops.py holds colnde_implicit_diffusion to
    for g, w_, tol in zip(st_a, want, (2e-5, 2e-5, 2e-6)):
        assert np.abs(g - w_).max() <= tol * np.abs(w_).max(), (np.abs(g - w_).max(), np.abs(w_).max())
    assert np.array_equal(st_a[2][:, 0], T[:, 0])                                                    # T′[1] = T_bottom, bit for bit


def test_progress_neural_network_mirror():
    import colnde
    p, (u, v, T, top), ref = _case(33)
    pj = {"ν₀": W.MPP["nu0"], "ν₋": W.MPP["nu_minus"], "ΔRi": W.MPP["dRi"], "Riᶜ": W.MPP["Ric"], "Pr": W.MPP["Pr"]}
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        dz, st = colnde.wind_mixing.progress_neural_network(nde, p.weights_truth, u, v, T, top, W.LZ, DT, pj, {"α": W.MPP["alpha"], "g": W.MPP["g"]}, True)
        dz2, st2 = nde.wm_embedded_step(p.weights_truth, u, v, T, top, W.LZ, DT, W.mpp_params(), True)
    assert all(np.array_equal(a, b) for a, b in zip(dz + st, dz2 + st2))


def _raw(nde, p, n=4, Lz=W.LZ):
    """colnde_wm_infer_dz_flux straight through ctypes (the refusals of the C ABI, not of the Python wrapper)."""
    z = lambda *s: np.zeros(s, np.float32)
    w, u, top, o = np.zeros(max(p.weights.size, 1), np.float32), z(max(n, 1), 32), z(3, max(n, 1)), [z(max(n, 1), 32) for _ in range(3)]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return nde._L.colnde_wm_infer_dz_flux(nde._h, P(w), P(u), P(u), P(u), P(top), ctypes.c_float(Lz), P(o[0]), P(o[1]), P(o[2]), n)


def test_refusals_name_the_reason():
    import colnde
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1.0)

    def refused(nde, match, **kw):
        assert _raw(nde, p, **kw) != 0
        msg = nde._L.colnde_last_error().decode()
        assert match in msg, msg

    fc = synthetic.free_convection_problem(8, Nz=32, n_save=3)
    with colnde.ColumnNDE(fc.cfg, 8) as nde:
        refused(nde, "needs a wind-mixing handle")
    with colnde.ColumnNDEEnsemble(p.cfg, 8, 2) as e:
        refused(e, "holds an ensemble of 2 models")
    with colnde.ClosureColumns(p.cfg, 8, 2) as c:
        refused(c, "closure handle")
    with colnde.ColumnNDE(p.cfg.with_(smooth_NN=True), 8) as nde:
        refused(nde, "no smoothing filter")
    wide = synthetic.wind_mixing_problem(8, n_frames=3, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
    with colnde.ColumnNDE(wide.cfg, 8) as nde:
        refused(nde, "three 96-50-20-31 networks")
        assert "96-400-400-31" in nde._L.colnde_last_error().decode() and "wm_infer" not in nde.describe()
    with colnde.ColumnNDE(p.cfg, 8) as nde:
        refused(nde, "n_columns >= 1 and Lz > 0", n=0)
        refused(nde, "n_columns >= 1 and Lz > 0", Lz=0.0)
        refused(nde, "n_columns >= 1 and Lz > 0", Lz=-1.0)
        u, v, T, top = W.embed_inputs(p)
        with pytest.raises(ValueError, match="top_flux: expected shape"):
            nde.wm_infer_dz_flux(p.weights_truth, u, v, T, top.T, W.LZ)
        with pytest.raises(colnde.ColndeError, match="dt > 0"):
            nde.wm_embedded_step(p.weights_truth, u, v, T, top, W.LZ, -1.0, W.mpp_params())
