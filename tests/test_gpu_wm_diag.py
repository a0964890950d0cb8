"""The wind-mixing embedding's saved-state diagnoses on the GPU: `colnde_wm_diagnose_flux` (diagnose_NN_flux_uw / _vw / _wT,
wind_mixing/src/NDE_oceananigans.jl:226-286), `colnde_wm_embedded_step_flux` (the same with progress_neural_network, :380-405, in one call) and
`colnde_mpp_diagnose_flux` (diagnose_baseline_flux_*, :157-191) against the float64 restatement of tests/wm_diag_restatement.py.

Inputs: synthetic.wind_mixing_problem(200, n_frames=3, weight_divisor=1.0) through wm_embed_common.embed_inputs and
wm_diag_restatement.diag_inputs (T perturbed by a fixed profile: float32 and float64 take the same `Ri > 0` branch on every face, asserted; both
branches occur among the interior faces, asserted); weights_truth; Lz = 256; the first n columns per case.

Bounds, max|gpu − f64| / max|f64| per flux field: 10 x the distance of a float32 NumPy run of the restatement from the float64 one, computed on
the CPU on all 200 columns (the largest over halos given / absent), the project's convention:
    NN diagnosis   uw 4.46e-7 -> 4.46e-6   vw 3.98e-7 -> 3.98e-6   wT 1.16e-7 -> 1.16e-6 (ca = 0), 5.17e-8 -> 5.17e-7 (ca = 1)
    baseline, 77 columns, (uw, vw, wT):  Nz = 16  8.81e-9, 3.07e-7, 3.69e-7   Nz = 32  1.44e-8, 9.98e-8, 8.95e-8 (ca = 1: 8.96e-9)
                                         Nz = 64  2.29e-8, 1.11e-7, 8.91e-8 (ca = 1: 3.67e-9), each x 10
(the baseline's uw is that small because max|uw| is the replaced top flux, which is exact).  Measured on an MI355X, largest over the cases: NN
diagnosis uw 3.6e-7, vw 4.1e-7, wT 1.4e-7; baseline at Nz = 16 / 32 / 64: uw 6.6e-9 / 1.4e-8 / 2.1e-8, vw 1.7e-7 / 1.2e-7 / 1.1e-7, wT 2.1e-7 / 8.3e-8 /
7.0e-8.  Every run records them again (COLNDE_RECORD_ERRORS=1)."""
import ctypes
import functools

import numpy as np
import pytest

from colnde import synthetic
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W
from tests.test_gpu_parity import _record

pytestmark = pytest.mark.gpu

N_ALL = 200
DT = 60.0
FIELDS = ("uw", "vw", "wT")
NN_BOUND = {0: (4.46e-6, 3.98e-6, 1.16e-6), 1: (4.46e-6, 3.98e-6, 5.17e-7)}
BASE_N = 77
BASE_BOUND = {(16, 0): (8.81e-8, 3.07e-6, 3.69e-6), (16, 1): (8.81e-8, 3.07e-6, 3.69e-6),
              (32, 0): (1.44e-7, 9.98e-7, 8.95e-7), (32, 1): (1.44e-7, 9.98e-7, 8.96e-8),
              (64, 0): (2.29e-7, 1.11e-6, 8.91e-7), (64, 1): (2.29e-7, 1.11e-6, 3.67e-8)}


@functools.lru_cache(maxsize=None)
def _problem(Nz=32, n_all=N_ALL):
    kw = {} if Nz == 32 else {"Nz": Nz}
    p = synthetic.wind_mixing_problem(n_all, n_frames=3, weight_divisor=1.0, **kw)
    arrs = R.diag_inputs(W.embed_inputs(p), n_all)
    for a in arrs:
        a.setflags(write=False)
    return p, arrs


@functools.lru_cache(maxsize=None)
def _reference(ca, halo):
    p, (u, v, T, top, hb, ht) = _problem()
    ref = R.diagnose_NN_flux(p.cfg, p.weights_truth, u, v, T, top, W.LZ, W.MPP, bool(ca), (hb, ht) if halo else None)
    for a in ref:
        a.setflags(write=False)
    return ref


def _case(n, Nz=32, n_all=N_ALL):
    p, (u, v, T, top, hb, ht) = _problem(Nz, n_all)
    c = lambda a: np.ascontiguousarray(a[:n])
    c3 = lambda a: np.ascontiguousarray(a[:, :n])
    return p, (c(u), c(v), c(T), c3(top), c3(hb), c3(ht))


def _same_branches(u, v, T, dz, halos):
    """The precondition: float32 and float64 take the same `Ri > 0` branch on EVERY face of every column (nothing is masked out)."""
    Ri32 = R.richardson_number(u, v, T, np.float32(dz), W.MPP, halos, np.float32)
    Ri64 = R.richardson_number(u, v, T, dz, W.MPP, halos, np.float64)
    assert np.array_equal(Ri32 > 0, Ri64 > 0)
    return Ri64 > 0


def _errors(got, ref):
    return [float(np.abs(g.astype(np.float64) - r).max() / np.abs(r).max()) for g, r in zip(got, ref)]


def _cuda(*arrs):
    import torch
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def test_inputs_take_both_branches():
    _, (u, v, T, top, hb, ht) = _problem()
    pos = _same_branches(u, v, T, W.LZ / 32, (hb, ht))
    interior = pos[:, 1:32]
    assert interior.any() and (~interior).any()
    # both signs of the bottom and of the top T difference across columns
    assert (T[:, 0] > hb[2]).any() and (T[:, 0] < hb[2]).any() and (ht[2] > T[:, -1]).any() and (ht[2] < T[:, -1]).any()


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 77, 200])
def test_nn_diagnosis_parity_host_and_device_twins(n, ca, halo):
    import torch
    import colnde
    p, (u, v, T, top, hb, ht) = _case(n)
    halos = (hb, ht) if halo else None
    _same_branches(u, v, T, W.LZ / 32, halos)
    ref = tuple(r[:n] for r in _reference(ca, halo))
    with colnde.ColumnNDE(p.cfg, 4) as nde:                                      # the handle's own column count is unrelated to n
        host = nde.wm_diagnose_flux(p.weights_truth, u, v, T, top, W.LZ, W.mpp_params(), ca, halos)
        wd, ud, vd, Td, td, hbd, htd = _cuda(p.weights_truth, u, v, T, top, hb if halo else None, ht if halo else None)
        dev = nde.wm_diagnose_flux(wd, ud, vd, Td, td, W.LZ, W.mpp_params(), ca, (hbd, htd) if halo else None)
        torch.cuda.synchronize()
        dev = tuple(d.cpu().numpy() for d in dev)
    errs = _errors(host, ref)
    print("wm_diagnose_flux n=%d ca=%d halo=%d: rel err uw %.3e vw %.3e wT %.3e" % ((n, ca, halo) + tuple(errs)))
    _record("wm_diagnose_flux/%d/%d/%d" % (n, ca, halo), **dict(zip(FIELDS, errs)))
    for h_, d_ in zip(host, dev):
        assert h_.shape == (n, 33) and np.isfinite(h_).all() and np.array_equal(h_, d_)              # twins: bit for bit
    for nm, e, b in zip(FIELDS, errs, NN_BOUND[ca]):
        assert e <= b, (nm, e, b)


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
@pytest.mark.parametrize("n", [1, 33, 77])
def test_step_flux_bit_identities(n, ca, halo):
    import torch
    import colnde
    p, (u, v, T, top, hb, ht) = _case(n)
    outs = []
    for ma in ("bf16x3_exact", "f32_mfma"):
        with colnde.ColumnNDE(p.cfg, 4, matrix_arithmetic=ma) as nde:
            wd, td, hbd, htd = _cuda(p.weights_truth, top, hb if halo else None, ht if halo else None)
            halos = (hbd, htd) if halo else None
            ud, vd, Td = _cuda(u, v, T)
            alone = nde.wm_diagnose_flux(wd, ud, vd, Td, td, W.LZ, W.mpp_params(), ca, halos)
            step = nde.wm_embedded_step(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, hbd)
            a = nde.wm_embedded_step_flux(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, halos)    # out of place
            b = nde.wm_embedded_step_flux(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, halos)    # a second launch
            torch.cuda.synchronize()
            assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip((ud, vd, Td), (u, v, T)))  # inputs untouched
            c = nde.wm_embedded_step_flux(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), ca, halos, out=(ud, vd, Td))       # in place
            torch.cuda.synchronize()
            assert c[1][0].data_ptr() == ud.data_ptr()
            flat = lambda r: tuple(x.cpu().numpy() for part in r for x in part)
            a, b, c = flat(a), flat(b), flat(c)
            want = tuple(x.cpu().numpy() for x in step[0] + step[1] + alone)
            host = nde.wm_embedded_step_flux(p.weights_truth, u, v, T, top, W.LZ, DT, W.mpp_params(), ca, (hb, ht) if halo else None)
            host = tuple(x for part in host for x in part)
        for x, y, z, w_, h_ in zip(a, b, c, want, host):
            assert np.isfinite(x).all()
            assert np.array_equal(x, w_)          # ∂z, u′ v′ T′: wm_embedded_step_dev's bits; faces: wm_diagnose_flux_dev's
            assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, h_)
        outs.append(a)
    assert all(np.array_equal(x, y) for x, y in zip(*outs))                                          # both matrix arithmetics, equal bits


def test_exact_properties():
    import colnde
    n = 77
    p, (u, v, T, top, hb, ht) = _case(n)
    pr = W.mpp_params()
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        for ca in (0, 1):
            for halos in (None, (hb, ht)):
                a = nde.wm_diagnose_flux(p.weights_truth, u, v, T, top, W.LZ, pr, ca, halos)
                d = nde.wm_diagnose_flux(p.weights_truth, u, v, T, 2 * top, W.LZ, pr, ca, halos)
                b = nde.mpp_diagnose_flux(u, v, T, top, W.LZ / 32, pr, ca, None if halos is None else hb)
                b2 = nde.mpp_diagnose_flux(u, v, T, 2 * top, W.LZ / 32, pr, ca, None if halos is None else hb)
                for k in range(3):
                    assert np.array_equal(b[k][:, -1], top[k])                                       # baseline: the top face IS the top flux
                    assert np.array_equal(a[k][:, :-1], d[k][:, :-1]) and np.array_equal(b[k][:, :-1], b2[k][:, :-1])     # doubling it changes that face only
                    assert np.array_equal(b2[k][:, -1], 2 * top[k])
                    moved = top[k] != 0                                                          # (this problem's vw top flux is zero)
                    assert (a[k][:, -1] != d[k][:, -1])[moved].all() and np.array_equal(a[k][:, -1][~moved], d[k][:, -1][~moved])
                for k in range(2):
                    assert np.array_equal(np.abs(a[k][:, 0]), np.zeros(n, np.float32))               # face 0 of uw, vw: ±0
                    assert np.array_equal(np.abs(b[k][:, 0]), np.zeros(n, np.float32))
                    assert np.array_equal(a[k][:, -1], top[k]) and np.array_equal(d[k][:, -1], 2 * top[k])     # NN uw, vw at the top: top − 0·g
        f = colnde.wind_mixing.diagnose_NN_flux(nde, p.weights_truth, u[3], v[3], T[3], top[:, 3], W.LZ, W.MPP, W.MPP, True, (hb[:, 3], ht[:, 3]))
        g = colnde.wind_mixing.diagnose_baseline_flux(nde, u[3], v[3], T[3], top[:, 3], W.LZ, W.MPP, W.MPP, True, (hb[:, 3], None))
    for k in range(3):
        assert f[k].shape == g[k].shape == (33,) and np.array_equal(f[k], a[k][3]) and np.array_equal(g[k], b[k][3])


def test_beyond_one_pass_of_the_persistent_grid():
    """More columns than grid x 128 (one workgroup per CU, four 32-column tiles each): the only case that runs the next-group prefetch.  Every
    cyclic replica of the 200 columns must be bit-identical to its original."""
    import torch
    import colnde
    p, (u, v, T, top, hb, ht) = _case(N_ALL)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rep = (n_cu * 128) // N_ALL + 2
    n = rep * N_ALL
    assert n > n_cu * 128
    t = lambda a: torch.from_numpy(a).cuda()
    ud, vd, Td = (t(a).repeat(rep, 1).contiguous() for a in (u, v, T))
    td, hbd, htd = (t(a).repeat(1, rep).contiguous() for a in (top, hb, ht))
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        wd = t(p.weights_truth)
        small = nde.wm_embedded_step_flux(wd, t(u), t(v), t(T), t(top), W.LZ, DT, W.mpp_params(), 1, (t(hb), t(ht)))
        alone = nde.wm_diagnose_flux(wd, ud, vd, Td, td, W.LZ, W.mpp_params(), 1, (hbd, htd))
        big = nde.wm_embedded_step_flux(wd, ud, vd, Td, td, W.LZ, DT, W.mpp_params(), 1, (hbd, htd))
        torch.cuda.synchronize()
        small = tuple(x for part in small for x in part)
        big = tuple(x for part in big for x in part)
        for s_, b_ in zip(small + small[6:], big + tuple(alone)):
            assert bool(torch.isfinite(b_).all())
            assert torch.equal(b_.view(rep, N_ALL, -1), s_.unsqueeze(0).expand(rep, -1, -1))


@pytest.mark.parametrize("Nz", [16, 32, 64])
def test_baseline_diagnosis_parity(Nz):
    import torch
    import colnde
    n = BASE_N
    p, (u, v, T, top, hb, ht) = _case(n, Nz, BASE_N)
    dz = W.LZ / Nz
    hcfg = synthetic.free_convection_problem(1, Nz=Nz, n_save=2).cfg            # any handle kind: only Nz is the handle's
    for ca in (0, 1):
        for halo in (False, True):
            halos = (hb, None) if halo else None
            _same_branches(u, v, T, dz, halos)
            ref = R.diagnose_baseline_flux(u, v, T, top, dz, W.MPP, bool(ca), halos)
            with colnde.ColumnNDE(hcfg, 1) as nde:
                host = nde.mpp_diagnose_flux(u, v, T, top, dz, W.mpp_params(), ca, hb if halo else None)
                ud, vd, Td, td, hbd = _cuda(u, v, T, top, hb if halo else None)
                dev = nde.mpp_diagnose_flux(ud, vd, Td, td, dz, W.mpp_params(), ca, hbd)
                torch.cuda.synchronize()
                dev = tuple(d.cpu().numpy() for d in dev)
            errs = _errors(host, ref)
            print("mpp_diagnose_flux Nz=%d ca=%d halo=%d: rel err uw %.3e vw %.3e wT %.3e" % ((Nz, ca, halo) + tuple(errs)))
            _record("mpp_diagnose_flux/%d/%d/%d" % (Nz, ca, halo), **dict(zip(FIELDS, errs)))
            for h_, d_ in zip(host, dev):
                assert h_.shape == (n, Nz + 1) and np.isfinite(h_).all() and np.array_equal(h_, d_)
            for nm, e, b in zip(FIELDS, errs, BASE_BOUND[(Nz, ca)]):
                assert e <= b, (nm, e, b)


def _raw(nde, n=4, Lz=W.LZ, misalign=False):
    """colnde_wm_diagnose_flux[_dev] / colnde_wm_embedded_step_flux straight through ctypes (the refusals of the C ABI, not of the wrapper)."""
    z = lambda *s: np.zeros(s, np.float32)
    m = max(n, 1)
    w, u, top, o, f = z(20000), z(m, 32), z(3, m), [z(m, 32) for _ in range(6)], [z(m, 33) for _ in range(3)]
    pr = (ctypes.c_float * 7)(*W.mpp_params())
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L = nde._L
    if misalign:
        import torch
        buf = torch.zeros(8 * m * 33 + 16, device="cuda")
        wd = torch.zeros(20000, device="cuda")
        q = lambda i, off=0: buf.data_ptr() + 4 * (i * m * 33 + off)
        r = L.colnde_wm_diagnose_flux_dev(nde._h, wd.data_ptr(), q(0), q(1), q(2), q(3), None, None, ctypes.c_float(Lz), pr, 0, q(4), q(5, 1), q(6), n)
        return r, L.colnde_last_error().decode(), r, L.colnde_last_error().decode()
    r1 = L.colnde_wm_diagnose_flux(nde._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(Lz), pr, 0, P(f[0]), P(f[1]), P(f[2]), n)
    m1 = L.colnde_last_error().decode()
    r2 = L.colnde_wm_embedded_step_flux(nde._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(Lz), ctypes.c_float(DT), pr, 0, P(o[0]), P(o[1]),
                                        P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(f[0]), P(f[1]), P(f[2]), n)
    return r1, m1, r2, L.colnde_last_error().decode()


def test_refusals_name_the_reason():
    import colnde
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1.0)

    def refused(nde, match, **kw):
        r1, m1, r2, m2 = _raw(nde, **kw)
        assert r1 != 0 and r2 != 0
        assert match in m1 and match in m2, (m1, m2)

    fc = synthetic.free_convection_problem(8, Nz=32, n_save=3)
    with colnde.ColumnNDE(fc.cfg, 8) as nde:
        refused(nde, "needs a wind-mixing handle")
    with colnde.ColumnNDEEnsemble(p.cfg, 8, 2) as e:
        refused(e, "holds an ensemble of 2 models")
    with colnde.ColumnNDE(p.cfg.with_(smooth_NN=True), 8) as nde:
        refused(nde, "no smoothing filter")
    wide = synthetic.wind_mixing_problem(8, n_frames=3, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
    with colnde.ColumnNDE(wide.cfg, 8) as nde:
        refused(nde, "three 96-50-20-31 networks")
    with colnde.ColumnNDE(p.cfg, 8) as nde:
        refused(nde, "n_columns >= 1 and Lz > 0", n=0)
        refused(nde, "n_columns >= 1 and Lz > 0", Lz=0.0)
        refused(nde, "16-byte aligned", misalign=True)
