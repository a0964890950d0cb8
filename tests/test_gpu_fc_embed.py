"""The free-convection embedded step on the GPU: `colnde_fc_embedded_step` (progress_neural_network, free_convection/src/oceananigans_nn.jl:153-165)
and `colnde_fc_diagnose_wT` (diagnose_wT_NN, :100-118) against the two existing launches, bit for bit, and against the float64 restatement of
tests/fc_embed_restatement.py.

Inputs: synthetic.inference_problem's network (weights / 1e2) at Nz = 32 and 64; 65 columns of fc_embed_restatement.switch_robust_case (every
centred and face gradient at least 0.2 x 32/Nz from zero: float32 and float64 take the same switches, asserted per case), the first n per case;
Lz = 1000, dt = 600.  Both tile widths are forced through COLNDE_FC_CW (the call reads it), so every n runs on 16- and on 32-column tiles.

Bounds.  T′: 2e-5 of max|T′| (tests/test_column_ops.py, convadj_kernel).  ∂z wT: relative L2 error 2e-6 (tests/test_gpu_fc.py, fc_infer_kernel).
wT_faces, max|gpu − f64| / max|f64|: 10 x the distance of a float32 NumPy run of the restatement from the float64 one on these inputs, the largest
over both Nz, halos given / absent and the six sizes — K = 10: 1.07e-7 -> 1.07e-6; K = 1e-3 (κ ∂T/∂z of the size of the network's flux): 1.72e-7 ->
1.72e-6.  Measured on an MI355X, largest over the cases: wT_faces 1.2e-7 (K = 10), 1.9e-7 (K = 1e-3), ∂z wT 2.3e-7, T′ 1.6e-6; every run
records them again (COLNDE_RECORD_ERRORS=1) so that the bounds can be tightened."""
import ctypes
import functools

import numpy as np
import pytest

from colnde import synthetic
from tests import fc_embed_restatement as R
from tests.test_gpu_parity import _record, _rel

pytestmark = pytest.mark.gpu

LZ, DT = 1000.0, 600.0
N_ALL = 65
SIZES = [1, 15, 17, 31, 33, 65]
T_TOL, DZ_REL = 2e-5, 2e-6
FACES_BOUND = {10.0: 1.07e-6, 1e-3: 1.72e-6}


@functools.lru_cache(maxsize=None)
def _problem(Nz):
    cfg, _, _, w = synthetic.inference_problem(1, 1, Nz=Nz)              # make_weights(..., 1e2): the net matters
    T, top, hb, ht = R.switch_robust_case(Nz, N_ALL)
    for a in (w, T, top, hb, ht):
        a.setflags(write=False)
    return cfg, w, (T, top, hb, ht)


@functools.lru_cache(maxsize=None)
def _reference(Nz, K, halo):
    cfg, w, (T, top, hb, ht) = _problem(Nz)
    ref = R.embedded_step(cfg, w, T, top, LZ, DT, K, (hb, ht) if halo else None)
    for a in ref:
        a.setflags(write=False)
    return ref


def _case(Nz, n):
    cfg, w, arrs = _problem(Nz)
    return cfg, w, tuple(np.ascontiguousarray(a[:n]) for a in arrs)


def _same_switches(T, halos):
    """float32 and float64 take the same κ switches in EVERY column (no column is dropped from a comparison)."""
    T64 = T.astype(np.float64)
    h64 = None if halos is None else tuple(a.astype(np.float64) for a in halos)
    assert np.array_equal(R.centred_switch(T, halos), R.centred_switch(T64, h64))
    assert np.array_equal(R.face_switch(T, halos), R.face_switch(T64, h64))


def _faces_err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def _cuda(*arrs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def test_inputs_cover_the_switch_patterns():
    _, _, (T, top, hb, ht) = _problem(32)
    f = R.face_switch(T, (hb, ht))
    assert (~f[0]).all() and f[1].all()                                       # an all-stable and an all-unstable column
    assert (f[2, 1:] != f[2, :-1]).all()                                       # an alternating one
    assert 0 < f[3].sum() < f.shape[1]


@pytest.mark.parametrize("cw", [16, 32])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("Nz", [32, 64])
def test_fused_step_against_the_two_launches_and_float64(Nz, n, cw, monkeypatch):
    import torch
    import colnde
    monkeypatch.setenv("COLNDE_FC_CW", str(cw))
    K = 10.0
    cfg, w, (T, top, hb, ht) = _case(Nz, n)
    _same_switches(T, (hb, ht))
    ref = tuple(r[:n] for r in _reference(Nz, K, True))
    dz = float(np.float32(LZ) / np.float32(Nz))
    with colnde.ColumnNDE(cfg, 4) as nde:                                      # the handle's own column count is unrelated to n
        assert "fc_embed=f32" in nde.describe()
        wd, Td, td, hbd, htd = _cuda(w, T, top, hb, ht)
        three = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, (hbd, htd), diagnose=True)
        two = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, (hbd, htd))         # as shipped: the two launches ...
        monkeypatch.setenv("COLNDE_FC_EMBED_FUSED", "1")
        nde.reset_kernel_times()
        nde.set_profiling(True)
        fused = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, (hbd, htd))       # ... and the fused forcing + adjustment kernel
        nde.set_profiling(False)
        assert nde.kernel_time("fc_embed")[1] == 1 and nde.kernel_time("infer")[1] == 0
        monkeypatch.delenv("COLNDE_FC_EMBED_FUSED")
        alone = nde.fc_diagnose_wT(wd, Td, td, LZ, K, (hbd, htd))
        pair = (nde.infer_dz_wT(wd, Td, td, LZ), nde.convective_adjustment(Td, DT, dz, K, hbd, htd))
        torch.cuda.synchronize()
        assert np.array_equal(Td.cpu().numpy(), T)                             # out of place: the input survives
        three, two, fused, pair = (tuple(a.cpu().numpy() for a in x) for x in (three, two, fused, pair))
        alone = alone.cpu().numpy()
    assert all(np.isfinite(a).all() for a in three)
    assert np.array_equal(three[0], pair[0])                                   # ∂z wT: colnde_infer_dz_wT_dev's bits
    assert np.array_equal(three[1], pair[1])                                   # T′: colnde_convective_adjustment_dev's bits
    assert np.array_equal(two[0], three[0]) and np.array_equal(two[1], three[1])
    assert np.array_equal(fused[0], three[0]) and np.array_equal(fused[1], three[1])
    assert np.array_equal(alone, three[2])                                     # diagnosis only = the faces of the three-output mode
    errs = dict(dz_rel=_rel(three[0], ref[0]), T_rel_max=float(np.abs(three[1] - ref[1]).max() / np.abs(ref[1]).max()), faces=_faces_err(three[2], ref[2]))
    print("fc_embed Nz=%d n=%d cw=%d: %s" % (Nz, n, cw, errs))
    _record("fc_embed/%d/%d/cw%d" % (Nz, n, cw), **errs)
    assert errs["T_rel_max"] <= T_TOL
    assert errs["dz_rel"] < DZ_REL
    assert errs["faces"] <= FACES_BOUND[K]


@pytest.mark.parametrize("cw", [16, 32])
@pytest.mark.parametrize("Nz", [32, 64])
def test_diagnosis_where_the_network_flux_matters(Nz, cw, monkeypatch):
    """K = 1e-3: κ ∂T/∂z is of the size of the network's flux, so an error in F shows in the faces (at K = 10 the gradient term dominates)."""
    import colnde
    monkeypatch.setenv("COLNDE_FC_CW", str(cw))
    K = 1e-3
    for halo in (False, True):
        cfg, w, (T, top, hb, ht) = _case(Nz, 33)
        halos = (hb, ht) if halo else None
        _same_switches(T, halos)
        ref = _reference(Nz, K, halo)[2][:33]
        with colnde.ColumnNDE(cfg, 4) as nde:
            got = nde.fc_diagnose_wT(w, T, top, LZ, K, halos)
        e = _faces_err(got, ref)
        print("fc_diagnose Nz=%d cw=%d halo=%d: %.3e" % (Nz, cw, halo, e))
        _record("fc_diagnose/%d/cw%d/%d" % (Nz, cw, halo), faces=e)
        assert got.shape == (33, Nz + 1) and e <= FACES_BOUND[K]
        stable = ~R.face_switch(T, halos)
        F = R.faces(cfg, w, T, top)
        assert np.abs(got[stable] - F[stable]).max() <= FACES_BOUND[K] * np.abs(F).max()      # κ = 0: the face is the network's flux


@pytest.mark.parametrize("Nz", [32, 64])
def test_null_halos_alias_and_host_twin(Nz):
    import torch
    import colnde
    n, K = 33, 10.0
    cfg, w, (T, top, _, _) = _case(Nz, n)
    _same_switches(T, None)
    ref = tuple(r[:n] for r in _reference(Nz, K, False))
    with colnde.ColumnNDE(cfg, 4) as nde:
        wd, Td, td = _cuda(w, T, top)
        null = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, None, diagnose=True)
        near = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, _cuda(T[:, 0], T[:, -1]), diagnose=True)     # the nearest interior value, explicitly
        one = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, (None, _cuda(T[:, -1])[0]), diagnose=True)
        inplace = nde.fc_embedded_step(wd, Td, td, LZ, DT, K, None, diagnose=True, T_out=Td)          # T_out is T
        torch.cuda.synchronize()
        assert inplace[1].data_ptr() == Td.data_ptr()
        host = nde.fc_embedded_step(w, T, top, LZ, DT, K, None, diagnose=True)                          # numpy path
        host_faces = nde.fc_diagnose_wT(w, T, top, LZ, K)
        null, near, one, inplace = (tuple(a.cpu().numpy() for a in x) for x in (null, near, one, inplace))
    for a, b, c, d, e in zip(null, near, one, inplace, host):
        assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(a, e)
    assert np.array_equal(host_faces, null[2])
    assert np.array_equal(null[2][:, 0], np.zeros(n, np.float32))               # face 0: no flux, no gradient
    assert np.abs(null[1] - ref[1]).max() <= T_TOL * np.abs(ref[1]).max() and _rel(null[0], ref[0]) < DZ_REL
    assert _faces_err(null[2], ref[2]) <= FACES_BOUND[K]
    stable = np.arange(n) % 4 == 0
    assert np.array_equal(null[1][stable], T[stable])                           # all-stable columns: T′ == T, bit for bit


def test_tile_width_threshold_and_reference_named_mirrors(monkeypatch):
    """4,097 columns: the first size on 32-column tiles without forcing (fc_tile_width); the fused kernel's bits against the two launches only."""
    monkeypatch.setenv("COLNDE_FC_EMBED_FUSED", "1")
    import torch
    import colnde
    from colnde import free_convection as FC
    Nz, n, K = 32, 4097, 10.0
    cfg, w, (T, top, hb, ht) = _case(Nz, N_ALL)
    rep = (n + N_ALL - 1) // N_ALL
    T, top = np.ascontiguousarray(np.tile(T, (rep, 1))[:n]), np.ascontiguousarray(np.tile(top, rep)[:n])
    with colnde.ColumnNDE(cfg, 4) as nde:
        wd, Td, td = _cuda(w, T, top)
        dzw, Tn = nde.fc_embedded_step(wd, Td, td, LZ, DT, K)
        pair = (nde.infer_dz_wT(wd, Td, td, LZ), nde.convective_adjustment(Td, DT, LZ / Nz, K))
        torch.cuda.synchronize()
        assert torch.equal(dzw, pair[0]) and torch.equal(Tn, pair[1])
        # the mirrors of free_convection.py on an [nx, ny, Nz] field
        a = FC.progress_neural_network(nde, w, T[:48].reshape(8, 6, Nz), top[:48].reshape(8, 6), LZ, DT, K)
        f = FC.diagnose_wT_NN(nde, w, T[:48].reshape(8, 6, Nz), top[:48].reshape(8, 6), LZ, K)
        b = nde.fc_embedded_step(w, T[:48], top[:48], LZ, DT, K, diagnose=True)
    assert a[0].shape == a[1].shape == (8, 6, Nz) and f.shape == (8, 6, Nz + 1)
    assert np.array_equal(a[0].reshape(48, Nz), b[0]) and np.array_equal(a[1].reshape(48, Nz), b[1]) and np.array_equal(f.reshape(48, Nz + 1), b[2])


def _raw(nde, Nz, n=4, Lz=LZ, K=1.0):
    """colnde_fc_diagnose_wT / colnde_fc_embedded_step straight through ctypes (the refusals of the C ABI, not of the Python wrapper)."""
    z = lambda *s: np.zeros(s, np.float32)
    m = max(n, 1)
    w, T, top, o, f = z(200000), z(m, Nz), z(m), z(m, Nz), z(m, Nz + 1)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    r1 = nde._L.colnde_fc_diagnose_wT(nde._h, P(w), P(T), P(top), None, None, ctypes.c_float(Lz), ctypes.c_float(K), P(f), n)
    m1 = nde._L.colnde_last_error().decode()
    r2 = nde._L.colnde_fc_embedded_step(nde._h, P(w), P(T), P(top), None, None, ctypes.c_float(Lz), ctypes.c_float(DT), ctypes.c_float(K), P(o), P(o.copy()),
                                        None, n)
    return r1, m1, r2, nde._L.colnde_last_error().decode()


def test_refusals_name_the_reason():
    import colnde

    def refused(nde, match, Nz=32, **kw):
        r1, m1, r2, m2 = _raw(nde, Nz, **kw)
        assert r1 != 0 and r2 != 0
        assert match in m1 and match in m2, (m1, m2)

    wm = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1.0)
    with colnde.ColumnNDE(wm.cfg, 8) as nde:
        refused(nde, "needs a free-convection handle")
        assert "fc_embed" not in nde.describe()
    with colnde.ColumnNDEEnsemble(wm.cfg, 8, 2) as e:
        refused(e, "holds an ensemble of 2 models")
    with colnde.ClosureColumns(wm.cfg, 8, 2) as c:
        refused(c, "closure handle")
    with colnde.ColumnNDE(synthetic.free_convection_problem(8, Nz=16, n_save=3).cfg, 8) as nde:
        refused(nde, "covers Nz = 32 or 64 (this handle has Nz = 16)", Nz=16)
    with colnde.ColumnNDE(synthetic.free_convection_problem(8, Nz=32, n_save=3, layer_sizes=(32, 64, 64, 31)).cfg, 8) as nde:
        refused(nde, "this handle has Nz = 32 and network 32-64-64-31")
    cfg, w, (T, top, hb, ht) = _case(32, 4)
    with colnde.ColumnNDE(cfg, 8) as nde:
        refused(nde, "n_columns >= 1 and Lz > 0", n=0)
        refused(nde, "n_columns >= 1 and Lz > 0", Lz=0.0)
        refused(nde, "K >= 0", K=-1.0)
        with pytest.raises(colnde.ColndeError, match="dt > 0"):
            nde.fc_embedded_step(w, T, top, LZ, 0.0, 1.0)
        with pytest.raises(ValueError, match="top_flux: expected shape"):
            nde.fc_diagnose_wT(w, T, top[:3], LZ, 1.0)
