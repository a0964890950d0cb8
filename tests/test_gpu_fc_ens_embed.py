"""The K networks of a free-convection ensemble in the embedding at once, on the GPU: `colnde_ensemble_fc_embedded` against the
single-model entry points, bit for bit; conv ensembles against the K = 1 call on a single conv handle; every output of every member against the
float64 restatement of tests/fc_embed_restatement.py (conv members: on the `conv_to_dense` network); weight reuse, in place, refusals.

Inputs, references and tolerances: tests/fc_ens_embed_cases.py (K = 3 members on their own states, Nz = 32 | 64, n = 1 | 16 | 19 and 33 once).
Measured on an MI355X, largest over the cases — plain: ∂z wT 7.3e-8, T′ 1.6e-6, faces 1.3e-7 (K_ca = 10) and 1.5e-7 (1e-3); conv: ∂z wT
1.1e-7 (bound 3.84e-7), faces 1.3e-7 and 1.5e-7.  Every run records them again under COLNDE_RECORD_ERRORS=1."""
import ctypes

import numpy as np
import pytest

from tests import fc_ens_embed_cases as C
from tests.test_gpu_parity import _record

pytestmark = pytest.mark.gpu

K = C.K_MODELS
LZ, DT = C.LZ, C.DT


def _cuda(*arrs):
    import torch
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs)


def _np(r):
    return tuple(None if a is None else a.cpu().numpy() for a in r)


def _ensemble(Nz, c=0):
    import colnde
    return colnde.FreeConvectionEnsemble(C.config(Nz), 4, K, conv=c)            # the handle's own column count is unrelated to n


def _check_float64(tag, kind, got, Nz, c, n, halo, K_ca, step, faces):
    ref = C.reference(Nz, c, K_ca, halo)
    errs = {}
    for k in range(K):
        if step:
            errs["dz_rel"] = max(errs.get("dz_rel", 0.0), C.rel_l2(got[0][k], ref[0][k, :n]))
            errs["T_rel_max"] = max(errs.get("T_rel_max", 0.0), float(np.abs(got[1][k] - ref[1][k, :n]).max() / np.abs(ref[1][k, :n]).max()))
        if faces:
            errs["faces"] = max(errs.get("faces", 0.0), C.faces_err(got[2][k], ref[2][k, :n]))
    print("fc_ens_embed %s: %s" % (tag, errs))
    _record("fc_ens_embed/" + tag, **errs)
    assert all(np.isfinite(a).all() for a in got if a is not None)
    if step:
        assert errs["T_rel_max"] <= C.T_TOL
        assert errs["dz_rel"] < (C.DZ_REL_CONV if c else C.DZ_REL_PLAIN)
    if faces:
        assert errs["faces"] <= C.FACES_BOUND[(kind, K_ca)]


MODES = {"step": (True, False, C.K_STEP), "step+faces": (True, True, C.K_STEP), "faces": (False, True, C.K_DIAG)}


@pytest.mark.parametrize("halo", [True, False])
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("Nz", [32, 64])
def test_plain_ensemble_rows_are_the_single_handles_bits_and_float64(Nz, n, halo):
    import torch
    import colnde
    T, top, hb, ht = C.case(Nz, n)
    halos = (hb, ht) if halo else None
    C.same_switches(T, halos)
    W = C.weights(Nz)
    Wd, Td, td, hbd, htd = _cuda(W, T, top, hb if halo else None, ht if halo else None)
    hd = (hbd, htd) if halo else None
    with _ensemble(Nz) as ens, colnde.ColumnNDE(C.config(Nz), 4) as one:
        assert "fc_embed=f32" in one.describe()
        for mode, (step, faces, K_ca) in MODES.items():
            ens.reset_kernel_times()
            ens.set_profiling(True)
            r = ens.fc_embedded(Wd, Td, td, LZ, K_ca, DT if step else None, hd, step=step, faces=faces)
            ens.set_profiling(False)
            assert ens.kernel_time("fc_embed")[1] == 1 and ens.kernel_time("infer")[1] == 0 and ens.kernel_time("convadj")[1] == 0     # ONE launch
            got = _np(r)
            for k in range(K):
                hk = None if hd is None else (hbd[k].contiguous(), htd[k].contiguous())
                Tk = Td[k].contiguous()
                if step:
                    s = one.fc_embedded_step(Wd[k].contiguous(), Tk, td, LZ, DT, K_ca, hk, diagnose=faces)     # faces=False: the default pair of launches
                    assert np.array_equal(got[0][k], s[0].cpu().numpy()) and np.array_equal(got[1][k], s[1].cpu().numpy()), (mode, k)
                    if faces:
                        assert np.array_equal(got[2][k], s[2].cpu().numpy()), (mode, k)
                else:
                    assert np.array_equal(got[2][k], one.fc_diagnose_wT(Wd[k].contiguous(), Tk, td, LZ, K_ca, hk).cpu().numpy()), (mode, k)
            assert not step or not np.array_equal(got[0][0], got[0][1])          # the members differ
            _check_float64("plain/%d/%d/%d/%s" % (Nz, n, halo, mode), "plain", got, Nz, 0, n, halo, K_ca, step, faces)
        torch.cuda.synchronize()
        assert np.array_equal(Td.cpu().numpy(), T)                                # out of place: the input survives


@pytest.mark.parametrize("halo", [True, False])
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("Nz", [32, 64])
def test_conv_ensemble_rows_are_the_single_conv_handles_bits_and_float64(Nz, n, halo):
    import colnde
    c = 3
    T, top, hb, ht = C.case(Nz, n)
    halos = (hb, ht) if halo else None
    C.same_switches(T, halos)
    W = C.weights(Nz, c)
    Wd, Td, td, hbd, htd = _cuda(W, T, top, hb if halo else None, ht if halo else None)
    hd = (hbd, htd) if halo else None
    dz = float(np.float32(LZ) / np.float32(Nz))
    with _ensemble(Nz, c) as ens, colnde.ColumnNDE(C.config(Nz), 4, conv=c) as one:
        for mode, (step, faces, K_ca) in MODES.items():
            got = _np(ens.fc_embedded(Wd, Td, td, LZ, K_ca, DT if step else None, hd, step=step, faces=faces))
            for k in range(K):
                hk = None if hd is None else (hbd[k:k + 1].contiguous(), htd[k:k + 1].contiguous())
                s = _np(one.fc_embedded(Wd[k:k + 1].contiguous(), Td[k:k + 1].contiguous(), td, LZ, K_ca, DT if step else None, hk, step=step, faces=faces))
                for a, b in zip(got, s):
                    assert (a is None and b is None) or np.array_equal(a[k], b[0]), (mode, k)
                if step:                                                         # the sweep never sees the filter: colnde_convective_adjustment_dev's bits
                    ca = one.convective_adjustment(Td[k].contiguous(), DT, dz, K_ca, None if hd is None else hbd[k].contiguous(),
                                                   None if hd is None else htd[k].contiguous())
                    assert np.array_equal(got[1][k], ca.cpu().numpy()), (mode, k)
            _check_float64("conv3/%d/%d/%d/%s" % (Nz, n, halo, mode), "conv", got, Nz, c, n, halo, K_ca, step, faces)
        # the existing single-model entry points keep refusing a conv handle
        with pytest.raises(colnde.ColndeError, match="does not cover the convolutional first layer"):
            one.fc_embedded_step(Wd[0].contiguous(), Td[0].contiguous(), td, LZ, DT, 1.0)
        with pytest.raises(colnde.ColndeError, match="does not cover the convolutional first layer"):
            one.fc_diagnose_wT(Wd[0].contiguous(), Td[0].contiguous(), td, LZ, 1.0)


@pytest.mark.parametrize("c", [2, 8])
@pytest.mark.parametrize("Nz", [32, 64])
def test_other_filter_lengths_against_float64(Nz, c):
    """c = 2 and c = FC_CONV_MAX = 8, through the host twin (NumPy arrays) on a single conv handle per member and on the ensemble."""
    import colnde
    n, halo = 19, True
    T, top, hb, ht = C.case(Nz, n)
    C.same_switches(T, (hb, ht))
    W = C.weights(Nz, c)
    with _ensemble(Nz, c) as ens:
        for mode, (step, faces, K_ca) in MODES.items():
            if mode == "step":
                continue
            got = tuple(ens.fc_embedded(W, T, top, LZ, K_ca, DT if step else None, (hb, ht), step=step, faces=faces))
            _check_float64("conv%d/%d/%d/%d/%s" % (c, Nz, n, halo, mode), "conv", got, Nz, c, n, halo, K_ca, step, faces)
            if step:
                with colnde.ColumnNDE(C.config(Nz), 4, conv=c) as one:           # a single conv network, deployed: K = 1
                    s = one.fc_embedded(W[2:3], T[2:3], top, LZ, K_ca, DT, (hb[2:3], ht[2:3]))
                for a, b in zip(got, s):
                    assert np.array_equal(a[2], b[0])


@pytest.mark.parametrize("c", [0, 3])
def test_third_tile_weight_reuse_in_place_and_mirrors(c):
    """n = 33 once (three tiles); weights=None returns the bits of the call that packed; after other weights, those; T_out is T; the
    reference-named mirrors of free_convection.py."""
    import torch
    import colnde
    from colnde import free_convection as FC
    Nz, n = 32, C.N_ALL
    T, top, hb, ht = C.case(Nz, n)
    C.same_switches(T, None)
    W = C.weights(Nz, c)
    W2 = np.ascontiguousarray(W[::-1])                                           # other weights: the members in reverse order
    with _ensemble(Nz, c) as ens:
        Wd, W2d, Td, td = _cuda(W, W2, T, top)
        with pytest.raises(colnde.ColndeError, match="colnde_ensemble_fc_embedded_dev: weights == NULL"):
            ens.fc_embedded(None, Td, td, LZ, C.K_STEP, DT)                     # nothing packed yet
        first = _np(ens.fc_embedded(Wd, Td, td, LZ, C.K_STEP, DT))
        _check_float64("reuse/c%d" % c, "conv" if c else "plain", first, Nz, c, n, False, C.K_STEP, True, True)
        again = _np(ens.fc_embedded(None, Td, td, LZ, C.K_STEP, DT))
        other = _np(ens.fc_embedded(W2d, Td, td, LZ, C.K_STEP, DT))
        other_again = _np(ens.fc_embedded(None, Td, td, LZ, C.K_STEP, DT))
        faces_only = _np(ens.fc_embedded(None, Td, td, LZ, C.K_STEP, None, step=False))
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
        for a, b in zip(other, other_again):
            assert np.array_equal(a, b)
        assert not np.array_equal(first[0], other[0]) and np.array_equal(first[1], other[1])        # the forcing is the network's, the sweep is not
        assert np.array_equal(faces_only[2], other[2]) and faces_only[0] is None and faces_only[1] is None
        # every member on the same state: member 0 of W is member 2 of W2
        same = np.ascontiguousarray(np.broadcast_to(T[:1], T.shape))
        a = ens.fc_embedded(W, same, top, LZ, C.K_STEP, DT)
        b = ens.fc_embedded(W2, same, top, LZ, C.K_STEP, DT)
        assert all(np.array_equal(x[0], y[2]) for x, y in zip(a, b))
        # in place
        Ti = Td.clone()
        inplace = ens.fc_embedded(W2d, Ti, td, LZ, C.K_STEP, DT, dz_out=torch.empty_like(Ti), T_out=Ti)
        torch.cuda.synchronize()
        assert inplace.T_new.data_ptr() == Ti.data_ptr()
        for x, y in zip(_np(inplace), other):
            assert np.array_equal(x, y)
        # the mirrors, on an [K, 3, 11, Nz] field
        m = FC.ensemble_progress_neural_network(ens, W2, T.reshape(K, 3, 11, Nz), top.reshape(3, 11), LZ, DT, C.K_STEP, diagnose=True)
        f = FC.ensemble_diagnose_wT_NN(ens, None, T.reshape(K, 3, 11, Nz), top.reshape(3, 11), LZ, C.K_STEP)
        assert m[0].shape == m[1].shape == (K, 3, 11, Nz) and m[2].shape == f.shape == (K, 3, 11, Nz + 1)
        assert all(np.array_equal(x.reshape(y.shape), y) for x, y in zip(m, other)) and np.array_equal(f, m[2])


def test_single_plain_handle_is_k_1():
    import colnde
    Nz, n = 64, 19
    T, top, hb, ht = C.case(Nz, n)
    w = C.weights(Nz)[1]
    with colnde.ColumnNDE(C.config(Nz), 4) as one:
        r = one.fc_embedded(w[None], T[1:2], top, LZ, C.K_STEP, DT, (hb[1:2], ht[1:2]))
        s = one.fc_embedded_step(w, T[1], top, LZ, DT, C.K_STEP, (hb[1], ht[1]), diagnose=True)
    for a, b in zip(r, s):
        assert np.array_equal(a[0], b)


def _raw(h, fn="colnde_ensemble_fc_embedded", Nz=32, n=4, Kk=K, Lz=LZ, dt=DT, K_ca=1.0, w=True, dz=True, To=True, faces=True, shift=0):
    """The C ABI straight through ctypes: the refusals of the library, not of the Python wrapper."""
    import torch
    dev = fn.endswith("_dev")
    z = (lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")) if dev else (lambda *s: np.zeros(s, np.float32))
    m = max(n, 1)
    bufs = dict(w=z(Kk * 200000), T=z(Kk * m * Nz + 4), top=z(m), dz=z(Kk * m * Nz), To=z(Kk * m * Nz), faces=z(Kk * m * (Nz + 1)))
    P = (lambda a, o=0: ctypes.c_void_p(a.data_ptr() + 4 * o)) if dev else (lambda a, o=0: ctypes.c_void_p(a.ctypes.data + 4 * o))
    rc = getattr(h._L, fn)(h._h, P(bufs["w"]) if w else None, P(bufs["T"], shift), P(bufs["top"]), None, None, ctypes.c_float(Lz), ctypes.c_float(dt),
                           ctypes.c_float(K_ca), P(bufs["dz"]) if dz else None, P(bufs["To"]) if To else None, P(bufs["faces"]) if faces else None, n)
    return rc, h._L.colnde_last_error().decode()


def test_refusals_name_the_function_and_leave_the_handle_working():
    import colnde
    from colnde import synthetic
    sc = (1.0,) * 6

    def refused(h, match, **kw):
        for fn in ("colnde_ensemble_fc_embedded", "colnde_ensemble_fc_embedded_dev"):
            if "shift" in kw and not fn.endswith("_dev"):
                continue                                                         # host arrays carry no alignment rule
            rc, msg = _raw(h, fn, **kw)
            assert rc != 0 and fn in msg and match in msg, (fn, msg)

    wm = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1.0)
    with colnde.ColumnNDE(wm.cfg, 8) as nde:
        refused(nde, "needs free-convection networks", Kk=1)
    with colnde.ColumnNDEEnsemble(wm.cfg, 8, 2) as e:
        refused(e, "needs free-convection networks", Kk=2)
    with colnde.ClosureColumns(wm.cfg, 8, 2) as cl:
        refused(cl, "closure handle", Kk=2)
    with colnde.ColumnNDE(synthetic.free_convection_problem(8, Nz=16, n_save=3).cfg, 8) as nde:
        refused(nde, "covers Nz = 32 or 64 (this handle has Nz = 16)", Nz=16, Kk=1)
    with colnde.ColumnNDE(synthetic.free_convection_problem(8, Nz=32, n_save=3, layer_sizes=(32, 64, 64, 31)).cfg, 8) as nde:
        refused(nde, "this handle has Nz = 32 and network 32-64-64-31", Kk=1)
    p = synthetic.free_convection_problem(4, Nz=32, n_save=3, substeps=2, t_end=0.01)
    for c in (0, 3):
        with _ensemble(32, c) as ens:
            ens.set_problem(p.x0, p.bcs, p.x0[:, None, :].repeat(3, axis=1))
            Wc = C.weights(32, c)
            for match, kw in (("weights == NULL", dict(w=False)),                 # the first call on this handle
                              ("one output group", dict(To=False)), ("one output group", dict(dz=False)),
                              ("nothing to compute", dict(dz=False, To=False, faces=False)), ("dt > 0 required", dict(dt=0.0)),
                              ("K_ca >= 0 required", dict(K_ca=-1.0)), ("n_columns >= 1 and Lz > 0", dict(n=0)),
                              ("n_columns >= 1 and Lz > 0", dict(Lz=0.0)), ("16-byte aligned", dict(shift=1))):
                refused(ens, match, **kw)
                loss = ens.loss(Wc, sc)
                assert loss.shape == (K, 8) and np.isfinite(loss).all()          # after every refusal the handle still computes
            rc, msg = _raw(ens, "colnde_ensemble_fc_embedded_dev", dt=0.0, dz=False, To=False)       # without a step dt is not read
            assert rc == 0, msg
            loss = ens.loss(Wc, sc)
            assert np.isfinite(loss).all()
