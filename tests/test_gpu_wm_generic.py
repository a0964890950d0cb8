"""The wind-mixing embedding for networks of any trained architecture on the GPU: `colnde_ensemble_wm_embedded[_dev]` with a single `ColumnNDE`
handle as K = 1 (csrc/engine_wm_embed_any.hip) against the float64 restatements of tests/wm_embed_common.py and tests/wm_diag_restatement.py, the
oracle's modified_pacanowski_philander_step, `colnde_implicit_diffusion_dev` (bit for bit: the same sweep function) and, for the one shape both
serve, the persistent kernel (COLNDE_WM_GENERIC=1).

Shapes, weights, state and bounds: tests/wm_generic_cases.py; every fact stated there is checked by tests/test_wm_generic_host.py.  Errors are
max|gpu − f64| / max|f64| over the columns of the case."""
import ctypes
import functools

import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as O
from tests import wm_embed_common as W
from tests import wm_generic_cases as C
from tests.test_gpu_parity import _record      # COLNDE_RECORD_ERRORS=1: the measured errors join the other parity records

pytestmark = pytest.mark.gpu

DZ, ST, FC = ("dz_uw", "dz_vw", "dz_wT"), ("u_out", "v_out", "T_out"), ("uw", "vw", "wT")
WIDE = "96-400-400-31"
FORCING_CASES = [(name, n) for name in C.SHAPES for n in (1, 17)] + [(WIDE, n) for n in (15, 16, 33, 200)]


@functools.lru_cache(maxsize=None)
def _handle(name, ma="bf16x3_exact"):
    """one handle per shape and arithmetic for the whole module (the handle's own column count is unrelated to the calls')"""
    import colnde
    return colnde.ColumnNDE(C.problem(name).cfg, 4, matrix_arithmetic=ma)


def _cu(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).cuda()      # (a copy: the cases are read-only)


def _call(nde, c, step=False, flux=False, ca=0, hb=None, ht=None, dev=False):
    """`ColumnNDE.wm_embedded` with the single handle as K = 1 -> {name: numpy array without the model axis}; dev: the device twin"""
    one = lambda a: None if a is None else np.ascontiguousarray(a)[None]
    args = [c.w[None], one(c.u), one(c.v), one(c.T), c.top]
    halos = [one(hb), one(ht)]
    if dev:
        import torch
        args, halos = [_cu(a) for a in args], [_cu(a) for a in halos]
    r = nde.wm_embedded(*args, W.LZ, C.DT if step else None, np.float32(W.mpp_params())[None], ca, halos[0], halos[1], step=step, flux=flux)
    if dev:
        torch.cuda.synchronize()
    out = {}
    for names, group in zip((DZ, ST, FC), r):
        for nm, a in zip(names, group or ()):
            out[nm] = (a.cpu().numpy() if dev else a)[0]
    return out


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for nm in a:
        assert np.isfinite(a[nm]).all() and np.array_equal(a[nm], b[nm]), (what, nm)


@pytest.mark.parametrize("name,n", FORCING_CASES)
def test_forcing(name, n):
    """One pipe is built (colnde_describe: wm_embed=generic_f32), so both matrix arithmetics of the handle must give the same bits."""
    c = C.case(name, n)
    ref = tuple(r[:n] for r in C.dz_ref(name))
    outs = []
    for ma in ("bf16x3_exact", "f32_mfma"):
        nde = _handle(name, ma)
        d = nde.describe()
        assert "wm_embed=generic_f32" in d and "wm_infer" not in d
        host = _call(nde, c)
        _same(host, _call(nde, c, dev=True), "host and device twins")
        _same(host, _call(nde, c), "two launches")
        outs.append(host)
    _same(outs[0], outs[1], "both matrix arithmetics")
    got = outs[0]
    assert set(got) == set(DZ)
    errs = C.rel_dist([got[k] for k in DZ], ref)
    print("wm_generic forcing %s n=%d: rel err uw %.3e vw %.3e wT %.3e" % ((name, n) + tuple(errs)))
    _record("wm_generic/forcing/%s/%d" % (name, n), **dict(zip(C.NETS, errs)))
    for nm, e in zip(C.NETS, errs):
        assert e <= C.DZ_BOUND[nm], (nm, e)
    assert np.array_equal(got["dz_wT"][:, 0], np.zeros(n, np.float32))                                # first interior wT face is exactly 0


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("name", [WIDE, "96-7-31"])
def test_step(name, n, ca, halo):
    import torch
    c = C.case(name, n)
    ref = tuple(r[:n] for r in C.dz_ref(name))
    hb = C.step_halo(c.u, c.v, c.T) if halo else None
    want = O.modified_pacanowski_philander_step(c.u, c.v, c.T, C.DT, W.LZ / 32, convective_adjustment=bool(ca), halo_bottom=hb, **W.MPP)
    nde = _handle(name)
    alone = _call(nde, c)
    host = _call(nde, c, step=True, ca=ca, hb=hb)
    assert set(host) == set(DZ + ST)
    # out of place on the device: the inputs survive
    wd, ud, vd, Td, td, hd = (_cu(a) for a in (c.w[None], c.u[None], c.v[None], c.T[None], c.top, None if hb is None else hb[None]))
    r = nde.wm_embedded(wd, ud, vd, Td, td, W.LZ, C.DT, np.float32(W.mpp_params())[None], ca, hd, None, step=True, flux=False)
    torch.cuda.synchronize()
    assert all(np.array_equal(x.cpu().numpy()[0], y) for x, y in zip((ud, vd, Td), (c.u, c.v, c.T)))          # inputs untouched
    _same(host, {nm: a.cpu().numpy()[0] for nm, a in zip(DZ + ST, r.dz + r.state)}, "out of place, device twin")
    # ... and the same kernel that colnde_implicit_diffusion_dev launches the sweep function of: equal bits (the step does not see the nets)
    diff = nde.implicit_diffusion(ud[0], vd[0], Td[0], C.DT, W.LZ / 32, W.mpp_params(), bool(ca), None if hd is None else hd[0])
    torch.cuda.synchronize()
    for nm, a in zip(ST, diff):
        assert np.array_equal(host[nm], a.cpu().numpy()), nm
    # in place through the C ABI: u_out aliasing u (the wrapper returns fresh tensors)
    dz = [torch.empty_like(ud) for _ in range(3)]
    pr = (ctypes.c_float * 7)(*W.mpp_params())
    D = lambda t: None if t is None else t.data_ptr()
    rc = nde._L.colnde_ensemble_wm_embedded_dev(nde._h, D(wd), D(ud), D(vd), D(Td), D(td), D(hd), None, W.LZ, C.DT, pr, ca, D(dz[0]), D(dz[1]), D(dz[2]),
                                                D(ud), D(vd), D(Td), None, None, None, n)
    assert rc == 0, nde._L.colnde_last_error().decode()
    torch.cuda.synchronize()
    _same(host, {nm: a.cpu().numpy()[0] for nm, a in zip(DZ + ST, dz + [ud, vd, Td])}, "in place")
    # the ∂z arrays are those of the state as given — the no-step call's bits — and not the networks on the diffused state
    post = _call(nde, C.SimpleNamespace(w=c.w, u=host["u_out"], v=host["v_out"], T=host["T_out"], top=c.top))
    for nm in DZ:
        assert np.array_equal(host[nm], alone[nm]), nm
    assert any(not np.array_equal(host[nm], post[nm]) for nm in DZ)
    errs = C.rel_dist([host[k] for k in DZ], ref)
    st_errs = C.rel_dist([host[k] for k in ST], want)
    print("wm_generic step %s n=%d ca=%d halo=%d: dz %.3e %.3e %.3e, state %.3e %.3e %.3e" % ((name, n, ca, halo) + tuple(errs) + tuple(st_errs)))
    _record("wm_generic/step/%s/%d/%d/%d" % (name, n, ca, halo), **dict(zip(C.NETS, errs)), **dict(zip(ST, st_errs)))
    for nm, e in zip(C.NETS, errs):
        assert e <= C.DZ_BOUND[nm], (nm, e)
    for nm, e, tol in zip(ST, st_errs, C.STEP_BOUND):
        assert e <= tol, (nm, e)
    assert np.array_equal(host["T_out"][:, 0], c.T[:, 0])                                             # T′[1] = T_bottom, bit for bit


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [0, 1])
@pytest.mark.parametrize("name", [WIDE, "96-7-31", "96-50-20-13-31"])
def test_face_diagnosis(name, ca, halo):
    n = 33
    c = C.diag_case(name, n)
    hb, ht = (c.hb, c.ht) if halo else (None, None)
    ref = tuple(r[:n] for r in C.face_ref(name, ca, halo))
    dz_ref = tuple(r[:n] for r in C.dz_ref_diag_state(name))
    nde = _handle(name)
    faces = _call(nde, c, flux=True, ca=ca, hb=hb, ht=ht)
    step = _call(nde, c, step=True, ca=ca, hb=hb)
    both = _call(nde, c, step=True, flux=True, ca=ca, hb=hb, ht=ht)
    assert set(both) == set(DZ + ST + FC) and set(faces) == set(DZ + FC)
    _same(both, {**step, **{k: faces[k] for k in FC}}, "step and flux in one call, and the two separate calls")
    _same({k: faces[k] for k in DZ}, {k: step[k] for k in DZ}, "the ∂z arrays of the two calls")
    _same(both, _call(nde, c, step=True, flux=True, ca=ca, hb=hb, ht=ht, dev=True), "host and device twins")
    errs = C.rel_dist([faces[k] for k in FC], ref)
    dz_errs = C.rel_dist([faces[k] for k in DZ], dz_ref)
    print("wm_generic faces %s ca=%d halo=%d: uw %.3e vw %.3e wT %.3e (dz %.3e %.3e %.3e)" % ((name, ca, halo) + tuple(errs) + tuple(dz_errs)))
    _record("wm_generic/faces/%s/%d/%d" % (name, ca, halo), **dict(zip(C.NETS, errs)))
    for nm, e in zip(C.NETS, errs):
        assert e <= C.FACE_BOUND[(ca, nm)], (nm, e)
    for nm, e in zip(C.NETS, dz_errs):
        assert e <= C.DZ_BOUND[nm], (nm, e)
    # ν = 0 on both end faces: the top face of uw, vw is the top flux itself, the bottom face 0; νT there is 1 only under convective adjustment with halos
    assert np.array_equal(faces["uw"][:, 32], c.top[0]) and np.array_equal(faces["vw"][:, 32], c.top[1])
    assert not faces["uw"][:, 0].any() and not faces["vw"][:, 0].any()
    if not (ca and halo):
        assert np.array_equal(faces["wT"][:, 32], c.top[2]) and not faces["wT"][:, 0].any()


@pytest.mark.parametrize("n", [1, 33, 77])
def test_kernel_against_kernel(n, monkeypatch):
    """The one shape both kernels serve: every output of the generic kernel is within 2 x the bound of the persistent kernel's — both are float32
    with different sum orders.  The switch is read per call."""
    monkeypatch.delenv("COLNDE_WM_GENERIC", raising=False)
    c = C.diag_case(C.FIXED, n)
    nde = _handle(C.FIXED)
    assert "wm_embed" not in nde.describe() and "wm_infer=f32" in nde.describe()
    single = nde.wm_infer_dz_flux(c.w, c.u, c.v, c.T, c.top, W.LZ)
    for ca in (0, 1):
        persistent = _call(nde, c, step=True, flux=True, ca=ca, hb=c.hb, ht=c.ht)
        monkeypatch.setenv("COLNDE_WM_GENERIC", "1")
        assert "wm_embed=generic_f32" in nde.describe() and "COLNDE_WM_GENERIC=1" in nde.describe()
        generic = _call(nde, c, step=True, flux=True, ca=ca, hb=c.hb, ht=c.ht)
        monkeypatch.delenv("COLNDE_WM_GENERIC")
        bounds = dict(zip(DZ, (C.DZ_BOUND[k] for k in C.NETS)), **dict(zip(ST, C.STEP_BOUND)), **dict(zip(FC, (C.FACE_BOUND[(ca, k)] for k in C.NETS))))
        errs = dict(zip(DZ + ST + FC, C.rel_dist([generic[k] for k in DZ + ST + FC], [persistent[k].astype(np.float64) for k in DZ + ST + FC])))
        print("wm_generic against persistent n=%d ca=%d: %s" % (n, ca, " ".join("%s %.2e" % kv for kv in errs.items())))
        _record("wm_generic/against_persistent/%d/%d" % (n, ca), **errs)
        assert any(not np.array_equal(generic[k], persistent[k]) for k in DZ)                        # (the switch did change the kernel)
        for nm, e in errs.items():
            assert e <= 2 * bounds[nm], (nm, e)
        _same(persistent, _call(nde, c, step=True, flux=True, ca=ca, hb=c.hb, ht=c.ht), "without the switch again")
    # without the switch the single-model entry point's bits are what they were: the persistent kernels'
    _same(dict(zip(DZ, single)), dict(zip(DZ, nde.wm_infer_dz_flux(c.w, c.u, c.v, c.T, c.top, W.LZ))), "wm_infer_dz_flux")
    _same(dict(zip(DZ, single)), _call(nde, c), "the unified call on the fixed shape")


def test_python_mirrors():
    from colnde import wind_mixing as WM
    name, n = "96-400-31", 33
    c = C.diag_case(name, n)
    nde = _handle(name)
    pj = {"ν₀": W.MPP["nu0"], "ν₋": W.MPP["nu_minus"], "ΔRi": W.MPP["dRi"], "Riᶜ": W.MPP["Ric"], "Pr": W.MPP["Pr"]}
    cj = {"α": W.MPP["alpha"], "g": W.MPP["g"]}
    both = _call(nde, c, step=True, flux=True, ca=1, hb=c.hb, ht=c.ht)
    f = WM.NN_forcings(nde, c.w, c.u, c.v, c.T, c.top, W.LZ)
    f3 = WM.NN_forcings(nde, c.w, c.u[3], c.v[3], c.T[3], c.top[:, 3], W.LZ)
    for k, nm in enumerate(DZ):
        assert np.array_equal(f[k], -both[nm]) and f3[k].shape == (32,) and np.array_equal(f3[k], -both[nm][3])
    dz, st = WM.progress_neural_network(nde, c.w, c.u, c.v, c.T, c.top, W.LZ, C.DT, pj, cj, True, c.hb)
    _same(dict(zip(DZ + ST, dz + st)), {k: both[k] for k in DZ + ST}, "progress_neural_network")
    faces = WM.diagnose_NN_flux(nde, c.w, c.u, c.v, c.T, c.top, W.LZ, pj, cj, True, (c.hb, c.ht))
    _same(dict(zip(FC, faces)), {k: both[k] for k in FC}, "diagnose_NN_flux")
    one = WM.diagnose_NN_flux(nde, c.w, c.u[5], c.v[5], c.T[5], c.top[:, 5], W.LZ, pj, cj, True, (c.hb[:, 5], c.ht[:, 5]))
    assert all(a.shape == (33,) and np.array_equal(a, both[nm][5]) for a, nm in zip(one, FC))


def _raw(nde, n=4, drop=(), host=True, misalign=False, n_params=None):
    """colnde_ensemble_wm_embedded[_dev] straight through ctypes with K = 1 (the refusals of the C ABI, not of the wrapper) -> (rc, message)"""
    L, m = nde._L, max(n, 1)
    P_ = n_params if n_params is not None else max(int(L.colnde_n_params(nde._h)), 1)
    pr = (ctypes.c_float * 7)(*W.mpp_params())
    if host:
        z = lambda *s: np.zeros(s, np.float32)
        keep = [z(P_), z(m, 32), z(3, m)] + [z(m, 32) for _ in range(6)] + [z(m, 33) for _ in range(3)]
        P = [a.ctypes.data_as(ctypes.c_void_p) for a in keep]
        fn = L.colnde_ensemble_wm_embedded
    else:
        import torch
        keep = [torch.zeros(P_, device="cuda"), torch.zeros(m * 32, device="cuda"), torch.zeros(3 * m + 4, device="cuda")] + \
               [torch.zeros(m * 32, device="cuda") for _ in range(6)] + [torch.zeros(m * 33 + 4, device="cuda") for _ in range(3)]
        P = [t.data_ptr() for t in keep]
        if misalign:
            P[10] += 4                                                             # vw: one float past a 16-byte boundary
        fn = L.colnde_ensemble_wm_embedded_dev
    names = DZ + ST + FC
    outs = {nm: ptr for nm, ptr in zip(names, P[3:])}
    for nm in drop:
        outs[nm] = None
    rc = fn(nde._h, P[0], P[1], P[1], P[1], P[2], None, None, ctypes.c_float(W.LZ), ctypes.c_float(C.DT), pr, 0, *[outs[nm] for nm in names], n)
    return rc, L.colnde_last_error().decode()


def test_refusals_name_the_reason():
    import colnde
    wide = C.problem(WIDE)

    def refused(nde, match, **kw):
        for host in ((False,) if kw.get("misalign") else (True, False)):
            rc, msg = _raw(nde, host=host, **kw)
            assert rc != 0 and match in msg and "colnde_ensemble_wm_embedded" in msg, (host, msg)

    with pytest.raises(colnde.ColndeError, match="96-50-20-31"):                   # a K = 2 ensemble cannot be created wide (unchanged)
        colnde.ColumnNDEEnsemble(wide.cfg, 8, 2)
    with colnde.ColumnNDE(wide.cfg.with_(smooth_NN=True), 8) as nde:
        refused(nde, "no smoothing filter")
        assert "wm_embed" not in nde.describe()
    fc = synthetic.free_convection_problem(8, Nz=32, n_save=3)
    with colnde.ColumnNDE(fc.cfg, 8) as nde:
        refused(nde, "needs a wind-mixing handle")
    sizes, acts = C.TOO_WIDE
    huge = synthetic.wind_mixing_problem(8, n_frames=3, layer_sizes=sizes, activations=acts)
    with colnde.ColumnNDE(huge.cfg, 8) as nde:
        refused(nde, "%d bytes of LDS" % C.lds_plan_bytes(sizes), n_params=4)      # refused before any array is touched
        assert "96-2048-2048-31" in nde._L.colnde_last_error().decode() and "wm_embed" not in nde.describe() and "wm_infer" not in nde.describe()
    nde = _handle(WIDE)
    refused(nde, "one output group", drop=("v_out",))
    refused(nde, "one output group", drop=("uw", "wT"))
    refused(nde, "16-byte aligned", misalign=True)
    for host in (True, False):
        rc, msg = _raw(nde, n=0, host=host)
        assert rc != 0 and "n_columns >= 1 and Lz > 0" in msg
        rc, msg = _raw(nde, host=host)
        assert rc == 0, msg
    # the four older entry points still refuse other layer sizes, and now name the unified call
    z = lambda *s: np.zeros(s, np.float32)
    w, u, top, o, f = z(nde.n_params), z(4, 32), z(3, 4), [z(4, 32) for _ in range(6)], [z(4, 33) for _ in range(3)]
    pr = (ctypes.c_float * 7)(*W.mpp_params())
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L = nde._L
    calls = [lambda: L.colnde_wm_infer_dz_flux(nde._h, P(w), P(u), P(u), P(u), P(top), ctypes.c_float(W.LZ), P(o[0]), P(o[1]), P(o[2]), 4),
             lambda: L.colnde_wm_embedded_step(nde._h, P(w), P(u), P(u), P(u), P(top), None, ctypes.c_float(W.LZ), ctypes.c_float(C.DT), pr, 0, P(o[0]), P(o[1]),
                                               P(o[2]), P(o[3]), P(o[4]), P(o[5]), 4),
             lambda: L.colnde_wm_diagnose_flux(nde._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(W.LZ), pr, 0, P(f[0]), P(f[1]), P(f[2]), 4),
             lambda: L.colnde_wm_embedded_step_flux(nde._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(W.LZ), ctypes.c_float(C.DT), pr, 0, P(o[0]),
                                                    P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(f[0]), P(f[1]), P(f[2]), 4)]
    for call in calls:
        assert call() != 0
        msg = L.colnde_last_error().decode()
        assert "three 96-50-20-31 networks" in msg and "96-400-400-31" in msg and "colnde_ensemble_wm_embedded deploys a single handle" in msg, msg
