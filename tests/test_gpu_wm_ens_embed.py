"""`colnde_ensemble_wm_embedded`: all K members of an ensemble advanced by one embedded iteration (and / or diagnosed) in ONE launch, each on its own
column state with its own weights and its own Pacanowski-Philander constants.

Inputs: synthetic.wind_mixing_problem(300, n_frames=3, weight_divisor=1.0) through wm_embed_common.embed_inputs and wm_diag_restatement.diag_inputs
(both `Ri > 0` branches occur); model k's state is that state plus the constant offsets (+0.003, −0.002, +0.05)(k + 1) on (u, v, T), so every model's
networks see a different input while the level differences — and with them the branch every face takes — stay those of the base state (the float64
case asserts that float32 and float64 agree on every face); model k's weights are perturb_weights(seed 100 + k) of weights_truth; model k's constants are
wm_embed_common.MPP — the one set tests/test_gpu_wm_diag.py uses — with all five moved by at most a factor 0.6 .. 1.4: nu0 (1 + 0.1 k), nu_minus
(1 − 0.05 k), dRi (1 − 0.1 k), Ric + 0.02 k, Pr (1 + 0.1 k).

The bit-for-bit cases need no tolerance.  The float64 case imports its bounds from the single-model tests (DZ_BOUND of tests/test_gpu_wm_embed.py, NN_BOUND of
tests/test_gpu_wm_diag.py): row k IS the single-model call's bits, and those bounds are 10 x the float32-vs-float64 distance of the restatement."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                   # (the child process of test_several_models_per_workgroup runs this file as a script)
    sys.path.insert(0, ROOT)

from colnde import synthetic
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W

pytestmark = pytest.mark.gpu

N_ALL = 300
DT = 60.0
K_MAX = 5
OUT_NAMES = ("dz_uw", "dz_vw", "dz_wT", "u_out", "v_out", "T_out", "uw", "vw", "wT")
GROUPS = [(True, True), (True, False), (False, True), (False, False)]               # (step, flux): the four instantiations


def model_mpp(k):
    m = dict(W.MPP)
    m.update(nu0=W.MPP["nu0"] * (1 + 0.1 * k), nu_minus=W.MPP["nu_minus"] * (1 - 0.05 * k), dRi=W.MPP["dRi"] * (1 - 0.1 * k), Ric=W.MPP["Ric"] + 0.02 * k,
             Pr=W.MPP["Pr"] * (1 + 0.1 * k))
    return m


def model_params(k):
    m = model_mpp(k)
    return tuple(np.float32(m[key]) for key in ("nu0", "nu_minus", "dRi", "Ric", "Pr", "alpha", "g"))


@functools.lru_cache(maxsize=None)
def _problem():
    p = synthetic.wind_mixing_problem(N_ALL, n_frames=3, weight_divisor=1.0)
    base = R.diag_inputs(W.embed_inputs(p), N_ALL)
    weights = np.stack([synthetic.perturb_weights(np.random.default_rng(100 + k), p.weights_truth, 0.05) for k in range(K_MAX)])
    weights.setflags(write=False)
    for a in base:
        a.setflags(write=False)
    return p, base, weights


def ens_case(K, n):
    """weights [K, P], u, v, T [K, n, 32], top [3, n], halo_bottom, halo_top [K, 3, n], params [K, 7]"""
    p, (u, v, T, top, hb, ht), weights = _problem()
    off = np.array([0.003, -0.002, 0.05])
    st = [np.ascontiguousarray(np.stack([(a[:n].astype(np.float64) + off[f] * (k + 1)).astype(np.float32) for k in range(K)])) for f, a in enumerate((u, v, T))]
    hs = [np.ascontiguousarray(np.stack([np.stack([(hl[f, :n].astype(np.float64) + off[f] * (k + 1)).astype(np.float32) for f in range(3)]) for k in range(K)]))
          for hl in (hb, ht)]
    params = np.array([model_params(k) for k in range(K)], dtype=np.float32)
    return p, np.ascontiguousarray(weights[:K]), st[0], st[1], st[2], np.ascontiguousarray(top[:, :n]), hs[0], hs[1], params


def flat(r):
    """WmEnsembleEmbedded -> {name: array} of the outputs it holds"""
    parts = tuple(r.dz) + (tuple(r.state) if r.state is not None else (None,) * 3) + (tuple(r.faces) if r.faces is not None else (None,) * 3)
    return {nm: a for nm, a in zip(OUT_NAMES, parts) if a is not None}


def single_model(nde, w, u, v, T, top, hb, ht, params, ca, step, flux):
    """The single-model calls the issue names, according to the output groups asked for -> {name: array}"""
    halos = (hb, ht) if hb is not None else None
    pr = tuple(float(x) for x in params)
    if step and flux:
        dz, st, fc = nde.wm_embedded_step_flux(w, u, v, T, top, W.LZ, DT, pr, ca, halos)
    elif step:
        (dz, st), fc = nde.wm_embedded_step(w, u, v, T, top, W.LZ, DT, pr, ca, hb), None
    else:
        dz, st = nde.wm_infer_dz_flux(w, u, v, T, top, W.LZ), None
        fc = nde.wm_diagnose_flux(w, u, v, T, top, W.LZ, pr, ca, halos) if flux else None
    parts = tuple(dz) + (tuple(st) if st is not None else (None,) * 3) + (tuple(fc) if fc is not None else (None,) * 3)
    return {nm: a for nm, a in zip(OUT_NAMES, parts) if a is not None}


def run_ens(ens, case, ca, halo, step, flux, **kw):
    _, w, u, v, T, top, hb, ht, params = case
    return ens.wm_embedded(w, u, v, T, top, W.LZ, DT if step else None, kw.pop("params", params), ca, hb if halo else None, ht if halo else None, step=step,
                           flux=flux, **kw)


def assert_same(a, b, what=""):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for nm in a:
        assert np.isfinite(a[nm]).all(), (what, nm)
        assert np.array_equal(a[nm], b[nm]), (what, nm, float(np.abs(a[nm] - b[nm]).max()))


CASE1 = [(3, 32, s, f, ca, hl) for (s, f) in GROUPS for ca in (0, 1) for hl in (False, True)] + \
        [(K, n, True, True, 1, True) for (K, n) in ((1, 33), (2, 1), (2, 300), (5, 129))]


@pytest.mark.parametrize("K,n,step,flux,ca,halo", CASE1)
def test_row_k_is_the_single_model_call_bit_for_bit(K, n, step, flux, ca, halo):
    import colnde
    case = ens_case(K, n)
    p, w, u, v, T, top, hb, ht, params = case
    with colnde.ColumnNDEEnsemble(p.cfg, 8, K) as ens:                               # the handle's own column count is unrelated to n
        got = flat(run_ens(ens, case, ca, halo, step, flux))
    assert set(got) == set(OUT_NAMES[:3] + (OUT_NAMES[3:6] if step else ()) + (OUT_NAMES[6:] if flux else ()))
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        for k in range(K):
            want = single_model(nde, w[k], u[k], v[k], T[k], top, hb[k] if halo else None, ht[k] if halo else None, params[k], ca, step, flux)
            assert_same({nm: a[k] for nm, a in got.items()}, want, "model %d" % k)
    assert got["dz_uw"].shape == (K, n, 32) and (not flux or got["uw"].shape == (K, n, 33))


def _child_outputs(path):
    """K = 5, n_col in {1, 129}, all output groups, halos, convective adjustment: every output into one .npz (run in a fresh process)"""
    import colnde
    out = {}
    for n in (1, 129):
        case = ens_case(5, n)
        with colnde.ColumnNDEEnsemble(case[0].cfg, 8, 5) as ens:
            for nm, a in flat(run_ens(ens, case, 1, True, True, True)).items():
                out["%d/%s" % (n, nm)] = a
    np.savez(path, **out)


def test_several_models_per_workgroup(tmp_path):
    """COLNDE_WM_ENS_GRID=2 and =1 in a fresh child process: the workgroups walk several models and re-copy the weight image; same bits as unconstrained."""
    res = []
    for grid in (None, "2", "1"):
        env = dict(os.environ)
        env.pop("COLNDE_WM_ENS_GRID", None)
        if grid is not None:
            env["COLNDE_WM_ENS_GRID"] = grid
        path = str(tmp_path / ("out_%s.npz" % grid))
        r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), path], env=env, capture_output=True,
                           text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(dict(np.load(path)))
    assert len(res[0]) == 18
    for other in res[1:]:
        assert_same(res[0], other)
    # ... and the unconstrained child's bits are those of the single-model call, for the model that sits in the middle of a walk
    import colnde
    case = ens_case(5, 129)
    p, w, u, v, T, top, hb, ht, params = case
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        want = single_model(nde, w[3], u[3], v[3], T[3], top, hb[3], ht[3], params[3], 1, True, True)
    for other in res:
        assert_same({nm: other["129/" + nm][3] for nm in OUT_NAMES}, want)


def test_against_float64():
    import colnde
    from tests.test_gpu_parity import _record
    from tests.test_gpu_wm_diag import FIELDS, NN_BOUND
    from tests.test_gpu_wm_embed import DZ_BOUND
    K, n = 3, 77
    case = ens_case(K, n)
    p, w, u, v, T, top, hb, ht, params = case
    for ca in (0, 1):
        with colnde.ColumnNDEEnsemble(p.cfg, 8, K) as ens:
            got = run_ens(ens, case, ca, True, False, True)
        for k in range(K):
            mpp = {key: float(x) for key, x in zip(("nu0", "nu_minus", "dRi", "Ric", "Pr", "alpha", "g"), params[k])}
            halos = (hb[k], ht[k])
            Ri32 = R.richardson_number(u[k], v[k], T[k], np.float32(W.LZ / 32), mpp, halos, np.float32)
            Ri64 = R.richardson_number(u[k], v[k], T[k], W.LZ / 32, mpp, halos, np.float64)
            assert np.array_equal(Ri32 > 0, Ri64 > 0)                              # the precondition of the bounds: the same branch on every face
            interior = (Ri64 > 0)[:, 1:32]
            assert interior.any() and (~interior).any()                            # both branches, for every model
            ref_dz = W.dz_fluxes(p.cfg, w[k], u[k], v[k], T[k], top, W.LZ)
            ref_fc = R.diagnose_NN_flux(p.cfg, w[k], u[k], v[k], T[k], top, W.LZ, mpp, bool(ca), halos)
            e_dz = [float(np.abs(g[k].astype(np.float64) - r).max() / np.abs(r).max()) for g, r in zip(got.dz, ref_dz)]
            e_fc = [float(np.abs(g[k].astype(np.float64) - r).max() / np.abs(r).max()) for g, r in zip(got.faces, ref_fc)]
            print("ensemble_wm_embedded model %d ca=%d: rel err dz %.3e %.3e %.3e   faces %.3e %.3e %.3e" % ((k, ca) + tuple(e_dz) + tuple(e_fc)))
            _record("ensemble_wm_embedded/%d/%d" % (k, ca), **dict(zip(("dz_uw", "dz_vw", "dz_wT") + tuple(FIELDS), e_dz + e_fc)))
            for e in e_dz:
                assert e <= DZ_BOUND, (k, ca, e_dz)
            for nm, e, b in zip(FIELDS, e_fc, NN_BOUND[ca]):
                assert e <= b, (k, ca, nm, e, b)


def test_twins_aliasing_and_the_handles_own_physics():
    import torch
    import colnde
    K, n = 3, 77
    case = ens_case(K, n)
    p, w, u, v, T, top, hb, ht, params = case
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    physics = np.ascontiguousarray(params[:, :5])
    own = np.concatenate([physics, np.tile(np.float32([p.cfg.alpha, p.cfg.g]), (K, 1))], axis=1)
    with colnde.ColumnNDEEnsemble(p.cfg, 8, K, physics=physics) as ens:
        host = flat(run_ens(ens, case, 1, True, True, True))
        dcase = (p,) + tuple(cu(a) for a in case[1:8]) + (params,)
        dev = run_ens(ens, dcase, 1, True, True, True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, cu(b)) for a, b in zip(dcase[2:5], (u, v, T)))                        # inputs untouched
        assert_same(host, {nm: a.cpu().numpy() for nm, a in flat(dev).items()}, "host and device twins")
        # in place through the C ABI: u_out aliasing u (the wrapper returns fresh tensors)
        ud, vd, Td = dcase[2].clone(), dcase[3].clone(), dcase[4].clone()
        dz = [torch.empty_like(ud) for _ in range(3)]
        fc = [torch.empty((K, n, 33), device="cuda") for _ in range(3)]
        pr = (ctypes.c_float * (7 * K))(*[float(x) for x in params.reshape(-1)])
        D = lambda t: t.data_ptr()
        rc = ens._L.colnde_ensemble_wm_embedded_dev(ens._h, D(dcase[1]), D(ud), D(vd), D(Td), D(dcase[5]), D(dcase[6]), D(dcase[7]), W.LZ, DT, pr, 1, D(dz[0]),
                                                    D(dz[1]), D(dz[2]), D(ud), D(vd), D(Td), D(fc[0]), D(fc[1]), D(fc[2]), n)
        assert rc == 0, ens._L.colnde_last_error().decode()
        torch.cuda.synchronize()
        assert_same(host, {nm: a.cpu().numpy() for nm, a in zip(OUT_NAMES, dz + [ud, vd, Td] + fc)}, "in place")
        # params = None: the handle's physics followed by cfg.alpha, cfg.g
        explicit = flat(run_ens(ens, case, 1, True, True, True, params=own))
        assert_same(flat(run_ens(ens, case, 1, True, True, True, params=None)), explicit, "params=None")
        # ... and after set_physics the new constants
        physics2 = np.ascontiguousarray(physics[::-1])
        ens.set_physics(physics2)
        own2 = np.concatenate([physics2, own[:, 5:]], axis=1)
        after = flat(run_ens(ens, case, 1, True, True, True, params=None))
        assert_same(after, flat(run_ens(ens, case, 1, True, True, True, params=own2)), "after set_physics")
        assert not np.array_equal(after["u_out"][0], explicit["u_out"][0]) and np.array_equal(after["u_out"][1], explicit["u_out"][1])


def test_models_are_independent():
    import colnde
    K, n = 3, 77
    case = ens_case(K, n)
    p, w, u, v, T, top, hb, ht, params = case
    with colnde.ColumnNDEEnsemble(p.cfg, 8, K) as ens:
        base = flat(run_ens(ens, case, 1, True, True, True))
        w2, u2, v2, T2, params2 = (a.copy() for a in (w, u, v, T, params))
        w2[1] = synthetic.perturb_weights(np.random.default_rng(7), w[1], 0.05)
        changed = {"weights": (p, w2, u, v, T, top, hb, ht, params),
                   "state": (p, w, u2, v2, T2, top, hb, ht, params),
                   "constants": (p, w, u, v, T, top, hb, ht, params2)}
        u2[1] += np.float32(0.01); v2[1] -= np.float32(0.01); T2[1] *= np.float32(1.001)
        params2[1, :5] *= np.float32(1.25)
        for what, c in changed.items():
            got = flat(run_ens(ens, c, 1, True, True, True))
            for nm in OUT_NAMES:
                assert np.array_equal(got[nm][0], base[nm][0]) and np.array_equal(got[nm][2], base[nm][2]), (what, nm)
            moved = [nm for nm in OUT_NAMES if not np.array_equal(got[nm][1], base[nm][1])]
            assert moved, what                                                     # (the change did reach model 1)


def _raw(h, L, K=2, n=4, Lz=W.LZ, dt=DT, drop=(), host=True, misalign=False):
    """colnde_ensemble_wm_embedded[_dev] straight through ctypes (the refusals of the C ABI, not of the wrapper) -> (rc, message)"""
    m = max(n, 1)
    pr = (ctypes.c_float * (7 * K))(*(list(W.mpp_params()) * K))
    if host:
        z = lambda *s: np.zeros(s, np.float32)
        keep = [z(K, 20000), z(K, m, 32), z(3, m)] + [z(K, m, 32) for _ in range(6)] + [z(K, m, 33) for _ in range(3)]
        P = [a.ctypes.data_as(ctypes.c_void_p) for a in keep]
        fn = L.colnde_ensemble_wm_embedded
    else:
        import torch
        keep = [torch.zeros(K * 20000, device="cuda"), torch.zeros(K * m * 32, device="cuda"), torch.zeros(3 * m + 4, device="cuda")] + \
               [torch.zeros(K * m * 32, device="cuda") for _ in range(6)] + [torch.zeros(K * m * 33 + 4, device="cuda") for _ in range(3)]
        P = [t.data_ptr() for t in keep]
        if misalign:
            P[10] += 4                                                             # vw: one float past a 16-byte boundary
        fn = L.colnde_ensemble_wm_embedded_dev
    outs = {nm: ptr for nm, ptr in zip(OUT_NAMES, P[3:])}
    for nm in drop:
        outs[nm] = None
    rc = fn(h, P[0], P[1], P[1], P[1], P[2], None, None, ctypes.c_float(Lz), ctypes.c_float(dt), pr, 0, *[outs[nm] for nm in OUT_NAMES], n)
    return rc, L.colnde_last_error().decode()


def test_refusals_name_the_reason():
    import colnde
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1.0)

    def refused(nde, match, **kw):
        for host in ((False,) if kw.get("misalign") else (True, False)):
            rc, msg = _raw(nde._h, nde._L, K=nde._L.colnde_n_models(nde._h), host=host, **kw)
            assert rc != 0 and match in msg and "colnde_ensemble_wm_embedded" in msg, (host, msg)

    with colnde.ClosureColumns(p.cfg, 8, 2) as cl:
        refused(cl, "closure handle")
    fc = synthetic.free_convection_problem(8, Nz=32, n_save=3)
    with colnde.ColumnNDE(fc.cfg, 8) as nde:
        refused(nde, "needs a wind-mixing handle")
    with colnde.ColumnNDE(p.cfg.with_(smooth_NN=True), 8) as nde:
        refused(nde, "no smoothing filter")
    with colnde.ColumnNDEEnsemble(p.cfg, 8, 2) as ens:
        refused(ens, "one output group", drop=("v_out",))
        refused(ens, "one output group", drop=("uw", "wT"))
        refused(ens, "dt > 0 required", dt=0.0)
        refused(ens, "dt > 0 required", dt=-1.0)
        refused(ens, "16-byte aligned", misalign=True)
        for host in (True, False):
            rc, msg = _raw(ens._h, ens._L, n=0, host=host)
            assert rc != 0 and "n_columns >= 1 and Lz > 0" in msg
            rc, msg = _raw(ens._h, ens._L, dt=0.0, drop=("u_out", "v_out", "T_out"), host=host)     # no step: dt is ignored
            assert rc == 0, msg
        # the single-model calls still refuse the ensemble handle
        z = lambda *s: np.zeros(s, np.float32)
        w, u, top, o, f = z(20000), z(4, 32), z(3, 4), [z(4, 32) for _ in range(6)], [z(4, 33) for _ in range(3)]
        pr = (ctypes.c_float * 7)(*W.mpp_params())
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        L = ens._L
        calls = [lambda: L.colnde_wm_infer_dz_flux(ens._h, P(w), P(u), P(u), P(u), P(top), ctypes.c_float(W.LZ), P(o[0]), P(o[1]), P(o[2]), 4),
                 lambda: L.colnde_wm_embedded_step(ens._h, P(w), P(u), P(u), P(u), P(top), None, ctypes.c_float(W.LZ), ctypes.c_float(DT), pr, 0, P(o[0]), P(o[1]),
                                                   P(o[2]), P(o[3]), P(o[4]), P(o[5]), 4),
                 lambda: L.colnde_wm_diagnose_flux(ens._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(W.LZ), pr, 0, P(f[0]), P(f[1]), P(f[2]), 4),
                 lambda: L.colnde_wm_embedded_step_flux(ens._h, P(w), P(u), P(u), P(u), P(top), None, None, ctypes.c_float(W.LZ), ctypes.c_float(DT), pr, 0, P(o[0]),
                                                        P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]), P(f[0]), P(f[1]), P(f[2]), 4)]
        for call in calls:
            assert call() != 0 and "holds an ensemble of 2 models" in L.colnde_last_error().decode()
    # a single-model handle is K = 1
    with colnde.ColumnNDE(p.cfg, 8) as nde:
        rc, msg = _raw(nde._h, nde._L, K=1)
        assert rc == 0, msg


def test_python_mirror_three_iterations():
    import colnde
    from colnde import wind_mixing
    K, n = 3, 5
    case = ens_case(K, n)
    p, w, u, v, T, top, hb, ht, params = case
    keys = ("nu0", "nu_minus", "dRi", "Ric", "Pr")
    ps = [dict(zip(keys, (float(x) for x in params[k, :5]))) for k in range(K)]
    consts = dict(alpha=float(params[0, 5]), g=float(params[0, 6]))
    state = (u, v, T)
    hist = []
    with colnde.ColumnNDEEnsemble(p.cfg, 8, K) as ens:
        for _ in range(3):
            dz, state = wind_mixing.ensemble_progress_neural_network(ens, w, state, top, W.LZ, DT, ps, consts, True, hb)
            hist.append((dz, state))
    with colnde.ColumnNDE(p.cfg, 4) as nde:
        for k in range(K):
            sk = (u[k], v[k], T[k])
            for it in range(3):
                dz, sk = wind_mixing.progress_neural_network(nde, w[k], sk[0], sk[1], sk[2], top, W.LZ, DT, ps[k], consts, True, hb[k])
                for a, b in zip(dz + sk, hist[it][0] + hist[it][1]):
                    assert np.isfinite(a).all() and np.array_equal(a, b[k]), (k, it)


if __name__ == "__main__":
    _child_outputs(sys.argv[1])
