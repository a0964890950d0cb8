"""CPU-side checks of `colnde_ensemble_profile`: the symbols against the header, the binding and the Julia wrapper; the null-handle refusal; the
wrapper's shape rules; and `wind_mixing._assemble_NDE_profile` — everything `NDE_profile` does after the device call (training_postprocessing.jl:392-599)
— held to the float64 restatement (tests/wm_profile_restatement.py) on random arrays, with and without the closure.

Tolerance of the assembly: it works in Float32 as the reference does; one unscaling σ x + μ and one subtraction or a sum of three products are a few
roundings each, so every key is held to 4e-6 of its own scale (atol, relative to max|key|: T ~ 19.5 unscaled carries ulp(19.5) ≈ 2e-6 of absolute
error against profile differences of O(1e-2)...O(1)) plus 4e-6 |value| (rtol) — about 30 float32 ulps, nothing measured on the code under test."""
import ctypes
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic, wind_mixing
from colnde.nde import check_wm_profile_arrays
from tests import wm_profile_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("colnde_ensemble_profile", "colnde_ensemble_profile_dev")
RTOL = ATOL = 4e-6


def test_symbols_declared_exported_bound_and_wrapped():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    assert re.search(r"#define\s+COLNDE_VERSION\s+106\b", text)                               # additive: the version stays
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.lib()
    assert L.colnde_version() == 106
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 9 == len(bound[name]), (name, len(args), len(bound[name]))
        assert all(t is ctypes.c_void_p for t in bound[name]) and all("*" in a for a in args), name   # nine pointers, no scalar
        assert hasattr(L, name), "%s declared in colnde.h but not exported" % name
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    m = re.search(r"ccall\(\(:colnde_ensemble_profile, libcolnde\), Cint,\s*\(([^)]*)\)", jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 9                   # the header's arity
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "colnde_ensemble_profile" in open(os.path.join(ROOT, doc)).read(), doc
    assert colnde.nde.KERNEL_IDS["wm_profile"] == 11


@pytest.mark.parametrize("name", NEW)
def test_null_handle_is_refused(name):
    L = _lib.lib()
    assert getattr(L, name)(None, None, None, None, None, None, None, None, None) != 0
    msg = L.colnde_last_error().decode()
    assert "null handle" in msg and name in msg


def test_wrapper_checks():
    z = lambda *s: np.zeros(s, np.float32)
    K, P, n, ns = 3, 19563, 5, 7
    check_wm_profile_arrays(K, P, n, ns, 32, z(K, P), z(K, n, ns, 96), z(K, 5))
    with pytest.raises(ValueError, match=r"weights: expected shape \(3, 19563\) for 3 models"):
        check_wm_profile_arrays(K, P, n, ns, 32, z(2, P), z(K, n, ns, 96))
    with pytest.raises(ValueError, match=r"sol: expected shape \(3, 5, 7, 96\)"):
        check_wm_profile_arrays(K, P, n, ns, 32, z(K, P), z(K, n, 96))
    with pytest.raises(ValueError, match=r"physics: expected shape \(3, 5\)"):
        check_wm_profile_arrays(K, P, n, ns, 32, z(K, P), z(K, n, ns, 96), z(K, 7))
    with pytest.raises(ValueError, match="no outputs"):
        check_wm_profile_arrays(K, P, n, ns, 32, z(K, P), z(K, n, ns, 96), None, False, False, False)


def _random_arrays(rng, n, ns, Nz=32):
    a = dict(sol=rng.standard_normal((n, ns, 3 * Nz)), losses=rng.uniform(0.0, 2.0, (n, 6, ns)))
    for nm in ("uw", "vw", "wT"):
        a[nm] = rng.standard_normal((n, ns, Nz + 1))
    a["Ri"] = rng.standard_normal((n, ns, Nz + 1)) * 10.0
    a["Ri"][:, :, 0] = a["Ri"][:, :, Nz] = np.nan                                            # the reference's boundary faces
    return {k: v.astype(np.float32) for k, v in a.items()}


@pytest.mark.parametrize("closure", [True, False])
def test_assemble_against_the_restatement(closure):
    kw = {} if closure else dict(modified_pacanowski_philander=False, zero_weights=False)
    cfg = synthetic.wind_mixing_problem(4, n_frames=6, weight_divisor=10, **kw).cfg
    rng = np.random.default_rng(5)
    n, ns = 4, cfg.n_save
    a, a0 = _random_arrays(rng, n, ns), _random_arrays(rng, n, ns)
    nn = tuple(rng.standard_normal((n, ns, 33)).astype(np.float32) for _ in range(3))
    truth = rng.standard_normal((n, ns, 96)).astype(np.float32)
    sc = (1.0, 0.7, 1.3, 5e-3, 4e-3, 6e-3)
    tp = dict(nu0=1e-4, nu_minus=0.1, dRi=1.0, Ric=0.25, Pr=1.0)
    got = wind_mixing._assemble_NDE_profile(cfg, a, truth, sc, a0 if closure else None, nn if closure else None, tp if closure else None)
    ref = R.postprocess(cfg, a, truth, sc, a0, nn, tp)
    worst = R.compare(got, ref, RTOL, ATOL)
    print("worst excess over the bound: %.3g" % worst)
    # the key set, with and without the closure (:534-599 minus the KPP keys)
    base = {"depth_profile", "depth_flux", "t", "truth_u", "truth_v", "truth_T", "truth_uw", "truth_vw", "truth_wT", "truth_Ri", "test_u", "test_v", "test_T",
            "test_uw", "test_vw", "test_wT", "test_Ri", "u_losses", "v_losses", "T_losses", "∂u∂z_losses", "∂v∂z_losses", "∂T∂z_losses", "losses", "loss",
            "losses_gradient", "loss_gradient"}
    M = "_modified_pacanowski_philander"
    extra = {"train_parameters", "test_uw_NN_only", "test_vw_NN_only", "test_wT_NN_only", "test_Ri" + M, "losses" + M, "loss" + M, "losses%s_gradient" % M,
             "loss%s_gradient" % M} | {"test_%s%s" % (q, M) for q in ("u", "v", "T", "uw", "vw", "wT")} | {
                 "%s_losses%s" % (q, M) for q in ("u", "v", "T", "∂u∂z", "∂v∂z", "∂T∂z")}
    assert set(got) == (base | extra if closure else base)
    # test_uw .- test_uw[1, 1]: the bottom face of the first frame of every simulation is exactly zero, and only that subtraction was applied
    for nm in ("uw", "vw", "wT"):
        assert not got["test_" + nm][:, 0, 0].any()
        un = np.float32(cfg.sigma[3 + ("uw", "vw", "wT").index(nm)]) * a[nm] + np.float32(cfg.mu[3 + ("uw", "vw", "wT").index(nm)])
        assert np.array_equal(got["test_" + nm], np.swapaxes(un, 1, 2) - un[:, :1, :1])
    # the sums: losses = u + v + T scaled, loss its mean over time; shapes [n_sim, Nt] and [n_sim]
    assert got["losses"].shape == (n, ns) and got["loss"].shape == (n,)
    assert np.allclose(got["losses"], sc[0] * a["losses"][:, 0] + sc[1] * a["losses"][:, 1] + sc[2] * a["losses"][:, 2], rtol=1e-6)
    assert np.allclose(got["loss_gradient"], got["losses_gradient"].mean(axis=1), rtol=1e-6)
    assert np.isnan(got["truth_Ri"][:, 0]).all() and np.isnan(got["truth_Ri"][:, 32]).all() and np.isfinite(got["truth_Ri"][:, 1:32]).all()


def test_assemble_needs_the_closure_arrays():
    cfg = synthetic.wind_mixing_problem(2, n_frames=3, weight_divisor=10).cfg
    a = _random_arrays(np.random.default_rng(1), 2, 3)
    with pytest.raises(ValueError, match="closure-only arrays"):
        wind_mixing._assemble_NDE_profile(cfg, a, np.zeros((2, 3, 96), np.float32), (1, 1, 1, 1, 1, 1))
