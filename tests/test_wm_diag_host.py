"""CPU checks of the wind-mixing flux diagnoses (wind_mixing/src/NDE_oceananigans.jl:157-191, :226-286): the restatement the GPU tests are held
to (tests/wm_diag_restatement.py) pinned by identities it must satisfy, and the Python argument checks."""
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from oracle import nde_oracle as O
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("colnde_wm_diagnose_flux", "colnde_wm_diagnose_flux_dev", "colnde_wm_embedded_step_flux", "colnde_wm_embedded_step_flux_dev",
       "colnde_mpp_diagnose_flux", "colnde_mpp_diagnose_flux_dev")


def _inputs(n=9):
    p = synthetic.wind_mixing_problem(n, n_frames=3, weight_divisor=1.0)
    return p, R.diag_inputs(W.embed_inputs(p), n)


def test_nn_faces_and_the_forcing_chains_convention():
    """(a) ν₀ = ν₋ = 0, no convective adjustment: the diagnosis is the NN faces [0; σy + μ − μ; top]; the forcing chain's faces (:288-329, the
    running sum of Δz ∂z F) differ from them on the INTERIOR faces by one constant per column: inv(scaling) of the already unscaled first
    element minus inv(scaling)(0), σ(σ y₁ + μ) for uw and vw, and σ y₁ for wT (:318 subtracts the unscaled first element itself)."""
    p, (u, v, T, top, hb, ht) = _inputs()
    mpp0 = dict(W.MPP, nu0=0.0, nu_minus=0.0)
    got = R.diagnose_NN_flux(p.cfg, p.weights_truth, u, v, T, top, W.LZ, mpp0, False, (hb, ht))
    F, ys = R.nn_faces(p.cfg, p.weights_truth, u, v, T, top)
    dzF = W.dz_fluxes(p.cfg, p.weights_truth, u, v, T, top, W.LZ)
    for k in range(3):
        sg, mu = p.cfg.sigma[3 + k], p.cfg.mu[3 + k]
        want = np.concatenate([np.zeros((9, 1)), (sg * ys[k] + mu) - mu, top[k].astype(np.float64)[:, None]], axis=1)
        assert np.array_equal(got[k], F[k]) and np.array_equal(got[k], want)
        chain = np.concatenate([np.zeros((9, 1)), np.cumsum(dzF[k] * (W.LZ / 32), axis=1)], axis=1)          # faces the ∂z arrays integrate to
        const = sg * (sg * ys[k][:, 0] + mu) if k < 2 else sg * ys[k][:, 0]
        scale = np.abs(F[k]).max()
        np.testing.assert_allclose(got[k][:, 1:32] - chain[:, 1:32], np.broadcast_to(const[:, None], (9, 31)), rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(chain[:, 32], top[k], rtol=0, atol=1e-12 * scale)                          # ... and both end at the top flux
        assert np.abs(const).min() > 1e-6 * scale                                                           # (the conventions do differ)


@pytest.mark.parametrize("ca", [False, True])
def test_zero_weights_give_the_baseline_but_for_the_top(ca):
    """(b) y = 0: F = [0; 0; top], so the NN diagnosis is −ν ∂z φ on every face below the top — the baseline.  At the top the baseline is the
    top flux itself; the NN diagnosis is top − ν·g, which is the top flux for uw and vw (ν = 0 there) and, for wT, top − νT g_T with νT = 0
    without convective adjustment and `Ri_top > 0 ? 0 : 1` with it: top − ∂z T where the halo cells make the top face unstable."""
    p, (u, v, T, top, hb, ht) = _inputs()
    w0 = np.zeros_like(p.weights_truth)
    nn = R.diagnose_NN_flux(p.cfg, w0, u, v, T, top, W.LZ, W.MPP, ca, (hb, ht))
    base = R.diagnose_baseline_flux(u, v, T, top, W.LZ / 32, W.MPP, ca, (hb, ht))
    for k in range(3):
        assert np.array_equal(nn[k][:, :-1], base[k][:, :-1])
        assert np.array_equal(base[k][:, -1], top[k].astype(np.float64))
    assert np.array_equal(nn[0][:, -1], top[0]) and np.array_equal(nn[1][:, -1], top[1])
    g_top = (ht[2].astype(np.float64) - T[:, -1]) / (W.LZ / 32)
    Ri_top = R.richardson_number(u, v, T, W.LZ / 32, W.MPP, (hb, ht))[:, -1]
    nuT_top = np.where(Ri_top > 0, 0.0, 1.0) if ca else np.zeros(9)
    assert np.array_equal(nn[2][:, -1], top[2] - nuT_top * g_top)
    if ca:
        assert (nuT_top == 1).any() and (nuT_top == 0).any()
    # no halo cells: the zero-gradient fill, g = 0 at both ends, and the top is the top flux for wT too
    nn0 = R.diagnose_NN_flux(p.cfg, w0, u, v, T, top, W.LZ, W.MPP, ca, None)
    assert np.array_equal(nn0[2][:, -1], top[2]) and np.array_equal(np.abs(nn0[2][:, 0]), np.zeros(9))


@pytest.mark.parametrize("ca", [False, True])
def test_explicit_limit_of_the_implicit_step(ca):
    """(c) (φ′ − φ)/Δt of the oracle's modified_pacanowski_philander_step tends to −∂z of the baseline flux (top flux 0) as Δt -> 0, on the interior
    cells (cell 0 carries `T′[1] = T_bottom` and the halo-less bottom row).  Bound: 1e-3 of the largest tendency; the O(Δt) remainder at the
    smaller Δt is estimated from the two Δt values (its difference between Δt and 2Δt) and must itself be below the bound."""
    p, (u, v, T, top, hb, ht) = _inputs()
    dz = W.LZ / 32
    flux = R.diagnose_baseline_flux(u, v, T, np.zeros_like(top), dz, W.MPP, ca, None)
    want = [-(f[:, 1:] - f[:, :-1]) / dz for f in flux]
    rates = []
    for dt in (2e-3, 1e-3):
        new = O.modified_pacanowski_philander_step(u, v, T, dt, dz, convective_adjustment=ca, **W.MPP)
        rates.append([(a - b.astype(np.float64)) / dt for a, b in zip(new, (u, v, T))])
    for k in range(3):
        scale = np.abs(want[k][:, 1:]).max()
        remainder = np.abs(rates[0][k][:, 1:] - rates[1][k][:, 1:]).max()
        err = np.abs(rates[1][k][:, 1:] - want[k][:, 1:]).max()
        assert remainder <= 1e-3 * scale, (remainder, scale)
        assert err <= 1e-3 * scale, (err, scale)


class _Recorder:
    """Stands in for a ColumnNDE: records what the reference-named mirrors pass on."""
    def wm_diagnose_flux(self, weights, u, v, T, top, Lz, params, ca, halos):
        self.args = (u, v, T, top, params, ca, halos)
        return tuple(np.zeros((T.shape[0], T.shape[1] + 1), np.float32) for _ in range(3))

    def mpp_diagnose_flux(self, u, v, T, top, dz, params, ca, hb):
        self.args = (u, v, T, top, dz, params, ca, hb)
        return tuple(np.zeros((T.shape[0], T.shape[1] + 1), np.float32) for _ in range(3))


def test_mirrors_shape_handling():
    """(d) [Nz] or [n, Nz] (or any leading shape), scalar or per-column top fluxes and halo cells."""
    from colnde import wind_mixing as WM
    pj = {"ν₀": 1e-4, "ν₋": 0.1, "ΔRi": 1.0, "Riᶜ": 0.25, "Pr": 1.0}
    rec = _Recorder()
    one = np.zeros(32, np.float32)
    f = WM.diagnose_NN_flux(rec, None, one, one, one, (1.0, 2.0, 3.0), 256.0, pj, {"α": 2e-4, "g": 9.81}, True, (np.zeros(3), None))
    assert all(a.shape == (33,) for a in f)
    u, v, T, top, params, ca, halos = rec.args
    assert T.shape == (1, 32) and top.shape == (3, 1) and top[:, 0].tolist() == [1.0, 2.0, 3.0] and halos[0].shape == (3, 1) and halos[1] is None
    assert params == (1e-4, 0.1, 1.0, 0.25, 1.0, 2e-4, 9.81) and ca is True
    many = np.zeros((4, 5, 32), np.float32)
    f = WM.diagnose_baseline_flux(rec, many, many, many, np.zeros((3, 20), np.float32), 256.0, W.MPP, W.MPP, False, None)
    assert all(a.shape == (4, 5, 33) for a in f) and rec.args[2].shape == (20, 32) and rec.args[4] == 8.0 and rec.args[7] is None
    with pytest.raises(ValueError, match="halos must be"):
        WM.diagnose_NN_flux(rec, None, one, one, one, (1.0, 2.0, 3.0), 256.0, pj, W.MPP, True, (np.zeros(3),))


def test_python_shape_and_alias_validation():
    chk = colnde.check_wm_diag_arrays
    n, Nz = 6, 32
    f = lambda *s: np.zeros(s, np.float32)
    u, v, T, top, hb, ht = f(n, Nz), f(n, Nz), f(n, Nz), f(3, n), f(3, n), f(3, n)
    faces, dz, out = tuple(f(n, Nz + 1) for _ in range(3)), tuple(f(n, Nz) for _ in range(3)), tuple(f(n, Nz) for _ in range(3))
    chk(Nz, n, (u, v, T), top, (hb, ht), faces, dz, out)
    chk(Nz, n, (u, v, T), top, (None, ht), faces, dz, (u, v, T))                          # the step in place
    chk(Nz, n, (u, v, T), top, None, faces)
    with pytest.raises(ValueError, match="halos must be"):
        chk(Nz, n, (u, v, T), top, (hb,), faces)
    with pytest.raises(ValueError, match="halo_top: expected shape"):
        chk(Nz, n, (u, v, T), top, (hb, f(3, n + 1)), faces)
    with pytest.raises(ValueError, match="halo_bottom: expected shape"):
        chk(Nz, n, (u, v, T), top, (f(n, 3), None), faces)
    with pytest.raises(ValueError, match="vw: expected shape"):
        chk(Nz, n, (u, v, T), top, None, (faces[0], f(n, Nz), faces[2]))
    with pytest.raises(ValueError, match="uw overlaps wT"):
        chk(Nz, n, (u, v, T), top, None, (faces[0], faces[1], faces[0]))
    buf = f(n * (Nz + 1))
    big, part = buf.reshape(n, Nz + 1), buf[:n * Nz].reshape(n, Nz)                       # a face array and a state array on the same memory
    with pytest.raises(ValueError, match="wT overlaps T"):
        chk(Nz, n, (u, v, part), top, None, (faces[0], faces[1], big))
    with pytest.raises(ValueError, match="uw overlaps dz_vw"):
        chk(Nz, n, (u, v, T), top, None, (big, faces[1], faces[2]), (dz[0], part, dz[2]))
    with pytest.raises(ValueError, match="dz_uw overlaps u"):
        chk(Nz, n, (u, v, T), top, None, faces, (u, dz[1], dz[2]))


def test_abi_declares_binds_and_documents_the_six_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colnde.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(colnde_[a-z_0-9A-Z]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.lib()
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in zip(NEW, (15, 15, 22, 22, 13, 13)):
        assert protos[name] == arity == len(bound[name]), name
        assert hasattr(L, name), "%s declared in colnde.h but not exported" % name
    for name in NEW[::2]:
        assert "(:%s, libcolnde)" % name in jl
    assert colnde.nde.KERNEL_IDS["flux_diag"] == 10
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "colnde_wm_diagnose_flux" in body and "colnde_mpp_diagnose_flux" in body, doc
