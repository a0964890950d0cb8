"""CPU checks of the free-convection embedded step: the float64 restatement the GPU tests compare with (tests/fc_embed_restatement.py) against
hand-worked Nz = 4 cases and an independent Thomas recurrence, and what needs no device of the header, the bindings and the Python wrappers."""
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from tests import fc_embed_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("colnde_fc_embedded_step", "colnde_fc_embedded_step_dev", "colnde_fc_diagnose_wT", "colnde_fc_diagnose_wT_dev")
F4 = np.array([[0.0, 0.3, -0.2, 0.5, 0.7]])          # some network faces [0; interior; top]


# ---------------------------------------------------------------------------------------------- hand-worked, Nz = 4, dz = 1 (Lz = 4), c K = 1
def test_all_stable_column_is_untouched():
    T = np.array([[1.0, 2.0, 3.0, 4.0]])
    assert np.array_equal(R.convective_adjustment(T, 2.0, 1.0, 0.5), T)
    assert np.array_equal(R.diagnose_wT(F4, T, 4.0, 0.5), F4)
    assert not R.centred_switch(T).any() and not R.face_switch(T).any()


def test_all_unstable_column():
    T = np.array([[4.0, 3.0, 2.0, 1.0]])
    K, dt = 0.5, 2.0                                                            # c K = dt K / dz² = 1
    assert R.centred_switch(T).all()
    # rows of oceananigans_nn.jl:25-32 with κ = K everywhere: d = 1 + 2cK (last: 1 + cK), ld = ud = −cK
    L = np.array([[3.0, -1, 0, 0], [-1, 3, -1, 0], [0, -1, 3, -1], [0, 0, -1, 2]])
    Tn = R.convective_adjustment(T, dt, 1.0, K)
    np.testing.assert_allclose(L @ Tn[0], T[0], rtol=0, atol=1e-14)
    # faces: zero-gradient halos give g = 0 at the end faces, −1 inside: wT = F − K (−1)
    assert np.array_equal(R.face_switch(T), np.array([[False, True, True, True, False]]))
    np.testing.assert_allclose(R.diagnose_wT(F4, T, 4.0, K), F4 + np.array([[0, K, K, K, 0]]), rtol=0, atol=1e-15)


def test_one_interior_inversion_with_and_without_halos():
    T = np.array([[1.0, 3.0, 2.0, 4.0]])
    K, dt = 0.5, 2.0
    # halos absent: the CENTRED gradients (2, 1, 1, 2)/2 are all positive — no adjustment — while face 2 is unstable (g = −1)
    assert np.array_equal(R.convective_adjustment(T, dt, 1.0, K), T)
    np.testing.assert_allclose(R.diagnose_wT(F4, T, 4.0, K), F4 + np.array([[0, 0, K, 0, 0]]), rtol=0, atol=1e-15)
    # halos 5 below, 0 above: cells 0 and 3 become unstable (3 − 5 < 0, 0 − 2 < 0), κ = [K, 0, 0, K]:
    #   L = [[2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, −1], [0, 0, −1, 2]]  ->  T′ = [1/2, 3, 8/3, 10/3]
    halos = (np.array([5.0]), np.array([0.0]))
    np.testing.assert_allclose(R.convective_adjustment(T, dt, 1.0, K, halos), [[0.5, 3.0, 8.0 / 3.0, 10.0 / 3.0]], rtol=1e-15)
    # end faces: g = 1 − 5 = −4 and 0 − 4 = −4
    np.testing.assert_allclose(R.diagnose_wT(F4, T, 4.0, K, halos), F4 + np.array([[4 * K, 0, K, 0, 4 * K]]), rtol=0, atol=1e-15)
    # dz enters the gradient: Lz = 8 -> dz = 2, g halves
    np.testing.assert_allclose(R.diagnose_wT(F4, T, 8.0, K, halos), F4 + np.array([[2 * K, 0, K / 2, 0, 2 * K]]), rtol=0, atol=1e-15)
    nan = R.diagnose_wT(F4, np.array([[1.0, np.nan, 2.0, 4.0]]), 4.0, K)
    assert np.isnan(nan[0, 1:3]).all() and np.array_equal(nan[0, [0, 3, 4]], F4[0, [0, 3, 4]])      # NaN < 0 is false: κ = 0, 0 · NaN = NaN


def _thomas(T, dt, dz, K, hb=None, ht=None):
    """The formula of tests/test_column_ops.py's float64 restatement (copied, with the halo cells as arguments)."""
    out = np.empty_like(T)
    c = dt / dz ** 2
    for i in range(T.shape[0]):
        x = T[i].copy()
        ext = np.concatenate([[x[0] if hb is None else hb[i]], x, [x[-1] if ht is None else ht[i]]])
        k = np.where(ext[2:] - ext[:-2] < 0, c * K, 0.0)
        Nz = x.size
        cp = np.zeros(Nz)
        b0 = 1 + k[0] + k[1]
        cp[0] = -k[1] / b0
        x[0] /= b0
        for r in range(1, Nz):
            a = -k[r]
            b = 1 + k[r] + (k[r + 1] if r < Nz - 1 else 0.0)
            den = b - a * cp[r - 1]
            cp[r] = (-k[r + 1] if r < Nz - 1 else 0.0) / den
            x[r] = (x[r] - a * x[r - 1]) / den
        for r in range(Nz - 2, -1, -1):
            x[r] -= cp[r] * x[r + 1]
        out[i] = x
    return out


@pytest.mark.parametrize("Nz", [4, 32, 64])
def test_adjustment_against_the_thomas_recurrence_on_random_columns(Nz):
    rng = np.random.default_rng(20261018 + Nz)
    T = np.linspace(5.0, 25.0, Nz)[None, :] + 2.3 * 20.0 / (Nz - 1) * rng.standard_normal((40, Nz))      # noise of 2.3 level spacings
    hb, ht = T[:, 0] + rng.standard_normal(40), T[:, -1] + rng.standard_normal(40)
    dt, dz, K = 1200.0, 2000.0 / Nz, 10.0
    assert R.centred_switch(T).any() and not R.centred_switch(T).all()
    np.testing.assert_allclose(R.convective_adjustment(T, dt, dz, K), _thomas(T, dt, dz, K), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.convective_adjustment(T, dt, dz, K, (hb, ht)), _thomas(T, dt, dz, K, hb, ht), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.convective_adjustment(T, dt, dz, K, (hb, None)), _thomas(T, dt, dz, K, hb, None), rtol=1e-12, atol=1e-12)


def test_forcing_part_is_the_oracles_and_the_faces_difference_to_it():
    cfg, T, top, w = synthetic.inference_problem(3, 3)
    F = R.faces(cfg, w, T, top)
    dzw = R.dz_wT(cfg, w, T, top, 1000.0)
    assert np.array_equal(F[:, 0], np.zeros(9)) and np.array_equal(F[:, -1], top.astype(np.float64))
    np.testing.assert_allclose((F[:, 1:] - F[:, :-1]) / (1000.0 / 32), dzw, rtol=1e-13, atol=1e-20)
    step = R.embedded_step(cfg, w, T, top, 1000.0, 600.0, 10.0)
    assert np.array_equal(step[0], dzw)                                          # the forcing is that of T as given ...
    assert not np.array_equal(R.dz_wT(cfg, w, step[1], top, 1000.0), dzw)         # ... not of the adjusted state


def test_switch_robust_inputs_are_what_they_claim():
    for Nz in (32, 64):
        T, top, hb, ht = R.switch_robust_case(Nz, 65)
        for halos in (None, (hb, ht)):
            for a in (T, T.astype(np.float64)):
                h = None if halos is None else tuple(x.astype(a.dtype) for x in halos)
                ext = np.concatenate([(a[:, 0] if h is None else h[0])[:, None], a, (a[:, -1] if h is None else h[1])[:, None]], axis=1)
                face, cen = ext[:, 1:] - ext[:, :-1], ext[:, 2:] - ext[:, :-2]
                inner = face[:, 1:-1] if halos is None else face
                assert np.abs(inner).min() > 0.19 * 32 / Nz and np.abs(cen).min() > 0.19 * 32 / Nz
        f = R.face_switch(T, (hb, ht))
        assert (~f[0]).all() and f[1].all() and (f[2, 1:] != f[2, :-1]).all()


# ---------------------------------------------------------------------------------------------- header, bindings, wrappers (no device)
def _prototypes():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\b(colnde_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_header_bindings_library_and_julia_move_together():
    protos = _prototypes()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.lib()
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in zip(NEW, (13, 13, 10, 10)):
        assert protos[name] == arity == len(bound[name]), name
        assert hasattr(L, name), "%s declared in colnde.h but not exported" % name
    for name in ("colnde_fc_embedded_step", "colnde_fc_diagnose_wT"):
        assert "(:%s, libcolnde)" % name in jl
    assert colnde.nde.KERNEL_IDS["fc_embed"] == 9
    for doc in ("INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "colnde_fc_embedded_step" in text and "colnde_fc_diagnose_wT" in text, doc


def test_array_rules_of_the_python_wrappers():
    chk = colnde.check_fc_embed_arrays
    buf = np.zeros(3 * 5 * 32 + 5 * 33, np.float32)
    T, dz, To = (buf[i * 160:(i + 1) * 160].reshape(5, 32) for i in range(3))
    faces = buf[480:].reshape(5, 33)
    top, hb, two = np.zeros(5, np.float32), np.zeros(5, np.float32), np.zeros(6 * 32, np.float32)
    chk(32, 5, T, top, (hb, None), dz, To, faces)
    chk(32, 5, T, top, None, dz, T, faces)                                       # T_out may be T itself
    with pytest.raises(ValueError, match="T: expected shape"):
        chk(32, 5, T.T, top)
    with pytest.raises(ValueError, match="top_flux: expected shape"):
        chk(32, 5, T, top[:4])
    with pytest.raises(ValueError, match="halo_top: expected shape"):
        chk(32, 5, T, top, (None, hb[:2]))
    with pytest.raises(ValueError, match="halos must be"):
        chk(32, 5, T, top, (hb,))
    with pytest.raises(ValueError, match="faces_out: expected shape"):
        chk(32, 5, T, top, None, dz, To, To)
    with pytest.raises(ValueError, match="dz_out overlaps T"):
        chk(32, 5, T, top, None, T, To)
    with pytest.raises(ValueError, match="T_out overlaps T"):
        chk(32, 5, two[:160].reshape(5, 32), top, None, dz, two[32:].reshape(5, 32))     # shifted by one column: not in place
    with pytest.raises(ValueError, match="dz_out overlaps T_out"):
        chk(32, 5, T, top, None, dz, dz)
