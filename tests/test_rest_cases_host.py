"""The columns at rest of tests/rest_cases.py on the CPU: the float64 references that tests/test_gpu_rest_columns.py holds the kernels to stay inside
their own conditions on this state — float32 and float64 agree on which faces are +Inf, −Inf, NaN and `Ri > 0`; the non-finite outputs are exactly
the neutral resting layer's (kind 2); the training oracle and the closure's finite-difference yardstick are finite and well conditioned — and the
embedding bounds written into the GPU module are 10 x (at most 12 x) the float32 restatement's own distance from float64, computed here."""
import functools

import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as O
from tests import closure_common as C
from tests import rest_cases as RC
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W
from tests import test_gpu_rest_columns as G

N, NZ = 16, 32
DZ = W.LZ / NZ
DT = 60.0


@functools.lru_cache(maxsize=None)
def _state():
    return RC.rest_state(synthetic.wind_mixing_problem(N, n_frames=5, weight_divisor=1e2))


def _halos(rs, halo):
    return (rs.halo_bottom, rs.halo_top) if halo else None


def test_the_four_kinds():
    rs = _state()
    Nz = NZ
    u, v, T = (rs.p.x0[:, f * Nz:(f + 1) * Nz] for f in range(3))
    k0, k1, k2, k3 = (rs.mask(k) for k in range(4))
    assert k0.sum() == k1.sum() == k2.sum() == k3.sum() == 4
    assert not u[k0].any() and not v[k0].any()
    for k in (k1, k2):
        assert not u[k, :16].any() and not v[k, :16].any() and (u[k, 16:] != 0).all() and (v[k, 16:] != 0).all()
    assert (np.diff(T[k0], axis=1)[:, 19] < 0).all()                                           # the resting face 20 is unstably stratified
    assert (np.diff(T[k2], axis=1)[:, 4:8] == 0).all() and (np.diff(T[k3], axis=1)[:, 9] == 0).all()
    assert (u[k3] != 0).all() and (v[k3] != 0).all()
    assert rs.u.dtype == np.float32 and rs.halo_bottom.shape == rs.halo_top.shape == rs.top.shape == (3, N)


@pytest.mark.parametrize("halo", [False, True])
def test_richardson_masks_agree_between_float32_and_float64(halo):
    rs = _state()
    Ri64 = R.richardson_number(rs.u, rs.v, rs.T, DZ, W.MPP, _halos(rs, halo))
    Ri32 = R.richardson_number(rs.u, rs.v, rs.T, np.float32(DZ), W.MPP, _halos(rs, halo), np.float32)
    for f in (np.isposinf, np.isneginf, np.isnan, lambda a: a > 0, lambda a: a == 0):
        assert np.array_equal(f(Ri64), f(Ri32))
    I = Ri64[:, 1:NZ]
    counts = (int(np.isposinf(I).sum()), int(np.isneginf(I).sum()), int(np.isnan(I).sum()), int((I == 0).sum()))
    assert counts == (224, 4, 16, 4), counts
    assert np.array_equal(np.isnan(I).any(axis=1), rs.mask(2)) and np.isnan(I[rs.mask(2), 4:8]).all()
    assert np.array_equal(np.isneginf(I).any(axis=1), rs.mask(0)) and np.array_equal((I == 0).any(axis=1), rs.mask(3))
    assert np.isfinite(I[rs.mask(3)]).all()                                                     # the control columns


@pytest.mark.parametrize("halo", [False, True])
@pytest.mark.parametrize("ca", [False, True])
def test_implicit_step_is_non_finite_on_the_neutral_resting_layer_only(ca, halo):
    rs = _state()
    hb = rs.halo_bottom if halo else None
    o64 = O.modified_pacanowski_philander_step(rs.u, rs.v, rs.T, DT, DZ, convective_adjustment=ca, halo_bottom=hb, **W.MPP)
    o32 = O.modified_pacanowski_philander_step(rs.u, rs.v, rs.T, DT, DZ, convective_adjustment=ca, halo_bottom=hb, dtype=np.float32, **W.MPP)
    k2 = rs.mask(2)
    for o in (o64, o32):
        for a in o[:2]:
            assert np.array_equal(~np.isfinite(a).all(axis=1), k2) and not np.isfinite(a[k2]).any()
        assert np.array_equal(o[2][:, 0], rs.T[:, 0].astype(o[2].dtype))                         # T′[0] = T_bottom, kind 2 included
        if ca:
            assert np.isfinite(o[2]).all()                                                       # NaN > 0 is false: ν_T = 1
        else:
            assert np.array_equal(~np.isfinite(o[2][:, 1:]).all(axis=1), k2) and not np.isfinite(o[2][k2, 1:]).any()
    for a64, a32 in zip(o64, o32):
        assert o32[0].dtype == np.float32 and np.array_equal(np.isfinite(a64), np.isfinite(a32))
        ok = np.isfinite(a64)
        assert np.abs(a32[ok] - a64[ok]).max() <= 1e-7 * np.abs(a64[ok]).max()


def _distance(a32, a64):
    """max|f32 − f64| / max|f64| over the entries where the float64 reference is finite, after asserting that the masks agree"""
    assert np.array_equal(np.isnan(a32), np.isnan(a64)) and np.array_equal(np.isinf(a32), np.isinf(a64))
    ok = np.isfinite(a64)
    return float(np.abs(a32[ok].astype(np.float64) - a64[ok]).max() / np.abs(a64[ok]).max())


@functools.lru_cache(maxsize=None)
def _flux_distances():
    """{("base" | "nn", ca): (uw, vw, wT)}: the float32 restatement's distance from the float64 one, the larger over halos given / absent"""
    rs = _state()
    p = synthetic.wind_mixing_problem(N, n_frames=5, weight_divisor=1.0)                         # the embedding tests' weights (same columns)
    out = {}
    for ca in (False, True):
        base, nn = np.zeros(3), np.zeros(3)
        for halo in (False, True):
            h = _halos(rs, halo)
            hb = (rs.halo_bottom, None) if halo else None                                        # (colnde_mpp_diagnose_flux takes the bottom halo alone)
            b64 = R.diagnose_baseline_flux(rs.u, rs.v, rs.T, rs.top, DZ, W.MPP, ca, hb)
            b32 = R.diagnose_baseline_flux(rs.u, rs.v, rs.T, rs.top, np.float32(DZ), W.MPP, ca, hb, np.float32)
            n64 = R.diagnose_NN_flux(p.cfg, p.weights_truth, rs.u, rs.v, rs.T, rs.top, W.LZ, W.MPP, ca, h)
            n32 = R.diagnose_NN_flux(p.cfg, p.weights_truth, rs.u, rs.v, rs.T, rs.top, W.LZ, W.MPP, ca, h, np.float32)
            for k in range(3):
                for f64 in (b64[k], n64[k]):
                    nan = np.isnan(f64)
                    assert not np.isinf(f64).any() and np.array_equal(nan.any(axis=1), rs.mask(2) & (k < 2 or not ca))
                    assert not nan.any() or (nan[rs.mask(2)][:, 5:9].all() and not np.delete(nan, np.s_[5:9], axis=1).any())
                base[k] = max(base[k], _distance(b32[k], b64[k]))
                nn[k] = max(nn[k], _distance(n32[k], n64[k]))
        out[("base", int(ca))], out[("nn", int(ca))] = tuple(base), tuple(nn)
    return out


def test_face_fluxes_have_the_same_masks_in_both_precisions():
    """(asserted while the distances are taken: NaN on faces 5..8 of the kind-2 columns and nowhere else; no NaN face of wT under ca = True)"""
    d = _flux_distances()
    print("float32 restatement's distance from float64 on the columns at rest:", d)
    assert all(np.isfinite(v).all() for v in d.values())


def test_embedding_bounds_of_the_gpu_module_are_10x_the_float32_restatements_distance():
    d = _flux_distances()
    for ca in (0, 1):
        for name, bounds in (("base", G.BASE_BOUND[ca]), ("nn", G.NN_BOUND[ca])):
            for e, b in zip(d[(name, ca)], bounds):
                assert 10 * e <= b <= 12 * e, (name, ca, e, b)


def test_training_oracle_is_finite_on_columns_at_rest():
    """weights / 1e2, 5 frames, the truth of weights_truth: loss 7.8e-5, every gradient entry finite"""
    rs = _state()
    p = rs.p
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)
    tot, terms, g, sol = O.loss_and_grad(p.cfg, p.x0, p.bcs, p.weights, truth, O.default_loss_scalings(p.cfg))
    assert np.isfinite(sol).all() and np.isfinite(terms).all() and np.isfinite(g).all() and g.any()
    assert 0 < tot < 1.0


def test_T_terms_bound_of_the_gpu_module_is_10x_the_float32_oracles_distance():
    """oracle.cref (float32 C) against the float64 oracle on the three training inputs of the GPU module: the total, the u and v terms and the
    gradient are inside the existing LOSS_RTOL / GRAD_REL of tests/test_gpu_parity.py; the two T terms are not, and T_TERMS_RTOL is 10 x theirs."""
    from oracle import cref
    from tests.test_gpu_parity import GRAD_REL, LOSS_RTOL, SOL_ATOL, _rel
    worst = 0.0
    for n, smooth_Ri in ((N, False), (N, True), (1, False)):
        p, truth, tot, terms, g, sol = G._train_ref(n, smooth_Ri)
        t32, terms32, g32, sol32 = cref.loss_grad(p.cfg, p.x0, p.bcs, p.weights, truth, G.TRAIN_SC, want_sol=True)
        rel = np.abs(terms32 / terms - 1)
        assert np.abs(sol32 - sol).max() < 0.1 * SOL_ATOL and abs(t32 / tot - 1) < 0.1 * LOSS_RTOL and _rel(g32, g) < 0.1 * GRAD_REL
        assert rel[[0, 1, 3, 4]].max() < 0.1 * LOSS_RTOL
        worst = max(worst, float(rel[[2, 5]].max()))
    assert worst > 0.5 * LOSS_RTOL                                                               # the existing constant cannot hold them
    assert 10 * worst <= G.T_TERMS_RTOL <= 12 * worst, worst


def test_closure_yardstick_is_well_conditioned_on_columns_at_rest():
    """The central difference of the float64 loss at relative steps 1e-6 and 1e-5: equal to 1e-6 per component, and no component within 1e-3 of
    zero relative to the largest — tests/test_gpu_closure.py's per-component GRAD_RTOL means something on this input."""
    from tests.test_gpu_closure import SC, SETS
    rs, truth = RC.rest_closure_problem(N, SETS)
    for s in SETS:
        a = C.fd_grad(rs.p.cfg, rs.p, truth, s, SC, rel=1e-6)
        b = C.fd_grad(rs.p.cfg, rs.p, truth, s, SC, rel=1e-5)
        assert np.isfinite(a).all() and np.abs(a / b - 1).max() < 1e-6, (a, b)
        assert np.abs(a).min() > 1e-3 * np.abs(a).max(), a
