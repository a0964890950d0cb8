"""The member loss of an ensemble on the host (no GPU): colnde_ensemble_set_member_loss and the three member entry points agree across
include/colnde.h, the library, the ctypes binding and the Julia wrappers; csrc/member_loss.h — the validation and the K LossWeights rows the kernels
read — compiled alone and held to a Python restatement; the float64 reference the GPU tests use (the oracle one column at a time, combined with the
weights: tests/member_loss_cases.py) is the oracle on the subset of columns for a 0/1 mask; and the inputs of the GPU tests have the power to see a
kernel that ignores the member."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import colnde
from colnde import _lib
from colnde.wind_mixing import member_column_weights, member_fractions
from oracle import nde_oracle as O
from tests import member_loss_cases as M
from tests.test_abi import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"colnde_ensemble_set_member_loss": 3, "colnde_ensemble_member_loss_dev": 3, "colnde_ensemble_member_loss_grad_dev": 3,
                "colnde_ensemble_member_loss_grad": 3}


def test_the_entry_points_in_header_library_ctypes_and_julia():
    L = _lib.lib()
    protos = _header_prototypes()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in ENTRY_POINTS.items():
        assert protos[name] == arity, name
        assert hasattr(L, name) and len(bound[name]) == arity, name
        assert re.search(r"ccall\(\(:%s,\s*libcolnde\)" % name, jl), name
    for fn in ("set_member_loss!", "member_loss!", "member_loss_grad!"):
        assert re.search(r"^(function )?%s\(" % re.escape(fn), jl, re.M), fn
    for method in ("set_member_loss", "member_loss", "member_loss_grad"):
        assert callable(getattr(colnde.ColumnNDEEnsemble, method)) and callable(getattr(colnde.FreeConvectionEnsemble, method))
    assert L.colnde_version() == 106                                          # the additions are additive
    header = open(os.path.join(ROOT, "include", "colnde.h")).read()
    for cite in ("NDE_training.jl:256-288", "loss.jl:11-31", "train_free_convection_nde.jl:60-66", "member_loss=scalings|columns|scalings+columns"):
        assert cite in header, cite
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s`" % name in table for name in ENTRY_POINTS)


# ---- csrc/member_loss.h, compiled alone ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("member_loss") / "member_loss_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "member_loss_check.cpp"),
                           "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _hex(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).ravel().view(np.uint32))


def _rows(header, wm, n_save, Nz, sc, cw, K, n_col):
    line = "W %d %d %d %d %d %d %d %s %s" % (wm, n_save, Nz, K, n_col, sc is not None, cw is not None, "" if sc is None else _hex(sc), "" if cw is None else _hex(cw))
    out = header([line])
    assert len(out) == K
    return np.array([[int(v, 16) for v in ln.split()] for ln in out], np.uint32).view(np.float32)


def _loss_weights_floats(scalings6, n_col_total, n_save, Nz, wind_mixing=True):
    """loss_weights() of api.hip, restated: float(scaling / (double)(n_col_total * n_save * Nz)) and the same over Nz + 1 for the gradient terms"""
    w = np.zeros(8, np.float32)
    n_prof, n_grad = float(n_col_total) * n_save * Nz, float(n_col_total) * n_save * (Nz + 1)
    sc = np.asarray(scalings6, np.float32)
    if wind_mixing:
        for k in range(3):
            w[k] = np.float32(np.float64(sc[k]) / n_prof)
            w[3 + k] = np.float32(np.float64(sc[3 + k]) / n_grad)
    else:
        w[2] = np.float32(np.float64(sc[2]) / n_prof)
    return w


SCALINGS = np.array([[1, 1, 1, 5e-3, 5e-3, 5e-3], [0.37, 0.37, 1.0, 2.1e-3, 2.1e-3, 8.4e-3], [12.5, 12.5, 1.0, 0.0, 0.0, 0.0]], np.float32)


@pytest.mark.parametrize("wm,n_save,Nz", [(1, 5, 32), (1, 289, 32), (0, 5, 32), (0, 9, 64)])
@pytest.mark.parametrize("n_col", [8, 17, 40])
def test_loss_weight_rows_are_the_restatement(header, wm, n_save, Nz, n_col):
    K = 3
    ones = np.ones((K, n_col), np.float32)
    base = np.array([_loss_weights_floats(SCALINGS[k], n_col, n_save, Nz, bool(wm)) for k in range(K)])
    # all-ones weights and no weights: loss_weights()'s floats, bit for bit
    for cw in (None, ones):
        got = _rows(header, wm, n_save, Nz, SCALINGS, cw, K, n_col)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
        assert np.array_equal(got, M.loss_weight_rows(SCALINGS, cw, n_col, n_save, Nz, bool(wm)))
    # no scalings: every scaling 1
    got = _rows(header, wm, n_save, Nz, None, None, K, n_col)
    assert np.array_equal(got, np.array([_loss_weights_floats(np.ones(6), n_col, n_save, Nz, bool(wm))] * K))
    # a 0/1 mask: the floats of a handle created on the member's columns alone
    masks = M.masks_for(n_col)
    cw = M.mask_weights(masks, n_col)
    got = _rows(header, wm, n_save, Nz, SCALINGS, cw, K, n_col)
    for k in range(K):
        assert np.array_equal(got[k], _loss_weights_floats(SCALINGS[k], len(masks[k]), n_save, Nz, bool(wm))), k
    # fractional weights: the sum is taken in double
    rng = np.random.default_rng(n_col)
    frac = rng.uniform(0.0, 3.0, (K, n_col)).astype(np.float32)
    frac[1, ::2] = 0.0
    got = _rows(header, wm, n_save, Nz, SCALINGS, frac, K, n_col)
    assert np.array_equal(got, M.loss_weight_rows(SCALINGS, frac, n_col, n_save, Nz, bool(wm)))
    if not wm:
        assert not got[:, [0, 1, 3, 4, 5, 6, 7]].any()                        # free convection: only scalings[k][2] is read


def test_refusals_in_their_order(header):
    OK, BAD_SCALING, BAD_WEIGHT, EMPTY, GLOBAL = range(5)
    K, n = 3, 8
    sc, cw = SCALINGS.copy(), M.mask_weights(M.MASKS8, n)

    def verdict(s, w, total=n):
        line = "V %d %d %d %d %d %s %s" % (K, n, total, s is not None, w is not None, "" if s is None else _hex(s), "" if w is None else _hex(w))
        return tuple(int(v) for v in header([line])[0].split())

    def edit(a, k, i, v):
        b = a.copy()
        b[k, i] = v
        return b

    assert verdict(sc, cw) == (OK, -1, -1) and verdict(None, cw) == (OK, -1, -1) and verdict(sc, None) == (OK, -1, -1)
    assert verdict(edit(sc, 1, 4, 0.0), cw)[0] == OK                          # a zero scaling switches a term off
    for bad in (np.nan, np.inf, -np.inf, -1e-30, -1.0):
        assert verdict(edit(sc, 1, 4, bad), cw) == (BAD_SCALING, 1, 4), bad
        assert verdict(sc, edit(cw, 2, 5, bad)) == (BAD_WEIGHT, 2, 5), bad
    assert verdict(sc, edit(edit(edit(cw, 0, 0, 0.0), 0, 2, 0.0), 0, 5, 0.0))[:2] == (EMPTY, 0)      # member 0 = {0, 2, 5}: nothing left
    assert verdict(sc, np.zeros_like(cw))[:2] == (EMPTY, 0)
    assert verdict(sc, cw, total=16)[0] == GLOBAL and verdict(edit(sc, 0, 0, np.nan), cw, total=16)[0] == GLOBAL      # the handle first
    assert verdict(edit(sc, 2, 0, np.nan), edit(cw, 0, 1, -1.0)) == (BAD_WEIGHT, 0, 1)                                # member by member
    assert verdict(edit(sc, 0, 5, np.nan), edit(cw, 0, 1, -1.0)) == (BAD_SCALING, 0, 5)                               # ... its scalings first
    assert header(["N 0 0", "N 1 0", "N 0 1", "N 1 1"]) == ["none", "scalings", "columns", "scalings+columns"]


def test_python_argument_helpers():
    cw = member_column_weights(3, 8, M.MASKS8)
    assert np.array_equal(cw, M.mask_weights(M.MASKS8, 8)) and cw.dtype == np.float32
    for bad in ([(0,), (1,)], [(0,), (), (1,)], [(0,), (8,), (1,)], [(0, 0), (1,), (2,)], [(-1,), (1,), (2,)]):
        with pytest.raises(ValueError):
            member_column_weights(3, 8, bad)
    assert member_fractions(3, M.FRACTIONS) == [M.FRACTIONS] * 3
    with pytest.raises(ValueError):
        member_fractions(3, [M.FRACTIONS] * 2)


# ---- the float64 reference of the GPU tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["base", "sched", "rkc2"])
def test_a_mask_is_the_oracle_on_the_subset_of_columns(kind):
    n = 8
    cw = M.mask_weights(M.MASKS8, n)
    scs = M.member_scalings(kind, n, M.key(cw))
    for k, idx in enumerate(M.MASKS8):
        tot, terms, g = M.reference(kind, n, k, scs[k], cw[k])
        tot_s, terms_s, g_s = M.subset_oracle(kind, n, k, scs[k], idx)
        assert abs(tot - tot_s) <= 1e-12 * abs(tot_s), (k, tot, tot_s)
        assert np.abs(terms - terms_s).max() <= 1e-12 * np.abs(terms_s).max(), k
        assert np.linalg.norm(g - g_s) <= 1e-12 * np.linalg.norm(g_s), k
    # all-ones weights: the oracle on every column
    p, truth, _, sched = M.problem(kind, n)
    tot, terms, g = M.reference(kind, n, 0, scs[0], np.ones(n))
    tot_a, terms_a, g_a = M.subset_oracle(kind, n, 0, scs[0], range(n))
    assert abs(tot - tot_a) <= 1e-12 * abs(tot_a) and np.linalg.norm(g - g_a) <= 1e-12 * np.linalg.norm(g_a)


@pytest.mark.parametrize("kind", ["base", "sched", "rkc2"])
def test_power_the_inputs_see_a_kernel_that_ignores_the_member(kind):
    """Oracle only.  Exchange the masks of members 0 and 1, or their scalings: both rows must move by at least ten times the bounds the GPU tests hold
    (8e-5 of the total, 2e-4 of the gradient's norm) — a kernel that reads another member's weights or scalings, or none, cannot pass them.  The
    scalings exist at all only if every member's Lu + Lv and gradient sums are positive."""
    n = 8
    cw = M.mask_weights(M.MASKS8, n)
    cw[2] = M.FRACTIONAL8                                                      # the GPU test's fourth input: the fractional row, on member 2
    for c in (M.mask_weights(M.MASKS8, n), cw):
        for k in range(M.K):
            _, terms, _ = M.combine(M.column_rows(kind, n, k, (1.0,) * 6), c[k])
            assert terms[0] + terms[1] > 0 and terms[3] + terms[4] > 0 and terms[2] > 0 and terms[5] > 0, (k, terms)
    scs = M.member_scalings(kind, n, M.key(cw))
    assert np.isfinite(scs).all() and (scs > 0).all()
    base = [M.reference(kind, n, k, scs[k], cw[k]) for k in range(M.K)]
    swap = {0: 1, 1: 0}
    for what in ("masks", "scalings"):
        for k, j in swap.items():
            other = M.reference(kind, n, k, scs[k], cw[j]) if what == "masks" else M.reference(kind, n, k, scs[j], cw[k])
            d_tot = abs(other[0] - base[k][0]) / abs(base[k][0])
            d_g = np.linalg.norm(other[2] - base[k][2]) / np.linalg.norm(base[k][2])
            print("%s exchanged, member %d: total moves by %.3e, gradient by %.3e of its norm" % (what, k, d_tot, d_g))
            assert d_tot >= 10 * M.LOSS_RTOL and d_g >= 10 * M.GRAD_RTOL, (what, k, d_tot, d_g)
    # the fractional row against the all-ones row of the same member
    ones = M.reference(kind, n, 2, scs[2], np.ones(n))
    assert abs(ones[0] - base[2][0]) / abs(base[2][0]) >= 10 * M.LOSS_RTOL
    assert np.linalg.norm(ones[2] - base[2][2]) / np.linalg.norm(base[2][2]) >= 10 * M.GRAD_RTOL


@pytest.mark.parametrize("n_col", [17, 40])
@pytest.mark.parametrize("kind", ["base", "sched"])
def test_power_weights_read_by_the_place_in_the_tile_are_seen(kind, n_col):
    """Oracle only, more than one 16-column tile: under M.tile_weights a kernel that read the weight of column c at c % 16 would compute another loss for
    every member — by at least ten times the bounds the GPU test holds (17 columns: the one column of the second tile is enough)."""
    cw, scs = M.tile_weights(n_col), M.fixed_scalings()
    wrong = M.tile_local(cw)
    assert (cw.sum(axis=1) > 0).all() and (wrong.sum(axis=1) > 0).all() and all(not np.array_equal(cw[k], wrong[k]) for k in range(M.K))
    for k in range(M.K):
        ref, bad = M.reference(kind, n_col, k, scs[k], cw[k]), M.reference(kind, n_col, k, scs[k], wrong[k])
        d_tot = abs(bad[0] - ref[0]) / abs(ref[0])
        d_g = np.linalg.norm(bad[2] - ref[2]) / np.linalg.norm(ref[2])
        print("%s, %d columns, member %d: weights by c %% 16 move the total by %.3e, the gradient by %.3e of its norm" % (kind, n_col, k, d_tot, d_g))
        assert d_tot >= 10 * M.LOSS_RTOL and d_g >= 10 * M.GRAD_RTOL, (k, d_tot, d_g)
