"""The facts tests/wm_generic_cases.py states and tests/test_gpu_wm_generic.py relies on, checked on the CPU (no GPU): the bounds are 10 x the float32
restatement's distance from the float64 one; float32 and float64 take the same `Ri > 0` branch on every face of the diagnosis inputs; the weights
tell exchanged nets and dropped biases apart by far more than the bounds; the state does not depend on the layer sizes; and the LDS plan of
csrc/engine_wm_embed_any.h, compiled alone, is the Python restatement, fits every case shape and refuses 96-2048-2048-31."""
import os
import subprocess

import numpy as np
import pytest

import colnde
from tests import distinct_nets as D
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W
from tests import wm_generic_cases as C
from tests.test_gpu_parity import _record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_state_does_not_depend_on_the_layer_sizes():
    p0 = C.problem(C.FIXED)
    for name, (sizes, acts, _) in C.SHAPES.items():
        p = C.problem(name)
        assert tuple(p.cfg.layer_sizes) == sizes and tuple(p.cfg.activations) == acts and p.cfg.Nz == 32
        assert np.array_equal(p.x0, p0.x0) and np.array_equal(p.bcs, p0.bcs), name
        D.assert_distinct_and_biased(p.cfg, C.weights(name))
        assert C.weights(name).shape == (p.cfg.n_params,)
    assert len(C.SHAPES["96-24-21-18-16-14-12-10-31"][0]) - 1 == colnde.config.COLNDE_MAX_LAYERS


def test_bounds_are_ten_times_the_float32_restatements_distance():
    """Measured on the machine the bounds were stored on — ∂z: uw 3.63e-7, vw 7.04e-7 (both 96-400-...), wT 4.76e-7; faces: uw 3.17e-7, vw 6.91e-7,
    wT 1.37e-7 (ca = 0) and 5.49e-8 (ca = 1: max|wT| is then the unit diffusivity's share, which float32 carries almost exactly).  Halos given or
    absent change no distance: they move two end faces that are far from the largest error."""
    dz = dict.fromkeys(C.NETS, 0.0)
    fc = {}
    for name in C.SHAPES:
        for nm, e in zip(C.NETS, C.rel_dist(C.dz_ref(name, np.float32), C.dz_ref(name))):
            dz[nm] = max(dz[nm], e)
        for ca in (0, 1):
            for halo in (False, True):
                for nm, e in zip(C.NETS, C.rel_dist(C.face_ref(name, ca, halo, np.float32), C.face_ref(name, ca, halo))):
                    fc[(ca, nm)] = max(fc.get((ca, nm), 0.0), e)
    _record("wm_generic_float32", **{"dz_" + k: v for k, v in dz.items()}, **{"face_ca%d_%s" % k: v for k, v in fc.items()})
    print("float32 restatement: dz", dz, "faces", fc)
    assert set(C.DZ_BOUND) == set(dz) and set(C.FACE_BOUND) == set(fc)
    for k, d in list(dz.items()) + list(fc.items()):
        stored = C.DZ_BOUND[k] if k in C.DZ_BOUND else C.FACE_BOUND[k]
        assert abs(stored - 10 * d) <= C.BOUND_SLACK * stored, (k, stored, 10 * d)


def test_float32_and_float64_take_the_same_branch_on_every_face_and_both_occur():
    u, v, T, top, hb, ht = C.diag_state()
    for halos in (None, (hb, ht)):
        Ri64 = R.richardson_number(u, v, T, W.LZ / 32, W.MPP, halos)
        Ri32 = R.richardson_number(u, v, T, W.LZ / 32, W.MPP, halos, np.float32)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(Ri64 > 0, Ri32 > 0)
            assert (Ri64[:, 1:-1] > 0).any() and (Ri64[:, 1:-1] <= 0).any()
    with np.errstate(invalid="ignore"):
        assert (Ri64[:, 0] > 0).any() and (Ri64[:, 0] <= 0).any() and (Ri64[:, -1] > 0).any() and (Ri64[:, -1] <= 0).any()     # (with halos: both end faces too)


@pytest.mark.parametrize("name", list(C.SHAPES))
def test_exchanged_nets_and_dropped_biases_move_the_result_by_far_more_than_the_bounds(name):
    cfg, w = C.problem(name).cfg, C.weights(name)
    u, v, T, top = C.embed_state()
    ref = C.dz_ref(name)
    for what, w2 in (("swap", D.swap_nets(cfg, w, 0, 1)), ("zero_biases", D.zero_biases(cfg, w))):
        moved = C.rel_dist(W.dz_fluxes(cfg, w2, u, v, T, top, W.LZ), ref)
        print("%s %s: dz_uw, dz_vw move by %.3g, %.3g" % (name, what, moved[0], moved[1]))
        for nm, e in zip(C.NETS[:2], moved[:2]):
            assert e > 1000 * C.DZ_BOUND[nm], (name, what, nm, e)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wm_generic") / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "wm_generic_plan_check.cpp"),
                           "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(shapes):
        r = subprocess.run([exe], input="".join("%d %s\n" % (len(s) - 1, " ".join(str(v) for v in s)) for s in shapes), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


def test_lds_plan_fits_every_case_shape_and_is_the_restatement(plan):
    shapes = [s for s, _, _ in C.SHAPES.values()] + [(96, 50, 20, 31), C.TOO_WIDE[0], (96, 600, 600, 31), (96,) + (600,) * 7 + (31,), (96, 601, 31), (96, 1, 31)]
    got = plan(shapes)
    for s, g in zip(shapes, got):
        bytes_, fits, st, gr, xs, y, b0, b1, ld0, ld1 = g
        assert bytes_ == C.lds_plan_bytes(s), s
        assert fits == (bytes_ <= C.LDS_LIMIT)
        assert fits == (s != C.TOO_WIDE[0]), (s, bytes_)                          # hidden widths up to 600 and up to COLNDE_MAX_LAYERS layers fit
        # the regions in order, none overlapping, every start a multiple of 16 bytes where 16-byte LDS accesses go (the face rows) and of 8 elsewhere
        assert (st, gr, xs, y) == (0, 1584, 3168, 3168 + 16 * 98) and b0 == y + 3 * 16 * 34 and b1 == b0 + 16 * ld0 and bytes_ == 4 * (b1 + 16 * ld1)
        assert gr % 4 == 0 and all(o % 2 == 0 for o in (xs, y, b0, b1))
        hidden = s[1:-1]
        assert ld0 >= max(hidden[0::2], default=0) and ld1 >= max(hidden[1::2], default=0)
        assert all(ld == 0 or ld % 4 == 2 for ld in (ld0, ld1))
    assert C.lds_plan_bytes(C.SHAPES["96-400-400-31"][0]) == 4 * (3168 + 1568 + 1632 + 2 * 16 * 402)
    assert got[shapes.index(C.TOO_WIDE[0])][0] == 4 * (3168 + 1568 + 1632 + 2 * 16 * 2050) > C.LDS_LIMIT
