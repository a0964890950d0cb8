"""The architectures, inputs, references and bounds of the generic wind-mixing embedding kernel (csrc/engine_wm_embed_any.hip; `colnde_ensemble_wm_embedded`
with a single handle as K = 1).  A helper, not a test: shared by tests/test_wm_generic_host.py (which checks every fact stated here on the CPU) and
tests/test_gpu_wm_generic.py.

Weights: `tests/distinct_nets.weights(cfg, seed, 1.0, 1.0)` — three separately drawn O(1) nets with U(−1, 1) biases, so that a wrong per-net offset or a
dropped bias moves the result (the host test measures by how much).  State: `synthetic.wind_mixing_problem(200, n_frames=3, weight_divisor=1.0)` through
`wm_embed_common.embed_inputs` (forcing, step) and `wm_diag_restatement.diag_inputs` (faces); it does not depend on the layer sizes.

Bounds: per output field 10 x the largest distance, over all shapes, of a float32 NumPy run of the float64 restatement from the float64 one
(max|f32 − f64| / max|f64| over the 200 columns; the faces per `convective_adjustment`, the larger of halos given / absent) — the project's convention:
the kernel sums in another order than NumPy and gets that margin, no more.  The float32 run goes through the BLAS NumPy was built with, whose summation
order belongs to the machine, so the host test holds the stored numbers to `BOUND_SLACK` of the product it recomputes, not to its last digit."""
import functools
from types import SimpleNamespace

import numpy as np

from colnde import synthetic
from tests import distinct_nets as D
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W

N_ALL = 200
SEED = 3
DT = 60.0
NETS = ("uw", "vw", "wT")
FIXED = "96-50-20-31"

# name -> (layer_sizes, activations, why)
SHAPES = {
    "96-31": ((96, 31), ("identity",), "one layer"),
    "96-7-31": ((96, 7, 31), ("swish", "identity"), "a row tile narrower than 16, K = 7"),
    "96-50-20-13-31": ((96, 50, 20, 13, 31), ("mish", "tanh", "leakyrelu", "identity"), "K = 13"),
    "96-24-21-18-16-14-12-10-31": ((96, 24, 21, 18, 16, 14, 12, 10, 31), ("identity", "leakyrelu", "tanh", "mish", "relu", "swish", "tanh", "swish"),
                                   "COLNDE_MAX_LAYERS, six activations, an output layer that is not the identity"),
    "96-400-31": ((96, 400, 31), ("relu", "identity"), "train_NN_args.jl:101-103"),
    "96-400-400-31": ((96, 400, 400, 31), ("swish", "swish", "identity"), "train_NDE.jl:97-103: the LDS-pressure case"),
    "96-600-31": ((96, 600, 31), ("relu", "identity"), "the largest width in the project's tests"),
}
TOO_WIDE = ((96, 2048, 2048, 31), ("relu", "relu", "identity"))          # its plan does not fit a workgroup's LDS

# 10 x the float32 restatement's distance from float64 (tests/test_wm_generic_host.py recomputes the products; measured distances there)
DZ_BOUND = {"uw": 3.63e-6, "vw": 7.04e-6, "wT": 4.76e-6}
FACE_BOUND = {(0, "uw"): 3.17e-6, (0, "vw"): 6.91e-6, (0, "wT"): 1.37e-6, (1, "uw"): 3.17e-6, (1, "vw"): 6.91e-6, (1, "wT"): 5.49e-7}
BOUND_SLACK = 0.25           # |stored − 10 d| <= BOUND_SLACK x stored
STEP_BOUND = (2e-5, 2e-5, 2e-6)                                            # u′, v′, T′: the bounds of tests/test_column_ops.py


def rel_dist(got, ref):
    """max|got − ref| / max|ref| per array of two tuples"""
    return [float(np.abs(np.asarray(g, np.float64) - r).max() / np.abs(r).max()) for g, r in zip(got, ref)]


@functools.lru_cache(maxsize=None)
def problem(name):
    """the synthetic problem of a shape (FIXED: the 96-50-20-31 mish nets) — x0 and bcs are the same arrays for every shape"""
    if name == FIXED:
        return synthetic.wind_mixing_problem(N_ALL, n_frames=3, weight_divisor=1.0)
    sizes, acts, _ = SHAPES[name]
    return synthetic.wind_mixing_problem(N_ALL, n_frames=3, weight_divisor=1.0, layer_sizes=sizes, activations=acts)


@functools.lru_cache(maxsize=None)
def weights(name):
    w = D.weights(problem(name).cfg, SEED, 1.0, 1.0)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def embed_state():
    """(u, v, T, top) of the forcing and step tests, float32, read-only"""
    s = W.embed_inputs(problem(FIXED))
    for a in s:
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def diag_state():
    """(u, v, T, top, halo_bottom, halo_top) of the face tests"""
    s = R.diag_inputs(embed_state(), N_ALL)
    for a in s:
        a.setflags(write=False)
    return s


def step_halo(u, v, T):
    """the bottom halo cells of the step tests (tests/test_gpu_wm_embed.py's pattern)"""
    n = T.shape[0]
    return np.ascontiguousarray(np.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] + np.where(np.arange(n) % 2, 0.01, -0.01)]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def dz_ref(name, dtype=np.float64):
    """the three ∂z arrays [200, 32] of `embed_state`, computed once per process"""
    u, v, T, top = embed_state()
    r = W.dz_fluxes(problem(name).cfg, weights(name), u, v, T, top, W.LZ, dtype)
    for a in r:
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def dz_ref_diag_state(name):
    """... of `diag_state` (the face tests' calls write the ∂z arrays too)"""
    u, v, T, top, _, _ = diag_state()
    return W.dz_fluxes(problem(name).cfg, weights(name), u, v, T, top, W.LZ)


@functools.lru_cache(maxsize=None)
def face_ref(name, ca, halo, dtype=np.float64):
    """the three face arrays [200, 33] of `diag_state`"""
    u, v, T, top, hb, ht = diag_state()
    r = R.diagnose_NN_flux(problem(name).cfg, weights(name), u, v, T, top, W.LZ, W.MPP, bool(ca), (hb, ht) if halo else None, dtype)
    for a in r:
        a.setflags(write=False)
    return r


def case(name, n):
    """the first n columns: SimpleNamespace(p, w, u, v, T, top, hb, ht) on `embed_state`"""
    u, v, T, top = embed_state()
    c = lambda a: np.ascontiguousarray(a[:n])
    return SimpleNamespace(p=problem(name), w=weights(name), u=c(u), v=c(v), T=c(T), top=np.ascontiguousarray(top[:, :n]))


def diag_case(name, n):
    u, v, T, top, hb, ht = diag_state()
    c = lambda a: np.ascontiguousarray(a[:n])
    r = lambda a: np.ascontiguousarray(a[:, :n])
    return SimpleNamespace(p=problem(name), w=weights(name), u=c(u), v=c(v), T=c(T), top=r(top), hb=r(hb), ht=r(ht))


def lds_plan_bytes(sizes):
    """Python restatement of csrc/engine_wm_embed_any.h: wm_any_plan(...).bytes"""
    stride = lambda w: (w + 3) // 4 * 4 + 2 if w > 0 else 0
    L = len(sizes) - 1
    wide = [0, 0]
    for l in range(L - 1):
        wide[l & 1] = max(wide[l & 1], sizes[l + 1])
    floats = 2 * 3 * 16 * 33 + 16 * 98 + 3 * 16 * 34 + 16 * stride(wide[0]) + 16 * stride(wide[1])
    return 4 * floats


LDS_LIMIT = 160 * 1024
