"""CPU-side checks of the tile ensemble (colnde_create_tile_ensemble: K wind-mixing NDEs of any tile16 architecture side by side): declared, exported,
bound in ctypes and in the Julia module with four arguments; every refusal decided from the configuration and the environment names its reason before
any device work; without a GPU a valid configuration fails loudly; `train_NDE_ensemble` sends the net-split shape where it went and everything else
to `TileNDEEnsemble`, refusing what that engine lacks before a handle is made; the planner's per-model bytes and refusal threshold (csrc/tape_plan.h),
built as a stand-alone program under AddressSanitizer and UBSan, against a NumPy restatement."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde.config import to_c_config
from colnde.nde import ENGINE_FC32, ENGINE_REGTILE, ENGINE_TILE16, is_net_split_shape
from colnde.wind_mixing import WindMixingNDE, train_NDE_ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "colnde_create_tile_ensemble"
WIDE = dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
PHYS = np.array([[1e-4, 0.1, 1.0, 0.25, 1.0], [5e-4, 0.08, 0.8, 0.2, 1.2]], np.float32)


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _create(cfg, n_col, K, physics=None, engine=0):
    cc, keep = to_c_config(cfg, n_col, 0, engine)
    h = ctypes.c_void_p()
    ph = None if physics is None else np.ascontiguousarray(physics, np.float32)
    rc = _lib.lib().colnde_create_tile_ensemble(ctypes.byref(cc), K, None if ph is None else ph.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    return rc, _lib.lib().colnde_last_error().decode(), h


def _wm(n=8, **kw):
    return synthetic.wind_mixing_problem(n, n_frames=3, **kw).cfg


def test_symbol_declared_exported_and_bound_with_four_arguments():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % NAME, header, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 4, m
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 4 and hasattr(_lib.lib(), NAME)
    assert "#define COLNDE_VERSION 106" in text and _lib.lib().colnde_version() == 106           # additive: the version stays
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    m = re.search(r"ccall\(\(:%s,\s*libcolnde\),\s*Cint,\s*\(([^)]*)\)" % NAME, jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 4, m
    assert "cannot be created" not in text                                                       # the header no longer says such an ensemble does not exist
    assert issubclass(colnde.TileNDEEnsemble, colnde.ColumnNDEEnsemble)
    own = {k for k, v in vars(colnde.TileNDEEnsemble).items() if callable(v)}
    assert own == {"__init__"}                                                                   # the subclass changes the constructor only


def test_configuration_refusals_name_their_reason_before_any_device_work():
    """Decided from the configuration alone (this machine may have no GPU): each names why, and the handle stays NULL."""
    wide = _wm(**WIDE)
    bad = PHYS.copy()
    cases = [
        (synthetic.free_convection_problem(8, n_save=3).cfg, 8, 2, None, 0, "colnde_create_fc_ensemble"),
        (wide.with_(inplace_variant=True), 8, 2, None, 0, "inplace_variant"),
        (wide, 8, 2, None, ENGINE_REGTILE, "engine forced to %d" % ENGINE_REGTILE),
        (wide, 8, 2, None, ENGINE_FC32, "engine forced to %d" % ENGINE_FC32),
        (wide.with_(substeps=0), 8, 2, None, 0, "substeps = 0"),
        (wide.with_(substeps=1), 8, 2, None, 0, "needs substeps >="),                            # below the stability bound of the default constants
        (wide, 8, 0, None, 0, "n_models = 0 outside 1..65535"),
        (wide, 8, -1, None, 0, "n_models = -1 outside 1..65535"),
        (wide, 8, 65536, None, 0, "n_models = 65536 outside 1..65535"),
        (wide, 4097, 2, None, 0, "4,096 columns"),
        (_wm(Nz=64), 8, 2, None, 0, "1,024-thread taped adjoint"),                              # 16 x 192 state values: a single handle's 512-thread kernels
        (_wm(Nz=128, layer_sizes=(384, 50, 20, 127)), 8, 2, None, 0, "taped adjoint cannot run"),    # 16 x 384 > 3,072
        (_wm(layer_sizes=(96, 2048, 2048, 31)), 8, 2, None, 0, "too large"),
        (wide.with_(modified_pacanowski_philander=False, zero_weights=False), 8, 2, PHYS, 0, "modified_pacanowski_philander = 1"),
    ]
    for q, v, what in ((0, np.nan, "is not finite"), (2, 0.0, "must be > 0"), (4, -1.0, "must be > 0"), (1, 100.0, "model 1")):
        b = bad.copy()
        b[1, q] = v
        cases.append((wide, 8, 2, b, 0, what))
    assert colnde.min_substeps(wide.with_(substeps=1)) > 1
    for cfg, n_col, K, ph, engine, what in cases:
        rc, msg, h = _create(cfg, n_col, K, ph, engine)
        assert rc != 0 and not h.value and what in msg, (what, msg)
        assert "no HIP device" not in msg, msg
    cc, keep = to_c_config(wide, 8, 0, 0)
    h = ctypes.c_void_p(1)
    assert _lib.lib().colnde_create_tile_ensemble(ctypes.byref(cc), 0, None, ctypes.byref(h)) != 0 and not h.value       # a refused creator leaves NULL
    assert _lib.lib().colnde_create_tile_ensemble(ctypes.byref(cc), 2, None, None) != 0
    assert "null out pointer" in _lib.lib().colnde_last_error().decode()


@pytest.mark.parametrize("name,value", [("COLNDE_T16_DWTAPE", "0"), ("COLNDE_T16_ZTAPE", "0"), ("COLNDE_T16_BLOCK", "32"), ("COLNDE_T16_TAPE_THREADS", "512"),
                                        ("COLNDE_T16_FWD_SPLIT", "1")])
def test_switches_that_leave_the_ensemble_kernels_are_refused(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    rc, msg, h = _create(_wm(**WIDE), 8, 3)
    assert rc != 0 and not h.value and name in msg and "no HIP device" not in msg, msg


def test_colnde_create_ensemble_still_refuses_these_shapes_in_its_own_words():
    cc, keep = to_c_config(_wm(**WIDE), 8, 0, 0)
    h = ctypes.c_void_p()
    assert _lib.lib().colnde_create_ensemble(ctypes.byref(cc), 2, None, ctypes.byref(h)) != 0 and not h.value
    msg = _lib.lib().colnde_last_error().decode()
    assert "net-split shape" in msg and "96-50-20-31" in msg and "wide networks and other architectures run one handle per model" in msg


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure")
@pytest.mark.parametrize("engine", [0, ENGINE_TILE16])
def test_valid_configuration_without_gpu_fails_only_for_the_missing_device(engine):
    for cfg, K, ph in ((_wm(**WIDE), 1, None), (_wm(**WIDE), 64, None), (_wm(), 3, PHYS[[0, 1, 0]]), (_wm(layer_sizes=(96, 400, 31), activations=("mish", "identity")), 2, PHYS),
                       (_wm(Nz=16, layer_sizes=(48, 20, 15), activations=("leakyrelu", "identity")), 65535, None),
                       (_wm(modified_pacanowski_philander=False, zero_weights=False, convective_adjustment=True, kappa=10.0, stepper="rkc2", substeps=1, **WIDE), 3, None)):
        rc, msg, h = _create(cfg, 8, K, ph, engine)
        assert rc != 0 and not h.value
        assert re.search("no HIP device|no CPU fallback", msg), msg
    with pytest.raises(colnde.ColndeError, match="no HIP device|no CPU fallback"):
        colnde.TileNDEEnsemble(_wm(**WIDE), 8, 4, physics=np.tile(PHYS, (2, 1)))


def test_shape_predicate_and_what_train_NDE_ensemble_refuses_before_a_handle(monkeypatch):
    assert is_net_split_shape(_wm()) and is_net_split_shape(_wm(activations=("swish", "swish", "identity")))
    for cfg in (_wm(**WIDE), _wm(layer_sizes=(96, 32, 400, 31)), _wm(layer_sizes=(96, 400, 31), activations=("mish", "identity")), _wm(activations=("mish", "swish", "identity")),
                _wm(activations=("mish", "mish", "tanh")), _wm(Nz=16), _wm(smooth_NN=True), _wm(smooth_Ri=True), _wm(inplace_variant=True),
                synthetic.free_convection_problem(8, n_save=3).cfg):
        assert not is_net_split_shape(cfg), cfg

    made = []

    class Refused(Exception):
        pass

    def creator(name):
        def f(*a, **kw):
            made.append(name)
            raise Refused(name)
        return f
    monkeypatch.setattr(colnde.nde.ColumnNDEEnsemble, "__init__", creator("net-split"))
    monkeypatch.setattr(colnde.nde.TileNDEEnsemble, "__init__", creator("tile"))
    monkeypatch.setattr(WindMixingNDE, "__init__", lambda self, cfg, n: self.__dict__.update(cfg=cfg, n_simulations=n, engine=type("E", (), dict(device=0, matrix_arithmetic="bf16x3_exact"))()))
    for cfg, where in ((_wm(), "net-split"), (_wm(**WIDE), "tile")):
        wm = WindMixingNDE(cfg, 8)
        W = np.zeros((2, cfg.n_params), np.float32)
        del made[:]
        with pytest.raises(Refused, match=where):
            train_NDE_ensemble(wm, W, PHYS, np.full(2, 1e-3, np.float32), maxiters=1)
        assert made == [where]
    wm = WindMixingNDE(_wm(**WIDE), 8)
    W = np.zeros((2, wm.cfg.n_params), np.float32)
    del made[:]
    for kw in (dict(training_fractions=dict(T=0.8, dTdz=0.1, profile=0.5)), dict(training_simulations=[[0, 1], [2, 3]]), dict(schedule=[2, 2])):
        with pytest.raises(ValueError, match=list(kw)[0]):
            train_NDE_ensemble(wm, W, PHYS, np.full(2, 1e-3, np.float32), maxiters=1, **kw)
    assert not made                                                                            # ... before any handle is made


# ---- the planner's arithmetic (csrc/tape_plan.h) as a stand-alone sanitized program ------------------------------------------------------------------
GB3 = 3 << 30


def _plan(K, n_tiles, n_steps, nst, ns, n_params, n_col, n_save, slab_rows, R, zcol, img, planes, ag, free_b):
    """NumPy restatement: per model the stage, delta and pre-activation tapes of n_tiles x n_steps x nst records of 16 columns, the slab rows, the solution,
    the packed images, the plane images (32-bit words) and the rows in global memory; refused when K of them exceed free memory less 3 GB."""
    rec = n_tiles * n_steps * nst
    floats = rec * 16 * (ns + R + zcol) + slab_rows * (n_params + 8) + n_col * n_save * ns + img + n_tiles * ag
    b = int(np.int64(floats) * 4 + np.int64(planes) * 4)
    share = max(free_b - GB3, 0) // K
    return rec, b, share, int(b > share)


def _shape_numbers(layers, Nz):
    """what the library derives from a network (build_model, engine_tile16.h, engine_dwgemm.h), restated for the grid of cases"""
    ns = 3 * Nz
    net = sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))
    pad4 = lambda n: (n + 3) // 4 * 4
    act_total = sum(pad4(b) for b in layers[1:])
    hidden = sum(pad4(b) for b in layers[1:-1])
    R = pad4(ns) + 2 * 3 * pad4(act_total)
    zcol = pad4(3 * hidden)
    t16 = lambda n: (n + 15) // 16
    img = 3 * 2 * sum(t16(a) * t16(b) * 256 for a, b in zip(layers[:-1], layers[1:]))
    t32 = lambda n: (n + 31) // 32
    planes = 3 * 4 * sum((t16(b) * t32(a) + t16(a) * t32(b)) * 3 * 64 for a, b in zip(layers[:-1], layers[1:]))
    ld_a = pad4(act_total + 16) + 2
    return ns, 3 * net, R, zcol, img, planes, 3 * 16 * ld_a


@pytest.fixture(scope="module")
def tile_planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_ens_plan") / "tile_ens_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tile_ens_plan_check.cpp"), "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def test_per_model_bytes_and_refusal_threshold_against_numpy(tile_planner):
    shapes = [((96, 400, 400, 31), 32, True), ((96, 32, 400, 31), 32, False), ((96, 400, 31), 32, False), ((96, 24, 31), 32, False), ((48, 20, 15), 16, False)]
    cases = []
    for layers, Nz, ag_rows in shapes:
        ns, n_params, R, zcol, img, planes, ag = _shape_numbers(layers, Nz)
        for n_tiles in (1, 3, 256):
            for n_steps, nst in ((6, 4), (760, 4), (3, 9)):
                for K in (1, 5, 64, 65535):
                    n_col, n_save, slices = 16 * n_tiles - 8, 4, 8
                    base = (K, n_tiles, n_steps, nst, ns, n_params, n_col, n_save, n_tiles + slices, R, zcol, img, planes if ag_rows else 0, ag if ag_rows else 0)
                    need = _plan(*base, 0)[1]
                    # around the threshold: the K models fit exactly, one byte short per model, and far on either side (K * need - 1 still gives every model its share less one)
                    for free_b in (0, GB3, GB3 + K * need - 1, GB3 + K * need, GB3 + K * need + K, GB3 + 2 * K * need, 288 << 30):
                        cases.append(base + (free_b,))
    got = tile_planner(cases)
    refused = 0
    for case, out in zip(cases, got):
        assert out == _plan(*case), (case, out, _plan(*case))
        refused += out[3]
    assert 0 < refused < len(cases)
    # the 400-400 net of the rate tool at 8 simulations, 760 steps: tens of MB per model, weight and plane images among them
    ns, n_params, R, zcol, img, planes, ag = _shape_numbers((96, 400, 400, 31), 32)
    rec, b, share, ref = _plan(64, 1, 760, 4, ns, n_params, 8, 20, 9, R, zcol, img, planes, ag, 288 << 30)
    assert rec == 3040 and not ref and b > (img + ag) * 4 + planes * 4 and b > rec * 16 * R * 4
