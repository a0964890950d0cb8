"""CPU-side checks of the conv handle (colnde_create_conv, colnde_conv_filter: the free-convection driver's `--conv` network on the fc32 kernels):
declared, exported, bound in ctypes and in the Julia module; every refusal decided from the configuration and the environment names its reason
before any device work; without a GPU a valid configuration fails loudly."""
import ctypes
import os
import re

import pytest

import colnde
from colnde import _lib, synthetic
from colnde.config import to_c_config
from colnde.nde import ENGINE_FC32, ENGINE_REGTILE, ENGINE_TILE16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["colnde_create_conv", "colnde_conv_filter"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _create(cfg, n_col, c, engine=0):
    cc, keep = to_c_config(cfg, n_col, 0, engine)
    h = ctypes.c_void_p()
    rc = _lib.lib().colnde_create_conv(ctypes.byref(cc), c, ctypes.byref(h))
    return rc, _lib.lib().colnde_last_error().decode(), h


def _fc(n=8, **kw):
    return synthetic.free_convection_problem(n, n_save=3, **kw).cfg


def test_conv_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colnde.h")).read(), flags=re.S)
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in bound, name
        assert hasattr(L, name), name
    assert len(bound["colnde_create_conv"]) == 3 and len(bound["colnde_conv_filter"]) == 1
    assert "#define COLNDE_VERSION 106" in open(os.path.join(ROOT, "include", "colnde.h")).read()       # additive: the version stays
    assert L.colnde_conv_filter(None) == -1


def test_julia_module_wraps_the_two_symbols_with_the_headers_arity():
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    m = re.search(r"ccall\(\(:colnde_create_conv,\s*libcolnde\),\s*Cint,\s*\(([^)]*)\)", jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 3, m
    m = re.search(r"ccall\(\(:colnde_conv_filter,\s*libcolnde\),\s*Cint,\s*\(([^)]*)\)", jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 1, m


def test_configuration_refusals_name_their_reason_before_any_device_work():
    """Decided from the configuration alone (this machine may have no GPU): each names why, and the handle stays NULL."""
    cases = [
        (_fc(), 8, 1, 0, "conv_filter = 1 outside 2..8"),
        (_fc(), 8, 0, 0, "conv_filter = 0 outside 2..8"),
        (_fc(), 8, 9, 0, "conv_filter = 9 outside 2..8"),
        (synthetic.wind_mixing_problem(8, n_frames=3).cfg, 8, 3, 0, "wind-mixing"),
        (_fc(layer_sizes=(32, 48, 40, 31)), 8, 3, 0, "plain fc32 configuration"),                      # another network
        (_fc(layer_sizes=(32, 30, 128, 128, 31), activations=("relu", "relu", "relu", "identity")), 8, 3, 0, "plain fc32 configuration"),   # the Toeplitz form is tile16's
        (synthetic.free_convection_problem(8, Nz=16, n_save=3).cfg, 8, 3, 0, "Nz = 16"),               # another Nz
        (_fc(), 8, 3, ENGINE_TILE16, "engine"),
        (_fc(), 8, 3, ENGINE_REGTILE, "engine"),
        (_fc().with_(stepper="rkc2"), 8, 3, 0, "FreeConvectionNDE under RKC2"),
        (_fc().with_(substeps=0), 8, 3, 0, "substeps = 0"),
        (_fc(convective_adjustment=True, substeps=2), 8, 3, 0, "colnde_min_substeps"),                # K = 10: far outside RK4's region at two sub-steps
        (_fc(), 4097, 3, 0, "4,096 columns"),
    ]
    for cfg, n_col, c, engine, what in cases:
        rc, msg, h = _create(cfg, n_col, c, engine)
        assert rc != 0 and not h.value and what in msg, (what, msg)
        assert "no HIP device" not in msg
    assert colnde.min_substeps(_fc(convective_adjustment=True, substeps=2)) > 2


@pytest.mark.parametrize("name,value", [("COLNDE_FC", "0"), ("COLNDE_FC_CW", "32"), ("COLNDE_FC_BLOCK", "32")])
def test_switches_that_send_the_handle_to_kernels_without_a_filter_are_refused(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    rc, msg, h = _create(_fc(), 8, 3)
    assert rc != 0 and not h.value and name in msg and "no HIP device" not in msg, msg


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure")
@pytest.mark.parametrize("engine", [0, ENGINE_FC32])
def test_valid_configuration_without_gpu_fails_only_for_the_missing_device(engine):
    for cfg, c in ((_fc(), 2), (_fc(), 8), (_fc(Nz=64), 5), (_fc(convective_adjustment=True, substeps=40, t_end=0.01), 3),
                   (_fc(convective_adjustment=True, substeps=2, t_end=0.01).with_(stepper="rkc2"), 3)):
        rc, msg, h = _create(cfg, 8, c, engine)
        assert rc != 0 and not h.value
        assert re.search("no HIP device|no CPU fallback", msg), msg
    with pytest.raises(colnde.ColndeError, match="no HIP device|no CPU fallback"):
        colnde.ColumnNDE(_fc(), 8, conv=3)
    with pytest.raises(colnde.ColndeError, match="no HIP device|no CPU fallback"):
        p = synthetic.free_convection_conv_problem(3, 3, n_save=3)
        colnde.free_convection.FreeConvectionNDE(p.cfg, p.x0, p.bcs, conv=3)


def test_python_front_end_passes_the_refusal_through():
    with pytest.raises(colnde.ColndeError, match="conv_filter = 9"):
        colnde.ColumnNDE(_fc(), 8, conv=9)
