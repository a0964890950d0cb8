"""CPU-side checks of the free-convection ensemble interface (colnde_create_fc_ensemble, colnde_ensemble_column_loss_dev,
colnde_ensemble_causal_penalty_dev): declared, exported, bound in ctypes and in the Julia module; every refusal that is decided from the
configuration and the environment names its reason before any device work; without a GPU a valid configuration fails loudly; the Python
front-ends check shapes before the library is asked for a handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde.config import to_c_config
from colnde.nde import ENGINE_FC32, ENGINE_TILE16, check_fc_ensemble_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["colnde_create_fc_ensemble", "colnde_ensemble_column_loss_dev", "colnde_ensemble_causal_penalty_dev"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _create(cfg, n_col, K, engine=0):
    c, keep = to_c_config(cfg, n_col, 0, engine)
    h = ctypes.c_void_p()
    rc = _lib.lib().colnde_create_fc_ensemble(ctypes.byref(c), K, ctypes.byref(h))
    return rc, _lib.lib().colnde_last_error().decode(), h


def _fc(n=8, **kw):
    return synthetic.free_convection_problem(n, n_save=3, **kw).cfg


def test_fc_ensemble_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colnde.h")).read(), flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in bound, name
        assert hasattr(L, name), name
    assert colnde.FreeConvectionEnsemble.__mro__[1] is colnde.ColumnNDEEnsemble


def test_julia_module_wraps_the_three_symbols():
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s,\s*libcolnde\)" % name, jl), name


def test_configuration_refusals_name_their_reason_before_any_device_work():
    """Decided from the configuration alone (this machine may have no GPU): each names why, and the handle stays NULL."""
    cases = [
        (synthetic.wind_mixing_problem(8, n_frames=3).cfg, 8, 3, 0, "wind-mixing"),
        (_fc(layer_sizes=(32, 48, 40, 31)), 8, 3, 0, "fc32 shape"),                              # another network
        (synthetic.free_convection_problem(8, Nz=16, n_save=3).cfg, 8, 3, 0, "Nz = 16"),          # another Nz
        (_fc().with_(stepper="rkc2"), 8, 3, 0, "fc32 shape"),                                    # FreeConvectionNDE under RKC2 is tile16's
        (_fc(), 8, 3, ENGINE_TILE16, "engine"),
        (_fc().with_(substeps=0), 8, 3, 0, "substeps = 0"),
        (_fc(convective_adjustment=True, substeps=2), 8, 3, 0, "colnde_min_substeps"),          # K = 10: lambda dt far outside RK4's region at two sub-steps
        (_fc(), 8, 0, 0, "n_models"),
        (_fc(), 8, 65536, 0, "n_models"),
        (_fc(), 4097, 3, 0, "4,096 columns"),
    ]
    for cfg, n_col, K, engine, what in cases:
        rc, msg, h = _create(cfg, n_col, K, engine)
        assert rc != 0 and not h.value and what in msg, (what, msg)
    assert colnde.min_substeps(_fc(convective_adjustment=True, substeps=2)) > 2


@pytest.mark.parametrize("name,value", [("COLNDE_FC", "0"), ("COLNDE_FC_CW", "32"), ("COLNDE_FC_BLOCK", "32")])
def test_switches_that_send_a_single_handle_elsewhere_are_refused(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    rc, msg, h = _create(_fc(), 8, 3)
    assert rc != 0 and not h.value and name in msg, msg


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure")
@pytest.mark.parametrize("engine", [0, ENGINE_FC32])
def test_valid_configuration_without_gpu_fails_loudly(engine):
    for cfg in (_fc(), _fc(Nz=64), _fc(convective_adjustment=True, substeps=40, t_end=0.01), _fc(convective_adjustment=True, substeps=2, t_end=0.01).with_(stepper="rkc2")):
        rc, msg, h = _create(cfg, 8, 4, engine)
        assert rc != 0 and not h.value
        assert "no HIP device" in msg and "no CPU fallback" in msg, msg
    with pytest.raises(colnde.ColndeError, match="no HIP device"):
        colnde.FreeConvectionEnsemble(_fc(), 8, 4)


def test_create_ensemble_still_refuses_free_convection():
    c, keep = to_c_config(_fc(), 8, 0, 0)
    h = ctypes.c_void_p()
    rc = _lib.lib().colnde_create_ensemble(ctypes.byref(c), 3, None, ctypes.byref(h))
    assert rc != 0 and not h.value and "free-convection" in _lib.lib().colnde_last_error().decode()
    with pytest.raises(colnde.ColndeError, match="free-convection"):
        colnde.ColumnNDEEnsemble(_fc(), 8, 3)


def test_python_shape_checks_raise_before_a_handle_is_requested(monkeypatch):
    cfg = _fc()
    P, K, n = cfg.n_params, 3, 8
    check_fc_ensemble_arrays(cfg, n, K, np.zeros((K, P)), np.zeros(K), np.zeros(K), np.zeros((K, n, 3, 32)), np.zeros((K, P + 8)))
    for kw, what in ((dict(weights=np.zeros((2, P))), "weights"), (dict(weights=np.zeros((K, P - 1))), "weights"), (dict(etas=np.zeros((K, 1))), "etas"),
                     (dict(coeff=np.zeros(K + 1)), "coeff"), (dict(sol=np.zeros((K, n, 3, 31))), "sol"), (dict(result=np.zeros((K, P))), "result")):
        with pytest.raises(ValueError, match=what):
            check_fc_ensemble_arrays(cfg, n, K, **kw)
    # from here on a request for a handle is an error of the test: the checks must come first
    def no_handle(*a):
        raise AssertionError("the library was asked for a handle")
    monkeypatch.setattr(_lib.lib(), "colnde_create_fc_ensemble", no_handle, raising=False)
    with pytest.raises(ValueError, match="free-convection"):
        colnde.FreeConvectionEnsemble(synthetic.wind_mixing_problem(8, n_frames=3).cfg, 8, K)
    with pytest.raises(ValueError, match="Nz = 32 or 64"):
        colnde.FreeConvectionEnsemble(_fc(layer_sizes=(32, 48, 40, 31)), 8, K)
    with pytest.raises(ValueError, match="n_columns"):
        colnde.FreeConvectionEnsemble(cfg, 4097, K)
    with pytest.raises(ValueError, match="n_models"):
        colnde.FreeConvectionEnsemble(cfg, 8, 0)
    from colnde.free_convection import compute_nde_solution_history, nde_loss_history, train_neural_differential_equation_ensemble
    p = synthetic.free_convection_problem(n, n_save=3)
    W = np.zeros((K, P), np.float32)
    truth = np.zeros((n, 3, 32), np.float32)
    with pytest.raises(ValueError, match="etas"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W, np.full(2, 1e-3), 1)
    with pytest.raises(ValueError, match="coeff"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W, np.full(K, 1e-3), 1, causal_coeff=np.zeros(K + 1))
    with pytest.raises(ValueError, match="weights"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W[:, :5], np.full(K, 1e-3), 1)
    with pytest.raises(ValueError, match="weights"):
        compute_nde_solution_history(p.x0, p.bcs, cfg, W[:, :5])
    with pytest.raises(ValueError, match="true_sols"):
        nde_loss_history(p.x0, p.bcs, truth[:, :2], cfg, W)
    with pytest.raises(ValueError, match="nde_params"):
        compute_nde_solution_history(p.x0, p.bcs[:, :1], cfg, W)
