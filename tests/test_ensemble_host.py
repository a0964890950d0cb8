"""CPU-side checks of the ensemble interface (colnde_create_ensemble and the colnde_ensemble_* calls): declared, exported, bound in
ctypes and in the Julia module; without a GPU creation fails loudly; the Python front-ends check the shapes of the per-model arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

import colnde
from colnde import _lib, synthetic
from colnde.config import to_c_config
from colnde.nde import check_ensemble_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["colnde_create_ensemble", "colnde_n_models", "colnde_ensemble_set_physics", "colnde_ensemble_forward_dev", "colnde_ensemble_loss_dev",
       "colnde_ensemble_loss_grad_dev", "colnde_ensemble_loss_grad", "colnde_ensemble_adam_step_dev"]


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_ensemble_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "colnde.h")).read(), flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in bound, name
        assert hasattr(L, name), name


def test_julia_module_wraps_every_ensemble_symbol():
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s,\s*libcolnde\)" % name, jl), name


def _create(cfg, n_col, K, physics=None):
    c, keep = to_c_config(cfg, n_col, 0, 0)
    h = ctypes.c_void_p()
    ph = None if physics is None else np.ascontiguousarray(physics, dtype=np.float32)
    rc = _lib.lib().colnde_create_ensemble(ctypes.byref(c), K, ph.ctypes.data_as(ctypes.c_void_p) if ph is not None else None, ctypes.byref(h))
    return rc, _lib.lib().colnde_last_error().decode(), h


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure")
def test_create_ensemble_without_gpu_fails_loudly():
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1e2)
    rc, msg, h = _create(p.cfg, 8, 4)
    assert rc != 0 and not h.value
    assert "no HIP device" in msg and "no CPU fallback" in msg
    with pytest.raises(colnde.ColndeError, match="no HIP device"):
        colnde.ColumnNDEEnsemble(p.cfg, 8, 4)


def test_configuration_refusals_name_their_reason_before_any_device_work():
    """These are decided from the configuration alone (no GPU needed): each names why."""
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1e2)
    ph = np.tile(np.array([[1e-4, 0.1, 1.0, 0.25, 1.0]], np.float32), (3, 1))
    cases = [
        (p.cfg.with_(substeps=0), None, "substeps = 0"),
        (p.cfg.with_(inplace_variant=True), None, "inplace_variant"),
        (p.cfg.with_(modified_pacanowski_philander=False, zero_weights=False), ph, "modified_pacanowski_philander = 1"),
        (synthetic.free_convection_problem(8, n_save=3).cfg, None, "free-convection"),
    ]
    for cfg, physics, what in cases:
        rc, msg, h = _create(cfg, 8, 3, physics)
        assert rc != 0 and not h.value and what in msg, (what, msg)
    rc, msg, _ = _create(p.cfg, 8193, 2)
    assert rc != 0 and "8,192 columns" in msg
    rc, msg, _ = _create(p.cfg, 8, 0)
    assert rc != 0 and "n_models" in msg
    unstable = ph.copy()
    unstable[1, 1] = 100.0                                         # nu_minus of model 1: far outside the shared step's stability bound
    rc, msg, _ = _create(p.cfg, 8, 3, unstable)
    assert rc != 0 and "model 1" in msg and "substeps" in msg


def test_python_side_checks_per_model_shapes():
    check_ensemble_arrays(3, 10, np.zeros((3, 10)), np.zeros((3, 5)), np.zeros(3))
    with pytest.raises(ValueError, match="weights"):
        check_ensemble_arrays(3, 10, weights=np.zeros((2, 10)))
    with pytest.raises(ValueError, match="weights"):
        check_ensemble_arrays(3, 10, weights=np.zeros((3, 9)))
    with pytest.raises(ValueError, match="physics"):
        check_ensemble_arrays(3, 10, physics=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="etas"):
        check_ensemble_arrays(3, 10, etas=np.zeros((3, 1)))
    p = synthetic.wind_mixing_problem(8, n_frames=3, weight_divisor=1e2)
    with pytest.raises(ValueError, match="physics"):               # refused before the library is asked for a handle
        colnde.ColumnNDEEnsemble(p.cfg, 8, 3, physics=np.zeros((2, 5), np.float32))
    from colnde.wind_mixing import train_NDE_ensemble

    class _Problem:                                                # the shapes are checked before the problem's handle is touched
        cfg = p.cfg
    W = np.zeros((3, p.cfg.n_params), np.float32)
    with pytest.raises(ValueError, match="etas"):
        train_NDE_ensemble(_Problem(), W, None, np.full(2, 1e-3))
    with pytest.raises(ValueError, match="physics"):
        train_NDE_ensemble(_Problem(), W, np.zeros((3, 6)), np.full(3, 1e-3))
    with pytest.raises(ValueError, match="weights"):
        train_NDE_ensemble(_Problem(), W[:, :5], None, np.full(3, 1e-3))
