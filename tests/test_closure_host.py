"""CPU-side checks of the closure-only model (colnde_create_closure and friends): the boundary is complete (declared = exported = bound =
ccalled), the stability bound follows its formula, the array checker rejects what the kernels could not read, and the float64 yardstick the GPU
gradient is held to — the central finite difference of `O.loss(O.solve(...))` — agrees with torch-float64 autograd through the literal restatement."""
import ctypes
import dataclasses
import os
import re
import types

import numpy as np
import pytest

import colnde
from colnde import _lib
from colnde.config import to_c_config

from tests import closure_common as C
from tests.test_abi import _declared_symbols, _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"colnde_closure_min_substeps": 2, "colnde_create_closure": 3, "colnde_closure_forward_dev": 3, "colnde_closure_loss_dev": 4,
       "colnde_closure_loss_grad_dev": 4, "colnde_closure_forward": 3, "colnde_closure_loss_grad": 4}


def test_closure_symbols_are_declared_exported_bound_and_ccalled():
    L = _lib.lib()
    declared, protos = _declared_symbols(), _header_prototypes()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in NEW.items():
        assert name in declared and protos[name] == arity, name
        assert hasattr(L, name), "%s not exported" % name
        assert len(bound[name]) == arity, name
        m = re.search(r"ccall\(\(:%s,\s*libcolnde\),\s*\w+,\s*\(([^()]*)\)" % name, jl)
        assert m, "%s is not ccalled in julia/ColumnNDE.jl" % name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    assert L.colnde_version() == 106


def _formula(cfg, params):
    nu0, num, dRi, Ric, Pr = params
    lam = 4 * cfg.tau * (nu0 + num) * max(1.0, 1.0 / Pr) / cfg.H ** 2 * cfg.Nz ** 2
    span = float(np.max(np.diff(cfg.save_times)))
    return max(1, int(np.ceil(lam * span / 2.785)))


def test_closure_min_substeps_follows_the_formula():
    cfg = C.closure_problem(1, n_frames=3)[0].cfg
    default = (1e-4, 1e-1, 0.1, 0.25, 1.0)
    assert colnde.closure_min_substeps(cfg, default) == _formula(cfg, default) == 2
    half = (1e-4, 1e-1, 0.1, 0.25, 0.5)                      # Pr = 0.5: max(1, 1/Pr) doubles the stiffest diffusivity, lambda dt / 2.785 = 1.39 -> 2.78
    assert colnde.closure_min_substeps(cfg, half) == _formula(cfg, half) == 3
    quarter = (1e-4, 1e-1, 0.1, 0.25, 0.25)
    assert colnde.closure_min_substeps(cfg, quarter) == _formula(cfg, quarter) == 6
    # the five constants of the call count, not cfg's own
    assert colnde.closure_min_substeps(cfg.with_(nu_minus=10.0), default) == 2
    L = _lib.lib()
    c, keep = to_c_config(cfg, 1, 0, 0)
    for bad in ((1e-4, 1e-1, 0.0, 0.25, 1.0), (1e-4, 1e-1, 0.1, 0.25, 0.0), (1e-4, 1e-1, 0.1, 0.25, -1.0)):
        assert L.colnde_closure_min_substeps(ctypes.byref(c), (ctypes.c_float * 5)(*bad)) == -1
        assert b"must be > 0" in L.colnde_last_error()
    with pytest.raises(colnde.ColndeError):
        colnde.closure_min_substeps(cfg, (1e-4, 1e-1, 0.0, 0.25, 1.0))


def test_closure_create_refuses_without_a_gpu_or_with_a_refused_configuration():
    import torch
    cfg = C.closure_problem(1, n_frames=3)[0].cfg
    L = _lib.lib()
    h = ctypes.c_void_p()
    c, keep = to_c_config(cfg, 1, 0, 0)
    c.smooth_Ri = 1                                           # refused before any device is looked for
    assert L.colnde_create_closure(ctypes.byref(c), 1, ctypes.byref(h)) != 0
    assert b"smooth_Ri" in L.colnde_last_error()
    if not torch.cuda.is_available():
        with pytest.raises(colnde.ColndeError, match="no HIP device|no CPU fallback"):
            colnde.ClosureColumns(cfg, 1)


def test_closure_array_checker():
    import torch
    ok = np.ones((3, 5), np.float32)
    colnde.check_closure_arrays(3, params=ok, out=np.zeros((3, 13), np.float32))
    with pytest.raises(ValueError, match=r"\(3, 5\)"):
        colnde.check_closure_arrays(3, params=np.ones((3, 4), np.float32))       # [K][4]
    with pytest.raises(ValueError, match="3 sets"):
        colnde.check_closure_arrays(3, params=np.ones((2, 5), np.float32))       # wrong K
    with pytest.raises(ValueError, match="n_sets"):
        colnde.check_closure_arrays(0)
    with pytest.raises(ValueError, match="float32 device tensor"):
        colnde.check_closure_arrays(3, params=torch.ones((3, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="float32 device tensor"):
        colnde.check_closure_arrays(3, params=torch.ones((3, 5), dtype=torch.float32))   # float32, but not on a device
    with pytest.raises(ValueError, match=r"\(3, 13\)"):
        colnde.check_closure_arrays(3, out=np.zeros((3, 8), np.float32))


def test_finite_difference_yardstick_agrees_with_float64_autograd():
    """3 columns, Nz = 32, 5 frames, 2 sub-steps, theta = 0, truth from TRUTH: d(loss)/d(constants) at the configuration's own constants by the central
    difference of the oracle (relative step 1e-6) against torch-float64 autograd through tests/literal_torch.py; 1e-6 relative per component."""
    import torch
    from tests import literal_torch as LT
    p, theta0, truth = C.closure_problem(3)
    cfg = p.cfg
    sc = np.array([1, 1, 1, 5e-3, 5e-3, 5e-3])
    at = C.cfg_params(cfg)
    g_fd = C.fd_grad(cfg, p, truth, at, sc)
    ns = types.SimpleNamespace(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg)})
    consts = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in at]
    for k, t in zip(C.KEYS, consts):
        setattr(ns, k, t)
    theta = torch.zeros(cfg.n_params, dtype=torch.float64)
    sols = [LT.solve_rk4(ns, torch.tensor(p.x0[i], dtype=torch.float64), torch.tensor(p.bcs[i], dtype=torch.float64), theta) for i in range(3)]
    truths = [torch.tensor(truth[i], dtype=torch.float64) for i in range(3)]
    total = LT.total_loss(ns, sols, truths, [float(s) for s in sc])
    assert abs(float(total.detach()) / C.f64_loss(cfg, p, truth, at, sc)[0] - 1) < 1e-12
    g_ad = np.array([float(g) for g in torch.autograd.grad(total, consts)])
    assert (np.abs(g_ad * at) > 1e-6).all(), g_ad * at            # every component carries signal on this input
    np.testing.assert_allclose(g_fd, g_ad, rtol=1e-6, atol=0)
    np.testing.assert_allclose(C.fd_grad(cfg, p, truth, at, sc, rel=1e-4), g_fd, rtol=1e-6, atol=0)
