"""CPU-side checks of the conv ensemble (colnde_create_conv_ensemble: K `--conv c` networks side by side on the 16-column fc32 kernels): declared,
exported, bound in ctypes and in the Julia module with four arguments; every refusal decided from the configuration and the environment — the union
of colnde_create_conv's and colnde_create_fc_ensemble's — names its reason before any device work; without a GPU a valid configuration fails
loudly; the Python front ends check the conv shapes before the library is asked for a handle; the planner's per-model bytes (csrc/tape_plan.h),
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
from colnde.free_convection import (compute_nde_solution_history, conv_n_params, nde_loss_history, train_neural_differential_equation_ensemble)
from colnde.nde import ENGINE_FC32, ENGINE_REGTILE, ENGINE_TILE16, check_fc_ensemble_arrays, fc_ensemble_n_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "colnde_create_conv_ensemble"


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _create(cfg, n_col, c, K, engine=0):
    cc, keep = to_c_config(cfg, n_col, 0, engine)
    h = ctypes.c_void_p()
    rc = _lib.lib().colnde_create_conv_ensemble(ctypes.byref(cc), c, K, ctypes.byref(h))
    return rc, _lib.lib().colnde_last_error().decode(), h


def _fc(n=8, **kw):
    return synthetic.free_convection_problem(n, n_save=3, **kw).cfg


def test_symbol_declared_exported_and_bound_with_four_arguments():
    text = open(os.path.join(ROOT, "include", "colnde.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % NAME, header, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 4, m
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert NAME in bound and len(bound[NAME]) == 4 and hasattr(_lib.lib(), NAME)
    assert "#define COLNDE_VERSION 106" in text                                                # additive: the version stays
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    m = re.search(r"ccall\(\(:%s,\s*libcolnde\),\s*Cint,\s*\(([^)]*)\)" % NAME, jl)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 4, m


def test_configuration_refusals_name_their_reason_before_any_device_work():
    """Decided from the configuration alone (this machine may have no GPU): each names why, and the handle stays NULL."""
    cases = [
        (_fc(), 8, 1, 3, 0, "conv_filter = 1 outside 2..8"),
        (_fc(), 8, 0, 3, 0, "conv_filter = 0 outside 2..8"),
        (_fc(), 8, 9, 3, 0, "conv_filter = 9 outside 2..8"),
        (_fc(), 8, -2, 3, 0, "conv_filter = -2 outside 2..8"),
        (synthetic.wind_mixing_problem(8, n_frames=3).cfg, 8, 3, 3, 0, "wind-mixing"),
        (_fc(layer_sizes=(32, 48, 40, 31)), 8, 3, 3, 0, "plain fc32 configuration"),               # another network
        (synthetic.free_convection_problem(8, Nz=16, n_save=3).cfg, 8, 3, 3, 0, "Nz = 16"),        # another Nz
        (_fc(), 8, 3, 3, ENGINE_TILE16, "engine"),
        (_fc(), 8, 3, 3, ENGINE_REGTILE, "engine"),
        (_fc().with_(stepper="rkc2"), 8, 3, 3, 0, "FreeConvectionNDE under RKC2"),
        (_fc().with_(substeps=0), 8, 3, 3, 0, "substeps = 0"),
        (_fc(convective_adjustment=True, substeps=2), 8, 3, 3, 0, "colnde_min_substeps"),         # K = 10: far outside RK4's region at two sub-steps
        (_fc(), 8, 3, 0, 0, "n_models = 0 outside 1..65535"),
        (_fc(), 8, 3, -1, 0, "n_models = -1 outside 1..65535"),
        (_fc(), 8, 3, 65536, 0, "n_models = 65536 outside 1..65535"),
        (_fc(), 4097, 3, 3, 0, "4,096 columns"),
    ]
    for cfg, n_col, c, K, engine, what in cases:
        rc, msg, h = _create(cfg, n_col, c, K, engine)
        assert rc != 0 and not h.value and what in msg, (what, msg)
        assert "no HIP device" not in msg, msg
    assert colnde.min_substeps(_fc(convective_adjustment=True, substeps=2)) > 2
    h = ctypes.c_void_p(1)
    cc, keep = to_c_config(_fc(), 8, 0, 0)
    assert _lib.lib().colnde_create_conv_ensemble(ctypes.byref(cc), 0, 3, ctypes.byref(h)) != 0 and not h.value      # a refused creator leaves NULL
    assert _lib.lib().colnde_create_conv_ensemble(ctypes.byref(cc), 3, 3, None) != 0
    assert "null out pointer" in _lib.lib().colnde_last_error().decode()


@pytest.mark.parametrize("name,value", [("COLNDE_FC", "0"), ("COLNDE_FC_CW", "32"), ("COLNDE_FC_BLOCK", "32")])
def test_switches_that_leave_the_16_column_kernels_are_refused(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    rc, msg, h = _create(_fc(), 8, 3, 3)
    assert rc != 0 and not h.value and name in msg and "no HIP device" not in msg, msg


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure")
@pytest.mark.parametrize("engine", [0, ENGINE_FC32])
def test_valid_configuration_without_gpu_fails_only_for_the_missing_device(engine):
    for cfg, c, K in ((_fc(), 2, 1), (_fc(), 8, 3), (_fc(Nz=64), 5, 65535), (_fc(convective_adjustment=True, substeps=40, t_end=0.01), 3, 4),
                      (_fc(convective_adjustment=True, substeps=2, t_end=0.01).with_(stepper="rkc2"), 3, 4)):
        rc, msg, h = _create(cfg, 8, c, K, engine)
        assert rc != 0 and not h.value
        assert re.search("no HIP device|no CPU fallback", msg), msg
    with pytest.raises(colnde.ColndeError, match="no HIP device|no CPU fallback"):
        colnde.FreeConvectionEnsemble(_fc(), 8, 4, conv=3)


def test_python_shape_rules_with_conv(monkeypatch):
    cfg = _fc()
    c, K, n = 3, 3, 8
    P = conv_n_params(32, c)
    assert fc_ensemble_n_params(cfg, c) == P == c + 1 + cfg.n_params - 128 * (c - 1) and fc_ensemble_n_params(cfg) == cfg.n_params
    assert fc_ensemble_n_params(_fc(Nz=64), 8) == conv_n_params(64, 8)
    check_fc_ensemble_arrays(cfg, n, K, np.zeros((K, P)), np.zeros(K), np.zeros(K), np.zeros((K, n, 3, 32)), np.zeros((K, P + 8)), conv=c)
    for kw, what in ((dict(weights=np.zeros((K, cfg.n_params))), "weights"), (dict(weights=np.zeros((2, P))), "weights"),
                     (dict(result=np.zeros((K, cfg.n_params + 8))), "result"), (dict(result=np.zeros((K, P))), "result"),
                     (dict(etas=np.zeros((K, 1))), "etas"), (dict(coeff=np.zeros(K + 1)), "coeff"), (dict(sol=np.zeros((K, n, 3, 31))), "sol")):
        with pytest.raises(ValueError, match=what):
            check_fc_ensemble_arrays(cfg, n, K, conv=c, **kw)
    with pytest.raises(ValueError, match="weights"):
        check_fc_ensemble_arrays(cfg, n, K, weights=np.zeros((K, P)))                      # the conv count is not the plain network's
    for bad in (1, 9, -3):
        with pytest.raises(ValueError, match="conv = %d outside 2..8" % bad):
            check_fc_ensemble_arrays(cfg, n, K, conv=bad)

    # from here on a request for a handle is an error of the test: the checks must come first
    def no_handle(*a):
        raise AssertionError("the library was asked for a handle")
    monkeypatch.setattr(_lib.lib(), "colnde_create_conv_ensemble", no_handle, raising=False)
    monkeypatch.setattr(_lib.lib(), "colnde_create_fc_ensemble", no_handle, raising=False)
    with pytest.raises(ValueError, match="conv = 9"):
        colnde.FreeConvectionEnsemble(cfg, n, K, conv=9)
    with pytest.raises(ValueError, match="n_columns"):
        colnde.FreeConvectionEnsemble(cfg, 4097, K, conv=c)
    p = synthetic.free_convection_problem(n, n_save=3)
    W = np.zeros((K, P), np.float32)
    truth = np.zeros((n, 3, 32), np.float32)
    with pytest.raises(ValueError, match="weights"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, np.zeros((K, cfg.n_params), np.float32), np.full(K, 1e-3), 1, conv=c)
    with pytest.raises(ValueError, match="etas"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W, np.full(2, 1e-3), 1, conv=c)
    with pytest.raises(ValueError, match="coeff"):
        train_neural_differential_equation_ensemble(p.x0, p.bcs, truth, cfg, W, np.full(K, 1e-3), 1, causal_coeff=np.zeros(K + 1), conv=c)
    with pytest.raises(ValueError, match="weights"):
        compute_nde_solution_history(p.x0, p.bcs, cfg, W, conv=4)
    with pytest.raises(ValueError, match="weights"):
        nde_loss_history(p.x0, p.bcs, truth, cfg, W)                                         # conv left at its default: the plain count
    with pytest.raises(ValueError, match="true_sols"):
        nde_loss_history(p.x0, p.bcs, truth[:, :2], cfg, W, conv=c)


# ---- the planner's arithmetic (csrc/tape_plan.h) as a stand-alone sanitized program ------------------------------------------------------------------
CSLAB_SEG = 256 * 9                                       # FC_CONV_GRAD_MAX_SLICES x FC_CONV_GRAD_SLOTS floats per time segment


def _model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab):
    """NumPy restatement: tapes of `seg` intervals (per_col_iv holds the conv tape's bytes), the slab rows [tile][segment] + [segment][512 slices],
    lambda between segments — what a plain ensemble's model owns — plus the filter slab per segment and the padded weight and gradient vectors."""
    nsg = -(-n_iv // seg)
    plain = per_col_iv * n32 * seg + (n32 // cw + 512) * nsg * (n_params + 8) * 4 + n32 * Nz * 4
    return int(plain + (nsg * cslab + 2 * n_params + 8) * 4)


def _seg(n32, n_iv, cw, Nz, per_col_iv, budget, n_params, cslab):
    seg = n_iv
    while seg > 1 and _model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab) > budget:
        seg -= 1
    return seg


def _per_col_iv(Nz, substeps, nst, ca, conv):
    R = 18 * Nz                                                  # (about the record's row length; the conv tape's term is what is under test)
    return substeps * nst * (R * 4 + 512 * 4 // 16 + (8 if ca else 0) + (16 * 2 * Nz // 16 * 4 if conv else 0))


@pytest.fixture(scope="module")
def conv_planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_ens_plan") / "conv_ens_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "conv_ens_plan_check.cpp"), "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, r.stderr
        out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def test_per_model_bytes_with_the_conv_tape_against_numpy(conv_planner):
    shapes = [(32, 4, 32, 24735), (32, 128, 64, 98623), (4096, 8, 32, 24735), (4096, 128, 64, 98623)]
    m_cases, s_cases = [], []
    for n32, n_iv, Nz, n_params in shapes:
        for ca in (False, True):
            p_conv, p_plain = _per_col_iv(Nz, 2, 4, ca, True), _per_col_iv(Nz, 2, 4, ca, False)
            assert p_conv - p_plain == 2 * 4 * 2 * Nz * 4                                # the conv tape: [x | z-bar] per column, stage and step
            for seg in sorted({1, 2, 3, n_iv // 2, n_iv - 1, n_iv} - {0}):
                m_cases.append(("M", n32, n_iv, 16, Nz, p_conv, n_params, seg, CSLAB_SEG))
            whole = _model_bytes(n32, n_iv, 16, Nz, p_conv, n_params, n_iv, CSLAB_SEG)
            one = _model_bytes(n32, n_iv, 16, Nz, p_conv, n_params, 1, CSLAB_SEG)
            for budget in sorted({0, 1, one - 1, one, one + 1, whole - 1, whole, whole + 1, 2 * whole} | {int(whole * f) for f in (0.05, 0.2, 0.5, 0.9)}):
                s_cases.append(("S", n32, n_iv, 16, Nz, p_conv, budget, n_params, CSLAB_SEG))
    got = conv_planner(m_cases)
    for case, (b,) in zip(m_cases, got):
        assert b == _model_bytes(*case[1:]), case
        n32, n_iv, cw, Nz, p, n_params, seg, cslab = case[1:]
        nsg = -(-n_iv // seg)
        plain = p * n32 * seg + (n32 // cw + 512) * nsg * (n_params + 8) * 4 + n32 * Nz * 4
        assert b - plain == (nsg * cslab + 2 * n_params + 8) * 4                          # the filter slab and the two padded vectors
    got = conv_planner(s_cases)
    kinds = set()
    for case, (seg, b) in zip(s_cases, got):
        n32, n_iv, cw, Nz, p, budget, n_params, cslab = case[1:]
        assert seg == _seg(*case[1:]) and b == _model_bytes(n32, n_iv, cw, Nz, p, n_params, seg, cslab), case
        assert 1 <= seg <= n_iv
        fits = b <= budget
        if seg > 1:
            assert fits, case                                                             # a plan above one interval always fits its budget
        if seg < n_iv:
            assert _model_bytes(n32, n_iv, cw, Nz, p, n_params, seg + 1, cslab) > budget    # ... and is the largest that does
        kinds.add("whole" if seg == n_iv and fits else "segments" if fits else "nothing fits")
    assert kinds == {"whole", "segments", "nothing fits"}                                 # a budget that forces segments and one that fits nothing
