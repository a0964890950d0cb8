"""The ensemble's error estimate and schedule choice on the host (no GPU): csrc/step_schedule.h's `sched_choose_round` — the decision rule as a pure
function — compiled alone under AddressSanitizer and UBSan and held to a NumPy restatement over drawn rounds; the three entry points in header,
library, ctypes and Julia; and the float64 expectation of the K = 3 case the GPU test uses, with its distance from the rule's thresholds."""
import os
import re
import subprocess

import numpy as np
import pytest

import colnde
from colnde import _lib
from tests import ens_schedule_cases as E
from tests import schedule_common as C
from tests.test_abi import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"colnde_ensemble_error_estimate_dev": 3, "colnde_ensemble_error_estimate": 3, "colnde_ensemble_choose_schedule": 5}
F = np.float32


@pytest.fixture(scope="module")
def choose_round(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ens_schedule") / "ens_schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g",
                           os.path.join(ROOT, "tests", "ens_schedule_check.cpp"), "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])
    bits = lambda v: int(np.asarray(v, F).view(np.uint32))

    def run(cases):
        """cases: (E, reltol, prev_est, S) -> [(verdict, est, S)]"""
        text = "".join(" ".join(str(v) for v in [len(e), bits(r), bits(p)] + [bits(x) for x in e] + list(s)) + "\n" for e, r, p, s in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = []
        for ln in r.stdout.splitlines():
            v = [int(x) for x in ln.split()]
            out.append((v[0], float(np.array(v[1], np.uint32).view(F)), v[2:]))
        assert len(out) == len(cases)
        return out
    return run


def _draw(rng, n_save):
    """one round: (E, reltol, prev_est, S).  The additions d are small multiples of 2^-16, so E is exact in float32 and d = dmax / 2 is a true tie."""
    n_iv = n_save - 1
    reltol = float(F(rng.choice([1e-3, 1e-4, 2.0 ** -10])))
    kind = rng.integers(8)
    d = rng.integers(0, 64, n_iv).astype(np.float64)
    if kind == 0:                                            # met: everything below reltol
        d = rng.integers(0, 3, n_iv).astype(np.float64) * (2.0 ** -6)
    if kind == 1 and n_iv > 1:                               # ties: the largest addition is even and another one is exactly its half
        i, j = rng.choice(n_iv, 2, replace=False)
        d[i] = 2 * rng.integers(8, 32)
        d = np.minimum(d, d[i])
        d[j] = d[i] / 2
    E = np.concatenate([[0.0], np.cumsum(d)]) * 2.0 ** -16
    if kind == 2 and n_iv > 1:                               # a damped stretch: E falls, the addition is clamped at 0
        k = rng.integers(1, n_save)
        E[k:] -= min(E[k], rng.integers(0, 64) * 2.0 ** -16)
    E = E.astype(F)
    if kind == 3:                                            # a solve that is not finite
        E[rng.integers(n_save)] = rng.choice([np.nan, np.inf, F(3.3e38)])
    S = [int(2 ** rng.integers(0, 13)) for _ in range(n_iv)]
    if kind == 4:
        S = [4096] * n_iv                                    # nothing left to double
    if kind == 5:
        S = [4096 if dv >= 0.5 * d.max() else s for dv, s in zip(d, S)]      # the intervals that carry the error are at the cap
    est = float(np.nanmax(E))
    # the 0.8 rule from both sides (0.8f * prev is rounded: one ulp either way is on a known side), and no previous round
    prev = float(rng.choice([-1.0, 0.0, est / 0.8 * (1 + 2e-6), est / 0.8 * (1 - 2e-6), est / 0.5, est / 0.95])) if est < 1e30 else -1.0
    return E, reltol, prev, S


def test_sched_choose_round_is_the_numpy_restatement(choose_round):
    rng = np.random.default_rng(20240607)
    cases = [_draw(rng, n_save) for n_save in (2, 7) for _ in range(520)]
    # by hand: each verdict once whatever the draws give, and the rule's corners
    h = 2.0 ** -10
    cases += [(F([0, h, 2 * h]), h, -1.0, [2, 2]),                      # est = 2h > reltol, d = (h, h): both doubled
              (F([0, h, h]), 2 * h, -1.0, [2, 2]),                      # met
              (F([0, h]), h, -1.0, [1]),                                # est == reltol: met
              (F([0, 4 * h, 6 * h]), h, -1.0, [4096, 8]),               # tie at dmax / 2 with the larger at the cap: the tie alone is doubled
              (F([0, 4 * h, 6 * h]), h, 7 * h, [8, 8]),                 # 6h > 0.8 x 7h: floor
              (F([0, 4 * h, 6 * h]), h, 8 * h, [8, 8]),                 # 6h <= 0.8 x 8h = 6.4h: goes on
              (F([0, 4 * h, 4 * h]), h, -1.0, [4096, 2]),               # the carrier at the cap, the other adds nothing... and 0 >= dmax / 2 is false
              (F([0, np.nan, h]), h, -1.0, [2, 2]), (F([np.inf, 0, h]), h, -1.0, [2, 2])]
    got = choose_round(cases)
    seen = set()
    for (Ev, reltol, prev, S), (verdict, est, S_out) in zip(cases, got):
        want = E.choose_round(Ev, reltol, prev, S)
        assert verdict == want[0] and S_out == want[2], (Ev, reltol, prev, S, verdict, want)
        assert est == want[1] or (np.isnan(est) and np.isnan(want[1])), (Ev, est, want[1])
        if verdict == E.NOT_FINITE:
            assert S_out == list(S)
        if verdict == E.DOUBLED:
            assert S_out != list(S) and all(b in (a, 2 * a) and b <= E.SCHEDULE_MAX for a, b in zip(S, S_out))
        seen.add(verdict)
    assert seen == {E.MET, E.DOUBLED, E.NOT_FINITE, E.FLOOR, E.TOO_STIFF}
    by_hand = [g[0] for g in got[-9:]]
    assert by_hand == [E.DOUBLED, E.MET, E.MET, E.DOUBLED, E.FLOOR, E.DOUBLED, E.TOO_STIFF, E.NOT_FINITE, E.NOT_FINITE]
    assert got[-9][2] == [4, 4] and got[-6][2] == [4096, 16] and got[-4][2] == [16, 16]
    # the draws themselves covered what they were drawn for
    drawn = list(zip(cases[:1040], got[:1040]))
    assert any(len(c[0]) == 2 for c, _ in drawn) and any(len(c[0]) == 7 for c, _ in drawn)
    assert any(np.isnan(c[0]).any() for c, _ in drawn) and any(np.isinf(c[0]).any() for c, _ in drawn)
    assert any(all(s == 4096 for s in c[3]) and g[0] == E.TOO_STIFF for c, g in drawn)
    assert any(c[2] > 0 and g[0] == E.FLOOR for c, g in drawn) and any(c[2] > 0 and g[0] == E.DOUBLED for c, g in drawn)
    ties = 0
    for (Ev, _, _, S), g in drawn:
        d = np.maximum(F(0), np.diff(Ev)) if np.isfinite(Ev).all() else None
        if d is not None and g[0] == E.DOUBLED and len(d) > 1 and (d == F(0.5) * d.max()).any():
            ties += 1
    assert ties >= 10, ties


def test_the_three_entry_points_in_header_library_ctypes_and_julia():
    L = _lib.lib()
    protos = _header_prototypes()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in ENTRY_POINTS.items():
        assert protos[name] == arity, name
        assert hasattr(L, name) and len(bound[name]) == arity, name
        assert re.search(r"ccall\(\(:%s,\s*libcolnde\)" % name, jl), name       # (its arity: tests/test_abi.py checks every ccall of the file)
    header = open(os.path.join(ROOT, "include", "colnde.h")).read()
    assert L.colnde_version() == int(re.search(r"#define COLNDE_VERSION (\d+)", header).group(1)) == 106
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s`" % name in table for name in ENTRY_POINTS)
    for method in ("ensemble_error_estimate", "choose_ensemble_schedule"):
        assert callable(getattr(colnde.ColumnNDEEnsemble, method))
    # a null handle is refused by name, before anything else is read
    for name in ENTRY_POINTS:
        args = [None] * ENTRY_POINTS[name]
        if name == "colnde_ensemble_choose_schedule":
            args[2] = 0.0
        assert getattr(L, name)(*args) != 0 and (name + ": null handle").encode() in L.colnde_last_error()


def test_the_k3_case_in_float64_stays_clear_of_the_thresholds(monkeypatch):
    """The greedy run on the float64 oracle, max over the members: the expectation written into tests/ens_schedule_cases.py, and — the condition the
    GPU comparison rests on — every round at least 5 % away from reltol and from the tie at half the largest addition."""
    p, W = E.problem_k3()
    assert W.shape == (3, p.cfg.n_params) and not np.array_equal(W[0], W[1]) and not np.array_equal(W[1], W[2])
    assert len({tuple(r) for r in E.PHYS_K3.T.tolist()}) == 5 and all(len(set(c)) > 1 for c in E.PHYS_K3.T.tolist())
    minima = np.max([colnde.schedule_min(c) for c in E.member_cfgs(p.cfg, E.PHYS_K3)], axis=0)
    start = tuple(C.pow2_ceil(int(v)) for v in minima)
    assert start == E.MINIMA_POW2_F64
    verdict, S, member_est, rounds = E.greedy(E.oracle_estimates(monkeypatch, p, W, E.PHYS_K3), start, E.RELTOL)
    for r in rounds:
        print("float64 round: S = %r, est = %.4e, |est - reltol| / reltol = %.3f, nearest addition to dmax / 2: %.3f" % r)
    assert E.clear_of_thresholds(rounds), rounds
    assert verdict == E.MET and S == E.SCHEDULE_F64 and len(rounds) == E.ROUNDS_F64
    assert member_est.max() <= E.RELTOL and int(np.argmax(member_est)) == 0          # the most viscous member drives the schedule
    assert sum(S) < 6 * 16                                                       # one count for all needs at least the longest interval's 16
