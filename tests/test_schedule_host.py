"""The step schedule on the host (no GPU): the four entry points of include/colnde.h agree with the ctypes binding and the Julia wrappers;
colnde_schedule_min is colnde_min_substeps interval by interval; csrc/step_schedule.h — the totals, tape offsets and tape sizes every launch
and allocation takes — compiled alone and held to a Python restatement; distributed.agree_schedule; and the float64 reference the GPU tests
use (the oracle with `_step_times` replaced) is the oracle itself on an all-equal schedule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import colnde
from colnde import _lib
from colnde.distributed import agree_schedule
from oracle import nde_oracle as O
from tests import schedule_common as C
from tests.test_abi import _header_prototypes
from tests.test_distributed_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"colnde_schedule_min": 2, "colnde_set_schedule": 2, "colnde_schedule": 2, "colnde_choose_schedule": 5}


def test_the_four_entry_points_in_header_library_ctypes_and_julia():
    L = _lib.lib()
    protos = _header_prototypes()
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    jl = open(os.path.join(ROOT, "julia", "ColumnNDE.jl")).read()
    for name, arity in ENTRY_POINTS.items():
        assert protos[name] == arity, name
        assert hasattr(L, name) and len(bound[name]) == arity, name
        assert re.search(r"ccall\(\(:%s,\s*libcolnde\)" % name, jl), name      # (its arity: tests/test_abi.py checks every ccall of the file)
    header = open(os.path.join(ROOT, "include", "colnde.h")).read()
    assert "CLEAR the schedule" in header                                     # colnde_set_substeps on a handle with a schedule: the header says so
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all("`%s`" % name in table for name in ENTRY_POINTS)


def _two_point_minima(cfg):
    t = cfg.save_times
    return tuple(colnde.min_substeps(cfg.with_(save_times=(t[i], t[i + 1]))) for i in range(len(t) - 1))


def test_schedule_min_is_min_substeps_of_every_two_point_configuration():
    base = C.base_problem(1).cfg
    uneven = base.with_(save_times=C.UNEVEN)
    assert colnde.schedule_min(uneven) == _two_point_minima(uneven) == C.UNEVEN_MIN
    assert tuple(C.pow2_ceil(v) for v in C.UNEVEN_MIN) == C.UNEVEN_POW2 and sum(C.UNEVEN_POW2) == 32
    assert colnde.min_substeps(uneven) == 13                                   # one count follows the longest interval: 6 x 16 = 96 steps
    assert colnde.schedule_min(base) == _two_point_minima(base) == (2, 2, 2)
    default = colnde.synthetic.wind_mixing_problem(1, n_frames=9).cfg            # the default axis: k/288
    assert colnde.schedule_min(default) == _two_point_minima(default) == (2,) * 8
    half = uneven.with_(Pr=0.5)                                                # twice the temperature diffusivity: twice lambda
    assert colnde.schedule_min(half) == _two_point_minima(half)
    assert half != uneven and colnde.schedule_min(half) == (4, 4, 4, 4, 13, 25)
    c, keep = colnde.config.to_c_config(uneven.with_(stepper="rkc2"), 1, 0, 0)
    out = (ctypes.c_int * 6)()
    assert _lib.lib().colnde_schedule_min(ctypes.byref(c), out) != 0 and b"RK4 only" in _lib.lib().colnde_last_error()


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "schedule_check.cpp"),
                           "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out
    return run


SCHEDULES = [(1, 1, 1), (1,) * 6, (4, 4, 4), (16,) * 6, (8, 2, 4), (2, 2, 8), C.UNEVEN_POW2, (2, 4096, 2), (4096,) * 96]


def test_totals_offsets_and_tape_sizes_are_the_restatement(header):
    """Tapes, slab rows and dW record counts are sized by the total, and the kernels index them by the running step counter: a wrong total or offset
    is an out-of-bounds tape write.  Restated: total = sum, offset(iv) = sum of the counts before iv, records = tiles x total x stages."""
    got = header([("T", len(s), 3) + s for s in SCHEDULES])
    for s, g in zip(SCHEDULES, got):
        assert g[0] == sum(s) and g[1] == 3 * len(s), s
        assert g[2:] == tuple(sum(s[:i]) for i in range(len(s) + 1)), s          # where each interval's steps begin; the last: the total
        if len(set(s)) == 1:
            assert g[0] == len(s) * s[0]                                        # all-equal: the total of substeps = c
    # the records of the net-split pair's tapes (floats per (tile, step, stage): stage inputs 16 x 96, pre-activations 16 x 216, rich 13,824, dW 16 x 720)
    cases = [(tiles, 4, rec, s) for tiles in (1, 3, 512) for rec in (1536, 3456, 13824, 11520) for s in SCHEDULES]
    got = header([("R", t, nst, rec, len(s)) + s for t, nst, rec, s in cases])
    for (t, nst, rec, s), g in zip(cases, got):
        assert g == (t * sum(s) * nst, t * sum(s) * nst * rec), (t, rec, s)
    assert max(g[1] for g in got) * 4 > 2 ** 40                                 # (sizes past 32 bits are computed in size_t)
    assert header([("P", v) for v in (1, 2, 3, 7, 13, 16, 17, 4095, 4096)]) == [(1,), (2,), (4,), (8,), (16,), (16,), (32,), (4096,), (4096,)]
    lam, bound = 4 * 172800 * 0.1001 / 256 ** 2 * 32 ** 2, 2.785
    spans = [k / 256.0 for k in (0.25, 0.5, 1, 4, 8)] + [0.0, 1e-9]
    assert header([("M", repr(sp), repr(lam), bound) for sp in spans]) == [(max(1, int(np.ceil(sp * lam / bound))),) for sp in spans]


def test_validation_order_and_verdicts(header):
    OK, NOT_POSITIVE, ABOVE_MAX, BELOW_MIN = range(4)
    m = (2, 2, 8)
    cases = [((2, 2, 8), 0, (OK, -1)), ((8, 2, 8), 0, (OK, -1)), ((2, 1, 8), 0, (BELOW_MIN, 1)), ((2, 1, 8), 1, (OK, -1)), ((2, 2, 0), 0, (NOT_POSITIVE, 2)),
             ((2, 2, 0), 1, (NOT_POSITIVE, 2)), ((-1, 2, 8), 0, (NOT_POSITIVE, 0)), ((4096, 2, 8), 0, (OK, -1)), ((4097, 2, 8), 0, (ABOVE_MAX, 0)),
             ((2, 2, 4097), 1, (ABOVE_MAX, 2)), ((1, 0, 9000), 0, (BELOW_MIN, 0))]
    assert header([("V", allow, 3) + c + m for c, allow, _ in cases]) == [v for _, _, v in cases]


def _agree_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = agree_schedule(((2, 2, 16, 4), (2, 8, 4, 4))[rank])
    np.save(os.path.join(out_dir, "sched%d.npy" % rank), np.array(got))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_agree_on_the_elementwise_maximum(tmp_path):
    world = 2
    mp.spawn(_agree_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert np.load(tmp_path / ("sched%d.npy" % r)).tolist() == [2, 8, 16, 4]


@pytest.mark.parametrize("c", [2, 4])
def test_the_patched_oracle_on_an_all_equal_schedule_is_the_oracle(c, monkeypatch):
    p = C.base_problem(3, substeps=c)
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth)
    ref = O.loss_and_grad(p.cfg, p.x0, p.bcs, p.weights, truth.astype(np.float32), np.array(C.SC, np.float64))
    C.oracle_schedule(monkeypatch, (c, c, c))
    other = p.cfg.with_(substeps=1)                     # the patched oracle reads the schedule, not cfg.substeps
    assert np.array_equal(O.solve(other, p.x0, p.bcs, p.weights_truth), truth)
    got = O.loss_and_grad(other, p.x0, p.bcs, p.weights, truth.astype(np.float32), np.array(C.SC, np.float64))
    assert got[0] == ref[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:]))
