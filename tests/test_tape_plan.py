"""csrc/tape_plan.h on the host: the planners' arithmetic (columns per pass, fc32's column blocks or time segments) compiled alone with the host
compiler and held, value for value, to tests/tape_plan_restatement.py — the three formulas as they stood in api.hip — over grids that reach every
branch, the ones only a nearly full card takes included.  No GPU, no library."""
import os
import subprocess

import pytest

from tests import tape_plan_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = {"regtile": (1024, 1024, R.rt_block), "fc32": (32, 8192, R.fc_block), "tile16": (16, 4096, R.t16_block)}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tape_plan") / "tape_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "tape_plan_check.cpp"),
                           "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(cases):
        r = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def _block_grid(tile, granule):
    pad = 16 if tile == 16 else 32                       # what the planner pads the column count to
    ns = [32, 64, 96, 992, 1024, 1056, 4080, 4096, 4128, 8160, 8192, 8224, 10016, 16384, 16416, 20000, 65536, 100000, 262112, 262144]
    if pad == 16:
        ns += [48, 4112, 12304]
    for n in ns:
        fits = {0, 1, tile - 1, tile, tile + 1, n - 1, n, n + 1, 2 * n}
        for k in range(1, n // granule + 2):
            fits.update((k * granule - 1, k * granule, k * granule + 1))
        for d in (2, 3, 5, 7):                          # equal blocks just short of fitting
            fits.update((n // d - 1, n // d, n // d + tile))
        for fit in sorted(f for f in fits if f >= 0):
            yield n, fit


@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_column_blocks_are_the_three_formulas(planner, engine):
    tile, granule, formula = ENGINES[engine]
    grid = list(_block_grid(tile, granule))
    got = planner([("B", n, fit, tile, granule) for n, fit in grid])
    partial = 0
    for (n, fit), (block,) in zip(grid, got):
        assert block == formula(n, fit), (engine, n, fit)
        assert block == n or block % tile == 0, (engine, n, fit, block)
        if fit < n:
            assert block <= fit, (engine, n, fit, block)
        if block:
            assert block * ((n + block - 1) // block) >= n
            partial += block < n
        else:
            assert fit < tile
    assert partial > 100                                 # (the grid does cut problems into blocks)


def test_regtile_clamp_is_the_shared_decrement_loop(planner):
    """api.hip clamped regtile's block with `fit / 1024 * 1024` where the other two step down in a loop: at tile = granule = 1,024 they agree."""
    grid = list(_block_grid(1024, 1024))
    got = planner([("B", n, fit, 1024, 1024) for n, fit in grid])

    def stepped(n32, fit):                               # fc_plan_tapes' shape at (1024, 1024)
        if fit >= n32:
            return n32
        if fit < 1024:
            return 0
        nb = (n32 + fit - 1) // fit
        block = ((n32 + nb - 1) // nb + 1023) // 1024 * 1024
        while block > fit:
            block -= 1024
        return block

    for (n, fit), (block,) in zip(grid, got):
        assert block == R.rt_block(n, fit) == stepped(n, fit), (n, fit)


def _segment_grid():
    for n32, n_iv, cw, n_params in [(4096, 8, 16, 24735), (4096, 128, 32, 24735), (65536, 8, 32, 24735), (65536, 288, 32, 98000), (262144, 16, 32, 24735),
                                    (20000, 5, 32, 100), (32, 4, 16, 24735)]:
        for per_col_iv in (8 * 1000 * 4 + 8 * 64, 4 * 2100 * 4 + 4 * 16 + 4 * 8):
            whole = per_col_iv * n_iv * n32
            budgets = {0, 31 * per_col_iv, 32 * per_col_iv, 33 * per_col_iv, whole - 1, whole, 2 * whole}
            for frac in (0.9, 0.6, 0.5, 0.4, 0.3, 0.26, 0.25, 0.2, 0.13, 0.1, 0.05, 0.02, 0.01, 0.004, 0.001, 0.0003, 0.0001):
                budgets.add(int(whole * frac))
            for cols in (16384, 16383, 8192, 8191, 1024):
                budgets.update((per_col_iv * cols, per_col_iv * n_iv * cols, per_col_iv * n_iv * cols - 1))
            for b in sorted(budgets):
                yield n32, n_iv, cw, per_col_iv, b, n_params


def test_fc32_blocks_or_segments(planner):
    grid = list(_segment_grid())
    got = planner([("F",) + c for c in grid])
    seen = set()
    for c, (block, seg) in zip(grid, got):
        n32, n_iv, cw, per_col_iv, budget, n_params = c
        b0, s0, branch = R.fc_block_seg(*c)
        seen.add(branch)
        assert (block, seg) == (b0, s0), (c, branch)
        if block >= 32 and seg >= 1:                     # a plan the ABI accepts: its tapes fit, whole tiles, the segments cover the axis
            assert block % 32 == 0 and block <= n32 and seg <= n_iv and per_col_iv * block * seg <= budget, (c, block, seg)
            assert block * ((n32 + block - 1) // block) >= n32 and seg * ((n_iv + seg - 1) // seg) >= n_iv
    # (a column block takes all the columns one interval fits for, so its segments hold one interval: only segments of all columns can shrink)
    assert seen >= {"whole", "blocks", "segments of all columns", "segments of a block", "segments of all columns, slab shrinks seg", "nothing",
                    "nothing (slab)"}, seen


def test_fc32_ensemble_segments_and_budget(planner):
    grid = [(n32, n_iv, 16, Nz, p, b, 24735) for n32, n_iv, Nz in [(32, 4, 32), (4096, 8, 32), (4096, 128, 64)] for p in (32512, 33696)
            for b in sorted({0, 1 << 20, 1 << 26, 1 << 30, 1 << 33} | {int(p * n32 * n_iv * f) for f in (0.01, 0.1, 0.3, 0.5, 0.9, 1.0, 1.2, 2.0)})]
    got = planner([("E",) + c for c in grid])
    segs = set()
    for c, (seg,) in zip(grid, got):
        assert seg == R.fc_ens_seg(*c), c
        segs.add((seg == c[1], seg == 1))
    assert segs >= {(True, False), (False, True), (False, False)}          # the whole axis, one interval, something between
    hb = [(0, 0), (5, 5), (5, 6), (6, 5), (287 << 30, 3 << 30), (1 << 30, 3 << 30)]
    assert planner([("H",) + c for c in hb]) == [(f - m if f > m else 0,) for f, m in hb]
