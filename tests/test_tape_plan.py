"""csrc/tape_plan.h on the host: the planners' arithmetic (columns per pass, fc32's column blocks or time segments) compiled alone with the host
compiler and held, value for value, to tests/tape_plan_restatement.py — the three formulas as they stood in api.hip — over grids that reach every
branch, the ones only a nearly full card takes included.  The second half does the same for the planners' decisions (plan_fc_tapes, plan_t16_tapes,
plan_t16_ens_tapes, plan_rt_tapes: on or off, optional tapes, overrides, refusals) against restatements of api_grad.hip / api_ensemble.hip as they
stood before those decisions moved; each restatement names the branch it took and the grids must reach every named one.  Those tests run the driver
a second time under the address and undefined-behaviour sanitizers.  No GPU, no library."""
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


# ---- the planners' decisions (plan_fc_tapes, plan_t16_tapes, plan_t16_ens_tapes, plan_rt_tapes) against their restatements ------------------------------
@pytest.fixture(scope="module")
def checked_planner(planner, tmp_path_factory):
    """The driver a second time under the address and undefined-behaviour sanitizers, over the same inputs: both must print the same."""
    exe = str(tmp_path_factory.mktemp("tape_plan_san") / "tape_plan_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "tape_plan_check.cpp"), "-I", os.path.join(ROOT, "climateparameterizations.jl_amd", "csrc"), "-o", exe])

    def run(cases):
        out = planner(cases)
        r = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in cases), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stderr
        assert [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()] == out
        return out

    return run


def _flag(v):                                            # None / False / True -> the header's FLAG_UNSET / FLAG_OFF / FLAG_ON
    return -1 if v is None else int(bool(v))


def _count(v):                                           # a forced block: atoi(value), 0 when unset
    return 0 if v is None else v


def _seg_count(v):                                       # COLNDE_FC_SEG: the count, 0 when unset, -1 when set to no count
    return 0 if v is None else (v if v >= 1 else -1)


def test_fc32_bytes_per_column_and_interval(checked_planner):
    grid = [(s, nst, row, 512, cw, sw, conv) for s in (1, 2, 20) for nst in (4, 7) for row in (18 * 32 + 31, 18 * 64 + 63) for cw in (16, 32) for sw in (0, 1)
            for conv in (0, 16 * 2 * 32, 16 * 2 * 64)]
    got = checked_planner([("P",) + c for c in grid])
    for (s, nst, row, mask, cw, sw, conv), (b,) in zip(grid, got):
        assert b == R.fc_per_col_iv(s, nst, row, mask, cw, bool(sw), conv) == s * nst * (4 * row + 4 * mask // cw + 8 * sw + conv // 16 * 4)


def _fc_tapes_grid():
    GB3 = 3 << 30
    for n32, n_iv, cw, Nz, n_params in [(32, 4, 16, 32, 24735), (4096, 8, 16, 32, 24735), (65536, 8, 32, 32, 24735), (262144, 16, 32, 64, 98623)]:
        p = 33696
        margin = GB3 + (n32 // cw * 8 + 4096) * (n_params + 8) * 4 + n32 * Nz * 4
        whole = p * n_iv * n32
        for b in sorted({0, 31 * p, 32 * p, whole - 1, whole, 2 * whole} | {int(whole * f) for f in (0.5, 0.26, 0.1, 0.01, 0.001)}):
            for fb in (None, 0, 16, 32, 100, 10 ** 6):
                for fs in (None, 0, 1, 3, 1000):
                    yield (n32, n_iv, cw, Nz, n_params, p, margin + b, fb, fs, False, 1, 0)
            yield (n32, n_iv, cw, Nz, n_params, p, b, None, None, False, 1, 0)              # (less free memory than the margin)
        if n32 > 4096:
            continue
        for K in (1, 3, 300):
            for cslab in (0, 256 * 9):
                frees = {0, GB3, GB3 + (1 << 40)}
                for seg in {1, max(1, n_iv // 2), n_iv}:
                    need = R.fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, p, n_params, seg, cslab)
                    frees.update((GB3 + K * need - 1, GB3 + K * need, GB3 + K * need + K))
                for free in sorted(frees):
                    for fs in (None, 0, 2, 1000):
                        yield (n32, n_iv, cw, Nz, n_params, p, free, None, fs, True, K, cslab)


def test_fc32_planner_of_single_handles_and_ensembles(checked_planner):
    grid = list(_fc_tapes_grid())
    got = checked_planner([("T", n32, n_iv, cw, Nz, P, p, free, int(ens), K, cslab, _count(fb), _seg_count(fs))
                           for n32, n_iv, cw, Nz, P, p, free, fb, fs, ens, K, cslab in grid])
    seen = set()
    for c, (block, seg, model_bytes, status) in zip(grid, got):
        n32, n_iv, cw, Nz, P, p, free, fb, fs, ens, K, cslab = c
        b0, s0, refused, need, branch = R.fc_tapes(n32, n_iv, cw, Nz, P, p, free, fb, fs, ens, K, cslab)
        seen.add(branch)
        assert status == (0 if not refused else 2 if ens else 1), (c, branch)
        assert (block, seg, model_bytes) == (b0, s0, need), (c, branch)
        if branch == "forced block alone":
            assert seg == n_iv
    assert seen >= {"single, unforced", "forced block alone", "forced seg alone", "both forced", "single refused", "ensemble, unforced", "ensemble, forced seg",
                    "ensemble refused", "conv ensemble"}, seen


T16_STATUS = {"taped": 0, "inreg": 1, "refused: rows in global, off": 2, "refused: rows in global, too large": 3, "refused: rows in global, no fit": 4}
T16_BRANCHES = {"forced off", "tile state too large", "needs Z", "off for LDS", "ZTAPE=0 defeats needs-Z", "rows-in-global refused (forced off)",
                "rows-in-global refused (too large)", "whole problem", "equal blocks", "forced block", "nothing fits, so in-register",
                "nothing fits with rows in global, so refused", "rich automatic", "rich automatic dropped for budget", "rich forced shrinks the block",
                "rich forced but not one tile fits, so dropped", "rich forced off"}


def _t16_grid():
    pc, pcr = 100000, 400000
    # (ns, n_bias, LDS bytes of the adjoint with its activation array, without it, with rows in global memory, rows in global memory)
    nets = [(96, 303, 60000, 40000, 30000, False), (256, 303, 60000, 40000, 30000, False), (96, 1293, 170000, 85000, 30000, False),
            (96, 1293, 170000, 170000, 30000, False), (96, 2493, 330000, 170000, 100000, True), (96, 5000, 330000, 170000, 100000, True),
            (256, 2493, 330000, 170000, 100000, True)]
    for n16 in (32, 4096, 20000):
        budgets = sorted({0, 15 * pc, 16 * pc, 16 * pcr - 1, 16 * pcr, n16 * pc - 1, n16 * pc, n16 * pcr - 1, n16 * pcr, 1000 * pc, 2048 * pcr, 5000 * pc})
        for net in nets:
            for split in (False, True):
                for budget in budgets:
                    for dw in (None, False, True):
                        for z in (None, False):
                            for rich in (None, False, True):
                                for fb in (None, 8, 16, 4096):
                                    yield (n16, 16) + net[:2] + (net[5], split) + net[2:5] + (pc, pcr, budget, dw, z, rich, fb)


def test_tile16_planner(checked_planner):
    grid = list(_t16_grid())
    got = checked_planner([("S",) + c[:4] + (int(c[4]), int(c[5])) + c[6:12] + (_flag(c[12]), _flag(c[13]), _flag(c[14]), _count(c[15])) for c in grid])
    seen = set()
    for c, (status, need_z, block, rich) in zip(grid, got):
        n16, tile, ns, n_bias, ag, split, lds, lds_noA, lds_ag, pc, pcr, budget, dw, z, fr, fb = c
        st0, z0, b0, r0, branch = R.t16_tapes(n16, ns, n_bias, ag, split, lds, lds_noA, lds_ag, pc, pcr, budget, dw, z, fr, fb)
        seen.add(branch)
        assert (status, bool(need_z), block, bool(rich)) == (T16_STATUS[st0], z0, b0, r0), (c, branch)
        if status == 0:                                  # a taped plan: whole tiles, and what it tapes fits unless the block was forced
            assert block % 16 == 0 and 16 <= block <= n16
            if fb is None or fb < 16:
                assert block * (pcr if rich else pc) <= budget, (c, block, rich)
            assert not (rich and not split)
    assert seen >= T16_BRANCHES, T16_BRANCHES - seen


def test_wind_mixing_ensemble_planner(checked_planner):
    rich_b, plain_b = 6585676, 5258572
    grid = [(K, nt, rich_b, plain_b, b, f) for K in (1, 2, 64, 129) for nt in (1, 2, 64)
            for b in sorted({0, K * plain_b - 1, K * plain_b, K * rich_b - 1, K * rich_b, 1 << 40}) for f in (None, False, True)]
    got = checked_planner([("N",) + c[:5] + (_flag(c[5]),) for c in grid])
    seen = set()
    for c, (rich, bytes_per_model, refused) in zip(grid, got):
        r0, need, ref0, branch = R.t16_ens_tapes(*c)
        seen.add(branch)
        assert (bool(rich), bytes_per_model, bool(refused)) == (r0, need, ref0), (c, branch)
    assert seen >= {"rich automatic", "rich gives way", "rich forced on", "rich forced off", "refused", "plain"}, seen


def test_regtile_planner(checked_planner):
    px, p2, pz = 1000, 500, 700
    grid = [(n32, px, p2, pz, b, wz, fb) for n32 in (32, 1024, 4096, 32768, 100000)
            for b in sorted({0, 1023 * 1500, 1024 * 1500, 1024 * 2200 - 1, 1024 * 2200, n32 * 1500, n32 * 2200 - 1, n32 * 2200, n32 // 2 * 2200, n32 // 3 * 1500})
            for wz in (False, True) for fb in (None, 16, 32, 2048, 10 ** 6)]
    got = checked_planner([("R",) + c[:5] + (int(c[5]), _count(c[6])) for c in grid])
    seen = set()
    for c, (block, ztape) in zip(grid, got):
        b0, z0, branch = R.rt_tapes(*c)
        seen.add(branch)
        assert (block, bool(ztape)) == (b0, z0), (c, branch)
        assert not (ztape and not c[5])
    assert seen >= {"whole with Z1", "blocks with Z1", "Z1 dropped to fit", "nothing fits", "forced block", "want_z off on entry"}, seen
