"""Handle life cycle: every device allocation a handle makes (weight images, tapes, slabs, the scratch of colnde_error_estimate /
colnde_choose_substeps, the split-arithmetic images) is returned by colnde_destroy, and a refused colnde_create or a failed call leaves
nothing behind.  One handle = one GPU = one host thread (include/colnde.h); a training script creates and destroys handles per stage of the
reference's schedule (train_NDE's epochs x optimisers, NDE_training.jl:335-372), so a leak here is a crash after a few hours there."""
import ctypes

import numpy as np
import pytest
import torch

import colnde
from colnde import _lib, synthetic
from colnde.config import to_c_config
from colnde.nde import ENGINE_REGTILE, ENGINE_TILE16

pytestmark = pytest.mark.gpu


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def _cases():
    wm = synthetic.wind_mixing_problem(70, n_frames=5, weight_divisor=1e2)
    fc = synthetic.free_convection_problem(70, Nz=32, n_save=9)
    # ConvectiveAdjustmentNDE at the step bench.py's configs[3] shard takes (save interval 1/128, 4 RKC2 steps of 17 stages: dt = 1/512).  Round 4 ran this case
    # at dt = 1/8 (2 steps of 132 stages over intervals of 1/4) and had to allow the two arithmetics 2e-2 apart: that step is 400x from converged
    # (profiles/r05_rkc2_conditioning.json) — the discrete dynamics flips switches on round-off — and the stage count has nothing to do with it
    ca = synthetic.free_convection_problem(40, Nz=64, n_save=5, t_end=4.0 / 128.0, convective_adjustment=True)
    return [
        ("regtile", wm, wm.cfg, dict(engine=ENGINE_REGTILE), [1, 1, 1, 5e-3, 5e-3, 5e-3], {}),
        ("net-split (AUTO)", wm, wm.cfg, dict(), [1, 1, 1, 5e-3, 5e-3, 5e-3], {}),
        ("tile16, f32 MFMA", wm, wm.cfg, dict(engine=ENGINE_TILE16, matrix_arithmetic="f32_mfma"), [1, 1, 1, 0, 0, 0], {}),
        ("fc32, time segments + column blocks", fc, fc.cfg, dict(), [0, 0, 1, 0, 0, 0], {"COLNDE_FC_SEG": "3", "COLNDE_FC_BLOCK": "32"}),
        ("fc32 64 levels, RKC2", ca, ca.cfg.with_(stepper="rkc2", substeps=4), dict(), [0, 0, 1, 0, 0, 0], {}),
    ]


@pytest.mark.parametrize("case", range(5))
def test_create_use_destroy_returns_all_device_memory(case, monkeypatch):
    name, p, cfg, kw, sc, env = _cases()[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = p.x0.shape[0]

    def cycle():
        with colnde.ColumnNDE(cfg, n, **kw) as nde:
            nde.set_problem(p.x0, p.bcs)
            truth = nde.forward(p.weights_truth)
            nde.set_problem(p.x0, p.bcs, truth)
            nde.error_estimate(p.weights)
            nde.choose_substeps(p.weights, 0.5)                          # (before the tapes are planned; RKC2: the stage table follows the step)
            if cfg.stepper == "rkc2":
                nde.set_substeps(cfg.substeps)
            tot, terms, grad = nde.loss_grad(p.weights, sc)
            nde.set_matrix_arithmetic("f32_mfma" if nde.matrix_arithmetic == "bf16x3_exact" else "bf16x3_exact")
            tot2, _, grad2 = nde.loss_grad(p.weights, sc)
            nde.loss_per_tstep(p.weights)
            # the two arithmetics agree to 1e-4 in the loss (ConvectiveAdjustmentNDE through live switches: 1e-3)
            assert np.isfinite(tot) and np.isfinite(grad).all() and abs(tot2 - tot) <= (1e-3 if cfg.stepper == "rkc2" else 1e-4) * abs(tot)
            return nde.describe()

    cycle()                                                              # (first use: the runtime's own pools, code objects)
    before = _free_bytes()
    for _ in range(24):
        d = cycle()
    after = _free_bytes()
    assert before - after <= (8 << 20), (name, before - after, d)          # (free memory may GROW: the runtime returns pool blocks of the first cycle)


def test_refused_create_and_failed_calls_leave_nothing_behind():
    p = synthetic.wind_mixing_problem(33, n_frames=3)
    L = _lib.lib()
    c, keep = to_c_config(p.cfg, 33)
    c.layer_sizes[3] = 30                                                # refused by validation
    h = ctypes.c_void_p()
    L.colnde_create(ctypes.byref(c), ctypes.byref(h))                    # (warm-up of the error path)
    before = _free_bytes()
    for _ in range(20):
        h = ctypes.c_void_p()
        assert L.colnde_create(ctypes.byref(c), ctypes.byref(h)) != 0 and not h.value
    # an engine that does not cover the configuration: refused after the device was selected
    from colnde.nde import ENGINE_FC32
    for _ in range(5):
        with pytest.raises(colnde.ColndeError):
            colnde.ColumnNDE(p.cfg, 33, engine=ENGINE_FC32)
    # calls that fail on a live handle: no problem set, a time step outside the stability region
    with colnde.ColumnNDE(p.cfg, 33) as nde:
        for _ in range(5):
            with pytest.raises(colnde.ColndeError):
                nde.loss_grad(p.weights, [1, 1, 1, 0, 0, 0])
            with pytest.raises(colnde.ColndeError):
                nde.error_estimate(p.weights)
    with pytest.raises(colnde.ColndeError):
        with colnde.ColumnNDE(p.cfg.with_(substeps=1), 33) as nde:
            nde.set_problem(p.x0, p.bcs)
            nde.forward(p.weights)
    after = _free_bytes()
    assert before - after <= (8 << 20), before - after


def test_create_refused_after_partial_construction_leaves_nothing_behind():
    """A creator that refuses AFTER it has allocated: the wide 3 x 96-400-400-31 network has its activation rows and both bf16 plane images on the
    device (about 8 MB: (75 + 325 + 26) tile-blocks x 192 items x 16 B x 3 nets each way, plus the rows) by the time `engine = regtile` turns out not to
    cover it; an RKC2 wind-mixing configuration has its coefficient table (kilobytes: there for the exit path) when `engine = fc32` does not."""
    from colnde.nde import ENGINE_FC32
    wide = synthetic.wind_mixing_problem(16, n_frames=3, weight_divisor=1e2, layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))
    small = synthetic.wind_mixing_problem(16, n_frames=3)
    for cfg, engine in ((wide.cfg, ENGINE_REGTILE), (small.cfg.with_(stepper="rkc2"), ENGINE_FC32)):
        def refused():
            with pytest.raises(colnde.ColndeError, match="requested, but it covers only"):
                colnde.ColumnNDE(cfg, 16, engine=engine)

        refused()                                                        # (warm-up of the error path)
        before = _free_bytes()
        for _ in range(8):
            refused()
        after = _free_bytes()
        print("refused create x 8: free memory fell by %d bytes (%s)" % (before - after, "regtile on the wide network" if engine == ENGINE_REGTILE else "fc32, RKC2"))
        assert before - after <= (8 << 20), (engine, before - after)


def test_two_handles_in_two_host_threads_do_not_disturb_each_other():
    """include/colnde.h: one handle = one host thread AT A TIME; two handles may be driven by two threads at once (ctypes releases the GIL
    for the call).  Their results are bit-identical to the serial ones and colnde_last_error stays per thread."""
    import threading
    wm = synthetic.wind_mixing_problem(40, n_frames=5, weight_divisor=1e2)
    fc = synthetic.free_convection_problem(40, Nz=32, n_save=5)
    jobs = [(wm, dict(engine=ENGINE_REGTILE), [1, 1, 1, 5e-3, 5e-3, 5e-3]), (fc, dict(), [0, 0, 1, 0, 0, 0]), (wm, dict(), [1, 1, 1, 0, 0, 0])]

    def prepare(p, kw):
        nde = colnde.ColumnNDE(p.cfg, 40, **kw)
        nde.set_problem(p.x0, p.bcs)
        nde.set_problem(p.x0, p.bcs, nde.forward(p.weights_truth))
        return nde

    handles = [prepare(p, kw) for p, kw, _ in jobs]
    try:
        serial = [h.loss_grad(p.weights, sc) for h, (p, _, sc) in zip(handles, jobs)]
        results, errors = [None] * len(jobs), [None] * len(jobs)

        def work(i):
            h, (p, _, sc) = handles[i], jobs[i]
            try:
                for _ in range(12):
                    r = h.loss_grad(p.weights, sc)
                    with pytest.raises(colnde.ColndeError, match="matrix_arithmetic"):          # an error of THIS thread, with its own message
                        _lib.check(h._L.colnde_set_matrix_arithmetic(h._h, 9))
                results[i] = r
            except BaseException as e:                                                          # noqa: BLE001 (reported below, in the main thread)
                errors[i] = e

        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert errors == [None] * len(jobs), errors
        for (t0, terms0, g0), (t1, terms1, g1) in zip(serial, results):
            assert t0 == t1 and np.array_equal(g0, g1) and np.array_equal(terms0, terms1)
    finally:
        for h in handles:
            h.close()
