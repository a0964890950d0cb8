"""What the step-schedule tests share (tests/test_schedule_host.py, tests/test_gpu_schedule.py): the problems, the float64 reference and the bounds.

The reference for a schedule is the oracle unchanged: `oracle.nde_oracle.solve` and `loss_and_grad` take their steps from the module-level
`_step_times(cfg)`, which `oracle_schedule` replaces (monkeypatch) with one that reads a schedule and keeps the (t, dt, save_idx) contract."""
import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O

SC = [1, 1, 1, 5e-3, 5e-3, 5e-3]
# the bounds tests/test_gpu_ensemble.py:99-100 holds these same kernels to on this problem family, and tests/test_gpu_parity.py's SOL_ATOL for the
# forward solve of this engine (scaled units, O(1) profiles)
LOSS_RTOL, GRAD_RTOL, SOL_ATOL = 8e-5, 2e-4, 2e-5
UNEVEN = tuple(k / 256.0 for k in (0, 1, 2, 3, 4, 8, 16))           # intervals of 1, 1, 1, 1, 4, 8 units of 1/256: exact in float32
UNEVEN_MIN = (2, 2, 2, 2, 7, 13)                                     # ceil(lambda dt / 2.785), lambda = 4 tau (nu0 + nu_minus) Nz^2 / H^2 = 1081.08
UNEVEN_POW2 = (2, 2, 2, 2, 8, 16)                                    # ... rounded up to powers of two: 32 steps, against 6 x 16 = 96 with one count
REFINED = tuple(k / 256.0 for k in (0, 0.25, 0.5, 0.75, 1, 2, 2.5, 3))   # (8, 2, 4) on (0, 1, 2, 3)/256 = substeps 2 on this axis, step for step


def base_problem(n_col, n_frames=4, **kw):
    """save times k/256 (exact in float32); the stability minimum is 2 per unit interval"""
    return synthetic.wind_mixing_problem(n_col, n_frames=n_frames, n_frames_total=257, weight_divisor=1e2, **kw)


def with_axis(p, save_times, **kw):
    return synthetic.ColumnProblem(p.cfg.with_(save_times=tuple(save_times), **kw), p.x0, p.bcs, p.weights, p.weights_truth)


def schedule_step_times(schedule):
    counts = [int(s) for s in schedule]

    def _step_times(cfg):
        ts = np.asarray(cfg.save_times, dtype=np.float64)
        assert len(counts) == len(ts) - 1
        out = []
        for i, S in enumerate(counts):
            dt = (ts[i + 1] - ts[i]) / S
            for s in range(S):
                out.append((ts[i] + s * dt, dt, i + 1 if s == S - 1 else -1))
        return out
    return _step_times


def oracle_schedule(monkeypatch, schedule):
    monkeypatch.setattr(O, "_step_times", schedule_step_times(schedule))


def pow2_ceil(v):
    p = 1
    while p < v:
        p *= 2
    return p


def estimate_norm(a, b, factor, floor=1e-3):
    """numpy restatement of colnde_error_estimate's norm: max over columns and save points of rms_i((a_i - b_i) / (floor + |b_i|)), times Richardson's factor"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = (a - b) / (floor + np.abs(b))
    return factor * np.sqrt((q * q).mean(axis=-1))          # [column][save point]
