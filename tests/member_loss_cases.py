"""What the member-loss tests share (tests/test_member_loss_host.py, tests/test_gpu_member_loss.py): the inputs, the float64 reference, the bounds.

The member loss of an ensemble (colnde_ensemble_set_member_loss): member k is differentiated under
    sum_q s[k][q] * sum_c w[k][c] * (term q of column c) / sum_c w[k][c].
The float64 reference is the oracle unchanged, one column at a time: `oracle.nde_oracle.loss_and_grad` on column c alone is term q of column c (and
its gradient), and the rows are combined with the weights here.  For a 0/1 mask this is the oracle on the subset of columns (the host test holds that
to 1e-12), so nothing in `oracle/` needs to know about weights.

Inputs: tests/test_gpu_ensemble.py's problems (5 save points), weights and PHYS rows, K = 3.  Masks on 8 columns: members on columns {0, 2, 5},
{1, 3, 4, 6, 7} and all; one fractional row.  Scalings: `calculate_loss_scalings` with the reference's fractions (0.8, 0.8, 0.5) on each member's
own unscaled terms over its own columns — determine_loss_scalings per member."""
import functools

import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O
from tests import schedule_common as C
from tests.test_gpu_ensemble import PHYS, _model_cfg, _weights

K = 3
FRACTIONS = dict(T=0.8, dTdz=0.8, profile=0.5)                       # train_NDE.jl:110, train_NDE_args.jl:174
LOSS_RTOL, GRAD_RTOL = 8e-5, 2e-4                                    # tests/test_gpu_ensemble.py:99-100
MASKS8 = ((0, 2, 5), (1, 3, 4, 6, 7), tuple(range(8)))
FRACTIONAL8 = (0.25, 1.0, 0.0, 0.5, 2.0, 0.0, 0.75, 1.5)             # exact in float32; two columns out


def mask_weights(masks, n_col):
    cw = np.zeros((len(masks), n_col), np.float32)
    for k, idx in enumerate(masks):
        cw[k, list(idx)] = 1.0
    return cw


def masks_for(n_col):
    """the masks of MASKS8 carried to n_col columns: the same pattern repeated, so every tile has columns in and out of members 0 and 1"""
    return tuple(tuple(c for c in range(n_col) if (c % 8) in m) for m in MASKS8)


def tile_weights(n_col):
    """Column weights [K, n_col] for more than one 16-column tile (17 and 40 columns): member 0 on the columns with c % 3 == 0, member 1 on the others,
    member 2 fractional, 0.25 (1 + c % 7).  The periods 3 and 7 share nothing with the tile width: a kernel that indexed the weights by the column's
    place in its tile (c % 16), or with another row stride, reads other weights (`tile_local` restates the first; the host test holds its distance)."""
    c = np.arange(n_col)
    return np.stack([(c % 3 == 0), (c % 3 != 0), 0.25 * (1 + c % 7)]).astype(np.float32)


def tile_local(cw):
    """the weights a kernel would read that indexed them by c % 16"""
    cw = np.asarray(cw)
    return cw[:, np.arange(cw.shape[1]) % 16]


def fixed_scalings():
    """three different positive rows (float32): calculate_loss_scalings on the 8-column masks, used wherever the test is not about the scalings' origin"""
    return member_scalings("base", 8, key(mask_weights(MASKS8, 8)))


@functools.lru_cache(maxsize=None)
def problem(kind, n_col):
    """(p, truth, physics or None, schedule or None) — kind: base | sched | rkc2.
    base: tests/test_gpu_ensemble.py's problem.  sched: the (0, 1, 2, 3)/256 axis under the schedule (8, 2, 4) (tests/schedule_common.py).
    rkc2: the RKC2 convective-adjustment branch of tests/test_gpu_ensemble.py (no closure constants to vary)."""
    if kind == "base":
        p = synthetic.wind_mixing_problem(n_col, n_frames=5, weight_divisor=1e2)
        phys, sched = PHYS[:K], None
    elif kind == "sched":
        p = C.base_problem(n_col)
        phys, sched = PHYS[:K], (8, 2, 4)
    else:
        p = synthetic.wind_mixing_problem(n_col, n_frames=5, weight_divisor=1e2, modified_pacanowski_philander=False, zero_weights=False,
                                          convective_adjustment=True, kappa=10.0, stepper="rkc2", substeps=1)
        phys, sched = None, None
    truth = O.solve(p.cfg, p.x0, p.bcs, p.weights_truth).astype(np.float32)       # (the truth of a scheduled problem: the axis' own cfg.substeps)
    if kind == "rkc2":
        # without the closure the synthetic columns are alike to four digits and no mask could be told from another: the truth of column c is
        # scaled by 1 + 0.002 c (data, like any other truth), which spreads the columns' losses over a factor of the order of ten
        truth = (truth * (1.0 + 2e-3 * np.arange(n_col, dtype=np.float32))[:, None, None]).astype(np.float32)
    for a in (p.x0, p.bcs, truth):
        a.setflags(write=False)                                                   # shared among the tests: left unchanged
    return p, truth, phys, sched


def weights(kind, n_col):
    return _weights(problem(kind, n_col)[0].cfg, K, seed=3 if kind == "rkc2" else 11)


def member_cfg(kind, n_col, k):
    p, _, phys, _ = problem(kind, n_col)
    return p.cfg if phys is None else _model_cfg(p.cfg, phys[k])


def _with_schedule(sched, fn):
    """fn() with the oracle stepping by `sched` (schedule_common.schedule_step_times), restored afterwards"""
    if sched is None:
        return fn()
    keep = O._step_times
    O._step_times = C.schedule_step_times(sched)
    try:
        return fn()
    finally:
        O._step_times = keep


@functools.lru_cache(maxsize=None)
def column_rows(kind, n_col, k, scalings):
    """The oracle on every column alone, for member k under `scalings` (a tuple of 6): (totals [n_col], terms [n_col, 6], grads [n_col, P]), float64."""
    p, truth, _, sched = problem(kind, n_col)
    cfg, w, sc = member_cfg(kind, n_col, k), weights(kind, n_col)[k], np.array(scalings, np.float64)
    rows = _with_schedule(sched, lambda: [O.loss_and_grad(cfg, p.x0[c:c + 1], p.bcs[c:c + 1], w, truth[c:c + 1], sc)[:3] for c in range(n_col)])
    return tuple(np.array([r[i] for r in rows], np.float64) for i in range(3))


def combine(rows, cw):
    """sum_c w_c (row of column c) / sum_c w_c for each of (totals, terms, grads)"""
    cw = np.asarray(cw, np.float64)
    return tuple((cw[:, None] * a if a.ndim == 2 else cw * a).sum(axis=0) / cw.sum() for a in rows)


def reference(kind, n_col, k, scalings, cw):
    """(total, scaled terms [6], grad [P]) of member k under its scalings and column weights, float64"""
    return combine(column_rows(kind, n_col, k, tuple(float(s) for s in scalings)), cw)


def subset_oracle(kind, n_col, k, scalings, idx):
    """the oracle on the columns idx alone: what a 0/1 mask must equal"""
    p, truth, _, sched = problem(kind, n_col)
    idx = list(idx)
    return _with_schedule(sched, lambda: O.loss_and_grad(member_cfg(kind, n_col, k), p.x0[idx], p.bcs[idx], weights(kind, n_col)[k], truth[idx],
                                                         np.array(scalings, np.float64))[:3])


@functools.lru_cache(maxsize=None)
def member_scalings(kind, n_col, cw_key):
    """determine_loss_scalings per member: calculate_loss_scalings with FRACTIONS on each member's own unscaled terms over its own columns.  float32
    values (what the ABI takes), as a [K, 6] array; cw_key: the column weights as a tuple of tuples."""
    cw = np.array(cw_key, np.float64)
    out = []
    for k in range(K):
        _, terms, _ = combine(column_rows(kind, n_col, k, (1.0,) * 6), cw[k])
        out.append(O.calculate_loss_scalings(terms, FRACTIONS, True))
    return np.array(out, np.float32)


def key(cw):
    return tuple(tuple(float(x) for x in row) for row in np.asarray(cw))


# ---- the restatement of csrc/member_loss.h --------------------------------------------------------------------------------------------------------
def loss_weight_rows(scalings, column_weights, n_col, n_save, Nz, wind_mixing=True):
    """the K LossWeights rows in float32: loss_weights()'s expression (api.hip) with sum_c w[k][c], summed in double, in the column count's place"""
    sc = np.asarray(scalings, np.float32)
    rows = np.zeros((sc.shape[0], 8), np.float32)
    for k in range(sc.shape[0]):
        s = float(n_col) if column_weights is None else float(np.asarray(column_weights, np.float32)[k].astype(np.float64).sum())
        n_prof, n_grad = s * n_save * Nz, s * n_save * (Nz + 1)
        if wind_mixing:
            rows[k, :3] = (sc[k, :3].astype(np.float64) / n_prof).astype(np.float32)
            rows[k, 3:6] = (sc[k, 3:6].astype(np.float64) / n_grad).astype(np.float32)
        else:
            rows[k, 2] = np.float32(np.float64(sc[k, 2]) / n_prof)
    return rows
