"""What the ensemble-schedule tests share (tests/test_ens_schedule_host.py, tests/test_gpu_ens_schedule.py).  A helper, not a test.

* `choose_round`: a NumPy restatement, in float32, of csrc/step_schedule.h's `sched_choose_round` — one round of the greedy choice.
* `greedy`: the whole run over any source of estimates (the float64 oracle, twin ensembles' `forward`), with the distance of every round from the
  rule's two thresholds.
* the K = 3 problem on which `colnde_ensemble_choose_schedule` is held to that run, and the schedule the float64 oracle gives on it.

The margins are conditions on the INPUTS, not tolerances: a round whose estimate sits within 5 % of reltol, or in which some interval's addition sits
within 5 % of half the largest, could go either way between float32 and float64 (or between two float32 summation orders), and a test that compares
counts would then compare round-off.  The constants, the weights' seed and the axis below are chosen so that no round is near; the tests assert it."""
import numpy as np

from colnde import synthetic
from tests import schedule_common as C
from tests.test_gpu_ensemble import _model_cfg

MET, DOUBLED, NOT_FINITE, FLOOR, TOO_STIFF = range(5)
VERDICTS = ("MET", "DOUBLED", "NOT_FINITE", "FLOOR", "TOO_STIFF")
SCHEDULE_MAX = 4096
F = np.float32

RELTOL = 1e-3
FACTOR_RK4 = 16.0 / 15.0                 # richardson_factor: the smooth wind-mixing closure under RK4
N_COL = 8
# (nu0, nu_minus, dRi, Ric, Pr) of the three members: tests/test_gpu_ensemble.py's first three rows with more viscosity in members 0 and 1.  Member 0
# (nu0 + nu_minus = 0.1301) sets the stability minima (2, 2, 2, 2, 8, 16: already powers of two, so the first round steps close to the bound) and drives
# the schedule: the float64 run below takes two rounds, est = 1.61e-3 then 2.59e-4, and doubles the first interval alone.
PHYS_K3 = np.array([[1e-4, 0.13, 1.0, 0.25, 1.0], [5e-4, 0.12, 0.8, 0.2, 1.0], [1e-3, 0.05, 1.3, 0.3, 1.2]], np.float32)
SEED = 11
# the float64 oracle's greedy run on this problem (tests/test_ens_schedule_host.py recomputes it): where it starts, and the schedule it ends at
MINIMA_POW2_F64 = (2, 2, 2, 2, 8, 16)
SCHEDULE_F64 = (4, 2, 2, 2, 8, 16)
ROUNDS_F64 = 2


def problem_k3():
    """the K = 3 problem: 8 columns on the uneven axis (intervals of 1, 1, 1, 1, 4, 8 units of 1/256), three separately drawn weight vectors"""
    p = C.with_axis(C.base_problem(N_COL), C.UNEVEN)
    W = np.stack([synthetic.make_weights(synthetic._rng(SEED, k), p.cfg, 1e2) for k in range(3)]).astype(np.float32)
    return p, W


def member_cfgs(cfg, physics):
    return [_model_cfg(cfg, row) for row in physics]


def choose_round(E, reltol, prev_est, S):
    """(verdict, est, S after the round): sched_choose_round in float32, statement by statement"""
    E, reltol, prev_est = np.asarray(E, F), F(reltol), F(prev_est)
    S = [int(s) for s in S]
    mx = F(0)
    for e in E:
        if not (e == e) or e > F(3.0e38):
            return NOT_FINITE, float(e), S
        if e > mx:
            mx = e
    if mx <= reltol:
        return MET, float(mx), S
    if prev_est > F(0) and mx > F(0.8) * prev_est:
        return FLOOR, float(mx), S
    d = [F(E[i + 1] - (E[i] if i else F(0))) for i in range(len(E) - 1)]
    dmax = F(0)
    for v in d:
        if v > dmax:
            dmax = v
    doubled = False
    for i, v in enumerate(d):
        if (v if v > F(0) else F(0)) >= F(0.5) * dmax and S[i] < SCHEDULE_MAX:
            S[i] *= 2
            doubled = True
    return (DOUBLED if doubled else TOO_STIFF), float(mx), S


def margins(E, reltol):
    """how far a round stands from the rule's thresholds: (|est - reltol| / reltol, min over intervals of |d[n] - dmax / 2| / (dmax / 2))"""
    E = np.asarray(E, np.float64)
    d = np.maximum(0.0, np.diff(np.concatenate([[0.0], E[1:]])))
    half = 0.5 * d.max()
    return abs(E.max() - reltol) / reltol, (np.abs(d - half).min() / half if half > 0 else np.inf)


def greedy(estimates_at, start, reltol, max_rounds=16):
    """The greedy run from `start`: estimates_at(S) -> [K, n_save] (every member's estimate at every save point under the counts S, Richardson's factor
    applied).  Returns (verdict, S, per-member estimates [K] of the last round, rounds), rounds = [(S, est, est margin, interval margin)]."""
    S, prev, rounds = [int(s) for s in start], -1.0, []
    for _ in range(max_rounds):
        est = np.asarray(estimates_at(tuple(S)), np.float64)
        E = est.max(axis=0)
        at = tuple(S)
        verdict, mx, S = choose_round(E, reltol, prev, S)
        rounds.append((at, mx) + margins(E, reltol))
        if verdict != DOUBLED:
            return verdict, tuple(S), est.max(axis=1), rounds
        prev = mx
    raise AssertionError("the greedy run did not end in %d rounds" % max_rounds)


def clear_of_thresholds(rounds):
    """every round of a run: the estimate not within 5 % of reltol, and no interval's addition within 5 % of half the largest"""
    return all(m_est > 0.05 and m_iv > 0.05 for _, _, m_est, m_iv in rounds)


def oracle_estimates(monkeypatch, p, W, physics, factor=FACTOR_RK4, floor=1e-3):
    """estimates_at for `greedy` on the float64 oracle: every member solved under S and under 2 S (tests/schedule_common.oracle_schedule)"""
    from oracle import nde_oracle as O
    cfgs = member_cfgs(p.cfg, physics)

    def solve(S):
        C.oracle_schedule(monkeypatch, S)
        return np.stack([O.solve(c, p.x0, p.bcs, w) for c, w in zip(cfgs, W)])

    def estimates_at(S):
        a, b = solve(S), solve(tuple(2 * s for s in S))
        return C.estimate_norm(a, b, factor, floor).max(axis=1)             # [K][column][save point] -> [K][save point]
    return estimates_at
