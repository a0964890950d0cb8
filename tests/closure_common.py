"""Shared by tests/test_closure_host.py and tests/test_gpu_closure.py: the closure-only problem (theta = 0), its float64 yardstick
(`O.solve` / `O.loss`) and the central finite difference of that loss with respect to the five Pacanowski-Philander constants."""
import numpy as np

from colnde import synthetic
from oracle import nde_oracle as O

KEYS = ("nu0", "nu_minus", "dRi", "Ric", "Pr")
TRUTH = (2e-4, 0.06, 0.6, 0.35, 1.4)            # the constants the truth trajectories are generated with
FD_REL_STEP = 1e-6


def with_params(cfg, p):
    return cfg.with_(**{k: float(v) for k, v in zip(KEYS, p)})


def cfg_params(cfg):
    return np.array([getattr(cfg, k) for k in KEYS], dtype=np.float64)


def closure_problem(n_columns, Nz=32, n_frames=5, substeps=2, **kw):
    """(problem, theta = 0, truth): truth = the float64 solve with the constants TRUTH, stored as float32 (what the handle receives)."""
    if Nz != 32:
        kw.setdefault("layer_sizes", (3 * Nz, 50, 20, Nz - 1))       # only so that validate() passes: the closure model has no networks
    p = synthetic.wind_mixing_problem(n_columns, Nz=Nz, n_frames=n_frames, substeps=substeps, **kw)
    theta0 = np.zeros(p.cfg.n_params)
    truth = O.solve(with_params(p.cfg, TRUTH), p.x0, p.bcs, theta0).astype(np.float32)
    return p, theta0, truth


def f64_solve(cfg, p, params):
    return O.solve(with_params(cfg, params), p.x0, p.bcs, np.zeros(cfg.n_params))


def f64_loss(cfg, p, truth, params, scalings, n_col_total=None):
    """(total, scaled terms) in float64; n_col_total: the global column count a shard is normalised by."""
    tot, terms = O.loss(cfg, f64_solve(cfg, p, params), truth, scalings)
    if n_col_total is not None:
        f = p.x0.shape[0] / float(n_col_total)
        tot, terms = tot * f, terms * f
    return tot, terms


def fd_grad(cfg, p, truth, params, scalings, rel=FD_REL_STEP, n_col_total=None):
    """Central finite difference of the float64 loss with respect to the five constants, relative step `rel`."""
    params = np.asarray(params, np.float64)
    g = np.zeros(5)
    for q in range(5):
        h = rel * params[q]
        a, b = params.copy(), params.copy()
        a[q] += h
        b[q] -= h
        g[q] = (f64_loss(cfg, p, truth, a, scalings, n_col_total)[0] - f64_loss(cfg, p, truth, b, scalings, n_col_total)[0]) / (2 * h)
    return g
