"""Shared inputs of the `--conv` network tests (tests/test_conv_layout.py, tests/test_gpu_conv.py): the three CPU-checked problems and the float64
oracle run, unchanged, on the equivalent four-layer Toeplitz network with its gradient folded back onto the conv parameter vector."""
import functools

import numpy as np

from colnde import synthetic
from colnde.free_convection import conv_dense_layer_sizes, conv_grad_from_dense, conv_to_dense
from oracle import nde_oracle as O

# name -> (Nz, c, keyword arguments of synthetic.free_convection_conv_problem)
CPU_CHECKED = {
    "fc/32/c3": (32, 3, dict(weight_divisor=10.0, t_end=1.0, n_save=3, substeps=2)),
    "ca/32/c8": (32, 8, dict(weight_divisor=1.0, t_end=0.004, n_save=3, substeps=15, convective_adjustment=True)),
    "ca/64/c2": (64, 2, dict(weight_divisor=10.0, t_end=0.001, n_save=3, substeps=15, convective_adjustment=True)),
}
FC_KW = CPU_CHECKED["fc/32/c3"][2]


def dense_cfg(cfg, c):
    """The configuration of the four-layer network `conv_to_dense` writes (what tile16 and the oracle run)."""
    return cfg.with_(layer_sizes=conv_dense_layer_sizes(cfg.Nz, c), activations=("relu", "relu", "relu", "identity"))


def oracle_loss_grad(cfg, c, x0, bcs, theta, truth, dtype=np.float64):
    """(total, folded gradient, sol) of the oracle on conv_to_dense(theta)."""
    dc = dense_cfg(cfg, c)
    sc = O.default_loss_scalings(dc)
    tot, _, g, sol = O.loss_and_grad(dc, x0, bcs, conv_to_dense(np.asarray(theta, np.float64), cfg.Nz, c), truth, sc, dtype=dtype)
    return tot, conv_grad_from_dense(g, cfg.Nz, c), sol


@functools.lru_cache(maxsize=None)
def reference(Nz, c, ncol, kw_items, stepper="rk4"):
    """Problem, truth and the oracle's (total, folded gradient, sol), computed once per case and shared (read-only)."""
    p = synthetic.free_convection_conv_problem(ncol, c, Nz=Nz, **dict(kw_items))
    cfg = p.cfg.with_(stepper=stepper) if stepper != "rk4" else p.cfg
    dc = dense_cfg(cfg, c)
    truth = O.solve(dc, p.x0, p.bcs, conv_to_dense(p.weights_truth.astype(np.float64), Nz, c)).astype(np.float32)
    tot, g, sol = oracle_loss_grad(cfg, c, p.x0, p.bcs, p.weights, truth)
    for a in (truth, g, sol, p.x0, p.bcs, p.weights):
        a.setflags(write=False)
    return p, cfg, truth, tot, g, sol


def kw_items(kw):
    return tuple(sorted(kw.items()))


def blocks(Nz, c):
    """(name, start, stop) of the conv parameter vector's blocks."""
    H, M = 4 * Nz, Nz - c + 1
    out, off = [], 0
    for name, n in (("filter_w", c), ("filter_b", 1), ("W1", H * M), ("b1", H), ("W2", H * H), ("b2", H), ("W3", H * (Nz - 1)), ("b3", Nz - 1)):
        out.append((name, off, off + n))
        off += n
    return out
