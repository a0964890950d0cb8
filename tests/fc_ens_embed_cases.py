"""Shared inputs, float64 references and tolerances of the ensemble free-convection embedding tests (tests/test_fc_ens_embed_host.py,
tests/test_gpu_fc_ens_embed.py).  A helper, not a test.

Members: K = 3 networks per kind with weights / 1e2 (the nets matter) — plain fc32, or `--conv c` (c = 2, 3, 8) with filter taps
U(-1, 1) sqrt(6 / (c + 1)) and a bias that centres the pre-activation near zero (both relu branches in every column), different per member.
States: member k has its own 33 columns of fc_embed_restatement.switch_robust_case (seed + k), the first n per case; the top flux is
member 0's, shared.  Lz = 1000, dt = 600.
K_ca = 10 with the step (c K = dt K / dz² of 6 ... 25: a strong adjustment), K_ca = 1e-3 for the diagnosis alone (κ ∂T/∂z of the size of the
network's flux, so an error in the network shows in the faces).

Tolerances.  Plain members keep the single-model bounds (tests/test_gpu_fc_embed.py): ∂z wT relative L2 2e-6, T′ 2e-5 of max|T′|,
faces 10 x the distance of the float32 NumPy restatement from the float64 one.  Conv members: T′ as plain (the sweep never sees the filter);
∂z wT and faces 10 x the float32 restatement's own distance from float64 on the conv_to_dense network — the project's rule.  `distances()`
measures those figures on the CPU; tests/test_fc_ens_embed_host.py asserts that they stay within a tenth of the bounds below.  Measured
(largest over Nz = 32 | 64, halos given / absent, the members and, conv, c = 2 | 3 | 8):
    plain  faces      K_ca = 10: 8.33e-8    K_ca = 1e-3: 1.30e-7
    conv   faces      K_ca = 10: 8.33e-8    K_ca = 1e-3: 1.36e-7
    conv   dz_wT (relative L2):  3.84e-8    (plain: 4.78e-8, against its fixed 2e-6)
"""
import functools

import numpy as np

from colnde import synthetic
from colnde.free_convection import conv_n_params, conv_to_dense
from tests import fc_embed_restatement as R
from tests.conv_cases import dense_cfg

LZ, DT = 1000.0, 600.0
K_STEP, K_DIAG = 10.0, 1e-3
K_MODELS, N_ALL = 3, 33
SIZES = (1, 16, 19)                  # one lane of a tile, a full tile, a partial second tile; N_ALL (a third tile) runs once
CONVS = (2, 3, 8)
T_TOL, DZ_REL_PLAIN = 2e-5, 2e-6
# 10 x the figures of the docstring
FACES_BOUND = {("plain", K_STEP): 8.33e-7, ("plain", K_DIAG): 1.30e-6, ("conv", K_STEP): 8.33e-7, ("conv", K_DIAG): 1.36e-6}
DZ_REL_CONV = 3.84e-7


@functools.lru_cache(maxsize=None)
def config(Nz):
    return synthetic.free_convection_problem(4, Nz=Nz, n_save=3, substeps=2, t_end=0.01).cfg


@functools.lru_cache(maxsize=None)
def weights(Nz, c=0):
    """[K, n_params] float32: K different members — plain (c = 0) or `--conv c`."""
    cfg = config(Nz)
    rows = []
    for k in range(K_MODELS):
        if not c:
            rows.append(synthetic.make_weights(synthetic._rng(411, k), cfg, 1e2))
            continue
        r = synthetic._rng(412 + c, k)
        filt = r.uniform(-1.0, 1.0, size=c) * np.sqrt(6.0 / (c + 1))
        dense = synthetic.make_weights(r, cfg.with_(layer_sizes=(Nz - c + 1, 4 * Nz, 4 * Nz, Nz - 1)), 1e2)
        # The states have column mean 15, a scaled input of (19.65 + 15/20 − μ_T)/σ_T everywhere plus the profile's variation: with this bias the
        # filter's pre-activation is centred on 0.05, so both relu branches are taken within every column (asserted in test_fc_ens_embed_host.py)
        x_mean = (19.65 + 15.0 / 20.0 - cfg.mu[2]) / cfg.sigma[2]
        rows.append(np.concatenate([filt, [0.05 - filt.sum() * x_mean], dense]))
    W = np.ascontiguousarray(np.stack(rows), dtype=np.float32)
    assert W.shape == (K_MODELS, conv_n_params(Nz, c) if c else cfg.n_params)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def states(Nz):
    """float32 (T [K, N_ALL, Nz], top [N_ALL] shared, halo_bottom [K, N_ALL], halo_top [K, N_ALL])."""
    per = [R.switch_robust_case(Nz, N_ALL, seed=20261020 + k) for k in range(K_MODELS)]
    out = (np.stack([p[0] for p in per]), per[0][1].copy(), np.stack([p[2] for p in per]), np.stack([p[3] for p in per]))
    for a in out:
        a.setflags(write=False)
    return out


def case(Nz, n):
    T, top, hb, ht = states(Nz)
    return tuple(np.ascontiguousarray(a) for a in (T[:, :n], top[:n], hb[:, :n], ht[:, :n]))


def oracle_network(Nz, c, k):
    """(configuration, θ) the float64 restatement evaluates for member k: the plain network, or `conv_to_dense` of the conv member."""
    cfg, w = config(Nz), weights(Nz, c)[k]
    return (cfg, w) if not c else (dense_cfg(cfg, c), conv_to_dense(w, Nz, c))


@functools.lru_cache(maxsize=None)
def reference(Nz, c, K_ca, halo, dtype=np.float64):
    """(∂z wT, T′, faces), each [K, N_ALL, ..]: fc_embed_restatement on every member's N_ALL columns, computed once and shared (read-only)."""
    T, top, hb, ht = states(Nz)
    rows = []
    for k in range(K_MODELS):
        cfg, w = oracle_network(Nz, c, k)
        rows.append(R.embedded_step(cfg, w.astype(dtype), T[k].astype(dtype), top.astype(dtype), LZ, DT, K_ca,
                                    (hb[k].astype(dtype), ht[k].astype(dtype)) if halo else None, dtype))
    out = tuple(np.stack([r[i] for r in rows]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def faces_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def same_switches(T, halos):
    """float32 and float64 take the same κ switches in EVERY column of every member: the GPU comparison excludes no column."""
    for k in range(T.shape[0]):
        h32 = None if halos is None else tuple(a[k] for a in halos)
        h64 = None if halos is None else tuple(a[k].astype(np.float64) for a in halos)
        assert np.array_equal(R.centred_switch(T[k], h32), R.centred_switch(T[k].astype(np.float64), h64))
        assert np.array_equal(R.face_switch(T[k], h32), R.face_switch(T[k].astype(np.float64), h64))


@functools.lru_cache(maxsize=None)
def distances():
    """The float32 NumPy restatement's own distance from float64 on these inputs: {("plain" | "conv", "faces", K_ca) | ("conv", "dz"): figure}, the
    largest over Nz, halos, members (per member, as the GPU test compares) and c."""
    out = {}

    def up(key, v):
        out[key] = max(out.get(key, 0.0), v)
    for Nz in (32, 64):
        for c in (0,) + CONVS:
            kind = "conv" if c else "plain"
            for halo in (False, True):
                for K_ca in (K_STEP, K_DIAG):
                    r64, r32 = reference(Nz, c, K_ca, halo), reference(Nz, c, K_ca, halo, np.float32)
                    for k in range(K_MODELS):
                        up((kind, "faces", K_ca), faces_err(r32[2][k], r64[2][k]))
                        up((kind, "dz"), rel_l2(r32[0][k], r64[0][k]))
    return out
