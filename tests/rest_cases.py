"""Columns at rest — the degenerate states of the Richardson-number closure, built once.  A helper, not a test: shared by
tests/test_rest_cases_host.py and tests/test_gpu_rest_columns.py.

LES columns start from rest: u = v = 0 at t = 0, and below the mixed layer for the whole run.  The training right-hand sides add ε = 1e-7 to the
three gradients (NDE_training.jl:115-119), so a resting face has S2 = 2 (σ_u ε)² = 5e-17 and Ri ~ ±1e15; the embedding (NDE_oceananigans.jl:17-58)
has no ε and sees +Inf, −Inf or 0/0 there.  `synthetic.wind_mixing_problem` adds noise to every level of u and v, so none of its faces is at rest.

`rest_state(p)` edits a copy of such a problem; the columns cycle through four kinds by `column % 4`.  Every edit is an assignment of a float32
value or one float32 subtraction: exact.  μ_u = μ_v = 0, so scaled 0 is physical 0.
    kind 0  the whole column at rest; T levels 20..23 lowered by 0.05 K, so that the resting face 20 is unstably stratified
            (Ri → −huge / −Inf, ν = ν₀ + ν₋) and every other face is stable (Ri → +huge / +Inf, ν = ν₀)
    kind 1  levels 0..15 at rest under the generated sheared upper half: Ri → +huge / +Inf on faces 1..15
    kind 2  as kind 1, plus T[4..8] = T[4]: a neutral layer at rest.  Training: Ri = B ε / S2 > 0; embedding: 0/0 on faces 5..8
    kind 3  untouched except T[10] = T[9]: a sheared face with Ri == 0 exactly (`Ri > 0` is false: ν_T = 1 under convective adjustment);
            the rest of the column is the control
Level numbers are those of Nz = 32; at another Nz the resting half is Nz/2 levels and the lowered levels start at 5 Nz/8 (`rest_top`,
`unstable_levels`); the neutral layer and the zero face keep their levels (Nz >= 16)."""
from dataclasses import dataclass, replace

import numpy as np

from tests import wm_embed_common as W

DT_UNSTABLE = 0.05           # K
NEUTRAL = slice(4, 9)        # kind 2: T[4..8] = T[4]
NEUTRAL_FACES = slice(5, 9)  # ... the faces between those levels
ZERO_FACE = 10               # kind 3: T[10] = T[9]
MIN_SHEAR = 1e-6             # m/s: the face differences of u and v are both exactly zero, or the larger is at least this
MIN_COMPONENT = 1e-12        # m/s: ... and the smaller is zero or at least this


def rest_top(Nz):
    """kinds 1, 2: levels 0 .. rest_top − 1 are at rest (16 of 32)"""
    return Nz // 2


def unstable_levels(Nz):
    """kind 0: the four levels lowered by DT_UNSTABLE (20..23 of 32)"""
    return slice(5 * Nz // 8, 5 * Nz // 8 + 4)


@dataclass
class RestState:
    p: object                # the edited ColumnProblem (x0 edited, everything else shared with the original)
    u: np.ndarray            # ocean-unit view, wm_embed_common.embed_inputs of the edited problem: [n, Nz] float32
    v: np.ndarray
    T: np.ndarray
    top: np.ndarray          # [3, n]
    halo_bottom: np.ndarray  # [3, n], wm_diag_restatement.diag_inputs' pattern
    halo_top: np.ndarray
    kind: np.ndarray         # [n] int: column % 4

    def mask(self, k):
        return self.kind == k


def rest_state(p):
    Nz = p.cfg.Nz
    n = p.x0.shape[0]
    assert Nz >= 16 and p.cfg.mu[0] == 0.0 and p.cfg.mu[1] == 0.0
    top_rest, unstable = rest_top(Nz), unstable_levels(Nz)
    x0 = p.x0.copy()
    assert x0.dtype == np.float32
    u, v, T = x0[:, :Nz], x0[:, Nz:2 * Nz], x0[:, 2 * Nz:]          # views
    kind = np.arange(n) % 4
    k0, k12, k2, k3 = kind == 0, (kind == 1) | (kind == 2), kind == 2, kind == 3
    u[k0] = 0.0
    v[k0] = 0.0
    T[k0, unstable] -= np.float32(DT_UNSTABLE / p.cfg.sigma[2])
    u[k12, :top_rest] = 0.0
    v[k12, :top_rest] = 0.0
    T[k2, NEUTRAL] = T[k2, NEUTRAL.start][:, None]
    T[k3, ZERO_FACE] = T[k3, ZERO_FACE - 1]
    q = replace(p, x0=x0)
    uo, vo, To, top = W.embed_inputs(q)
    # shear is exactly zero or what synthetic generated: on every face Δu = Δv = 0, or the larger of the two is at least MIN_SHEAR and neither
    # square underflows in float32 (nonzero |Δ| >= MIN_COMPONENT: Δ² >= 1e-24 >> 1.2e-38), so float32 and float64 agree on where S2 == 0
    du, dv = (np.abs(np.diff(a.astype(np.float64), axis=1)) for a in (uo, vo))
    big = np.maximum(du, dv)
    assert ((big == 0) | (big >= MIN_SHEAR)).all(), big[(big != 0) & (big < MIN_SHEAR)]
    for d in (du, dv):
        assert ((d == 0) | (d >= MIN_COMPONENT)).all()
    assert not uo[k0].any() and not vo[k0].any() and not uo[k12, :top_rest].any() and not vo[k12, :top_rest].any()
    c = np.arange(n)
    hb = np.stack([uo[:, 0] - 1e-3, vo[:, 0] + 2e-3, To[:, 0] + np.where(c % 2, 0.01, -0.01)]).astype(np.float32)
    ht = np.stack([uo[:, -1] + 2e-3, vo[:, -1] - 1e-3, To[:, -1] + np.where((c // 2) % 2, 0.01, -0.01)]).astype(np.float32)
    return RestState(q, uo, vo, To, top, np.ascontiguousarray(hb), np.ascontiguousarray(ht), kind)


def rest_closure_problem(n_columns, sets, Nz=32, n_frames=5, **kw):
    """The closure-only problem of tests/closure_common.closure_problem with the edit applied: (RestState, truth), sub-steps from
    `colnde.closure_min_substeps` over `sets`, truth = the float64 solve of the EDITED columns with the constants TRUTH, stored as float32."""
    import colnde
    from colnde import synthetic
    from oracle import nde_oracle as O
    from tests import closure_common as C
    if Nz != 32:
        kw.setdefault("layer_sizes", (3 * Nz, 50, 20, Nz - 1))
    p = synthetic.wind_mixing_problem(n_columns, Nz=Nz, n_frames=n_frames, **kw)
    need = max(colnde.closure_min_substeps(p.cfg, s) for s in sets)
    if need > p.cfg.substeps:
        p = synthetic.wind_mixing_problem(n_columns, Nz=Nz, n_frames=n_frames, **dict(kw, substeps=need))
    rs = rest_state(p)
    truth = O.solve(C.with_params(rs.p.cfg, C.TRUTH), rs.p.x0, rs.p.bcs, np.zeros(rs.p.cfg.n_params)).astype(np.float32)
    return rs, truth
