"""CPU checks of the wind-mixing embedded inference (wind_mixing/src/NDE_oceananigans.jl:288-329): the float64 restatement the GPU
tests are held to (tests/wm_embed_common.py) against a scalar-loop restatement and a hand-worked case, and the Python argument checks."""
import math

import numpy as np
import pytest

from colnde import synthetic
from colnde.nde import check_wm_embed_arrays
from tests import wm_embed_common as W


def _act(name, z):
    if name == "identity":
        return z
    if name == "relu":
        return max(z, 0.0)
    if name == "mish":
        return z * math.tanh(math.log1p(math.exp(z)))
    if name == "swish":
        return z / (1.0 + math.exp(-z))
    if name == "tanh":
        return math.tanh(z)
    if name == "leakyrelu":
        return z if z > 0 else 0.01 * z
    raise KeyError(name)


def _scalar_dz_fluxes(cfg, weights, u, v, T, top, Lz):
    """:288-329 once more, one column and one number at a time, reading the flat Flux.destructure vector directly."""
    Nz, sizes, acts = cfg.Nz, cfg.layer_sizes, cfg.activations
    w = [float(x) for x in weights]
    n = len(u)
    net_size = sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1))
    out = [[[0.0] * Nz for _ in range(n)] for _ in range(3)]
    dz = Lz / Nz
    for c in range(n):
        x = [(float(u[c][k]) - cfg.mu[0]) / cfg.sigma[0] for k in range(Nz)]
        x += [(float(v[c][k]) - cfg.mu[1]) / cfg.sigma[1] for k in range(Nz)]
        x += [(float(T[c][k]) - cfg.mu[2]) / cfg.sigma[2] for k in range(Nz)]
        for net in range(3):
            a, o = x, net * net_size
            for l in range(len(sizes) - 1):
                ni, no = sizes[l], sizes[l + 1]
                z = []
                for j in range(no):
                    acc = 0.0
                    for i in range(ni):
                        acc += w[o + i * no + j] * a[i]                      # vec(W[out x in]) column-major
                    z.append(_act(acts[l], acc + w[o + ni * no + j]))
                a, o = z, o + ni * no + no
            s, m = cfg.sigma[3 + net], cfg.mu[3 + net]
            if net < 2:
                un = [s * y + m for y in a]
                first = s * un[0] + m                                       # inv(scaling) of the already unscaled first element (sic)
                interior = [q - first for q in un]
            else:
                interior = [(s * y + m) - (s * a[0] + m) for y in a]
            F = [0.0] + interior + [float(top[net][c])]
            for k in range(Nz):
                out[net][c][k] = (F[k + 1] - F[k]) / dz
    return [np.array(o) for o in out]


@pytest.mark.parametrize("acts", [("mish", "mish", "identity"), ("relu", "tanh", "identity")])
def test_restatement_matches_scalar_loops(acts):
    p = synthetic.wind_mixing_problem(5, n_frames=3, weight_divisor=1.0, activations=acts)
    u, v, T, top = W.embed_inputs(p)
    got = W.dz_fluxes(p.cfg, p.weights_truth, u, v, T, top, W.LZ)
    want = _scalar_dz_fluxes(p.cfg, p.weights_truth, u, v, T, top, W.LZ)
    for g, w in zip(got, want):
        assert g.shape == (5, 32)
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * np.abs(w).max())


def test_hand_worked_identity_nets_Nz4():
    """Nz = 4, one Dense(12, 3, identity) per net picking x[0:3] (uw), x[4:7] (vw), x[8:11] (wT), zero bias; μ = 0 except μ_uw = 1,
    σ = 1 except σ_uw = 2, σ_wT = 3; Lz = 4 (Δz = 1)."""
    cfg = synthetic.wind_mixing_problem(1, Nz=4, n_frames=3, layer_sizes=(12, 3), activations=("identity",)).cfg.with_(
        mu=(0.0, 0.0, 0.0, 1.0, 0.0, 0.0), sigma=(1.0, 1.0, 1.0, 2.0, 1.0, 3.0))
    nets = []
    for k in range(3):
        Wm = np.zeros((3, 12))
        for j in range(3):
            Wm[j, 4 * k + j] = 1.0
        nets.append(np.concatenate([Wm.reshape(-1, order="F"), np.zeros(3)]))
    u, v, T = np.array([[1.0, 2.0, 4.0, 0.0]]), np.array([[3.0, 5.0, 6.0, 0.0]]), np.array([[2.0, 3.0, 7.0, 0.0]])
    top = np.array([[10.0], [20.0], [30.0]])
    dzu, dzv, dzT = W.dz_fluxes(cfg, np.concatenate(nets), u, v, T, top, 4.0)
    # uw: y = (1, 2, 4), a = 2y + 1 = (3, 5, 9), minus (2*3 + 1) = 7: (-4, -2, 2); faces (0, -4, -2, 2, 10)
    np.testing.assert_allclose(dzu[0], [-4.0, 2.0, 4.0, 8.0], rtol=0, atol=1e-14)
    # vw: y = a = (3, 5, 6), minus (1*3 + 0) = 3: (0, 2, 3); faces (0, 0, 2, 3, 20)
    np.testing.assert_allclose(dzv[0], [0.0, 2.0, 1.0, 17.0], rtol=0, atol=1e-14)
    # wT: 3 (y - y[0]) = (0, 3, 15); faces (0, 0, 3, 15, 30)
    np.testing.assert_allclose(dzT[0], [0.0, 3.0, 12.0, 15.0], rtol=0, atol=1e-14)


def test_python_shape_and_alias_validation():
    n, Nz = 6, 32
    f = lambda *s: np.zeros(s, np.float32)
    u, v, T, top, hb = f(n, Nz), f(n, Nz), f(n, Nz), f(3, n), f(3, n)
    dz, out = tuple(f(n, Nz) for _ in range(3)), tuple(f(n, Nz) for _ in range(3))
    check_wm_embed_arrays(Nz, n, (u, v, T), top, hb, dz, out)
    check_wm_embed_arrays(Nz, n, (u, v, T), top, None, dz, (u, v, T))                    # in place, field by field
    with pytest.raises(ValueError, match="u: expected shape"):
        check_wm_embed_arrays(Nz, n, (f(n, Nz + 1), v, T), top)
    with pytest.raises(ValueError, match="T: expected shape"):
        check_wm_embed_arrays(Nz, n, (u, v, f(n + 1, Nz)), top)
    with pytest.raises(ValueError, match="top_flux: expected shape"):
        check_wm_embed_arrays(Nz, n, (u, v, T), f(n, 3))
    with pytest.raises(ValueError, match="halo_bottom: expected shape"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, f(3, n + 1))
    with pytest.raises(ValueError, match="dz_vw: expected shape"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, None, (dz[0], f(n, 31), dz[2]))
    with pytest.raises(ValueError, match="dz_uw overlaps u"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, None, (u, dz[1], dz[2]))
    with pytest.raises(ValueError, match="dz_uw overlaps dz_wT"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, None, (dz[0], dz[1], dz[0]))
    with pytest.raises(ValueError, match="u_out overlaps v"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, None, dz, (v, out[1], out[2]))        # an output on ANOTHER field's input
    with pytest.raises(ValueError, match="dz_wT overlaps T_out"):
        check_wm_embed_arrays(Nz, n, (u, v, T), top, None, dz, (out[0], out[1], dz[2]))
    big = f(2 * n, Nz)
    with pytest.raises(ValueError, match="v_out overlaps v"):                             # a shifted window onto its own input is not "in place"
        check_wm_embed_arrays(Nz, n, (u, big[:n], T), top, None, dz, (out[0], big[1:n + 1], out[2]))
    try:
        import torch
    except ImportError:
        return
    tu, tdz = torch.zeros(n, Nz), tuple(torch.zeros(n, Nz) for _ in range(3))
    check_wm_embed_arrays(Nz, n, (tu, torch.zeros(n, Nz), torch.zeros(n, Nz)), torch.zeros(3, n), None, tdz, None)
    with pytest.raises(ValueError, match="dz_vw overlaps u"):
        check_wm_embed_arrays(Nz, n, (tu, torch.zeros(n, Nz), torch.zeros(n, Nz)), torch.zeros(3, n), None, (tdz[0], tu, tdz[2]), None)
