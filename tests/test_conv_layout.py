"""The parameter layout of the free-convection driver's `--conv` network (train_free_convection_nde.jl:110-122) and its reference: the float64
oracle run unchanged on the equivalent four-layer Toeplitz network, its gradient folded onto the c + 1 filter entries.  No GPU."""
import numpy as np
import pytest

from colnde import synthetic
from colnde.free_convection import conv_dense_layer_sizes, conv_grad_from_dense, conv_n_params, conv_to_dense
from oracle import nde_oracle as O
from tests.conv_cases import CPU_CHECKED, blocks, dense_cfg, kw_items, oracle_loss_grad, reference


@pytest.mark.parametrize("Nz,c", [(32, 2), (32, 3), (32, 8), (64, 2), (64, 5)])
def test_conv_n_params(Nz, c):
    M, H = Nz - c + 1, 4 * Nz
    assert conv_n_params(Nz, c) == c + 1 + H * M + H + H * H + H + H * (Nz - 1) + Nz - 1
    assert blocks(Nz, c)[-1][2] == conv_n_params(Nz, c)
    plain = H * Nz + H + H * H + H + H * (Nz - 1) + Nz - 1
    assert conv_n_params(Nz, c) == c + 1 + plain - H * (c - 1)          # the engine's padded vector drops 4Nz (c - 1) zeros, gains the filter
    p = synthetic.free_convection_conv_problem(3, c, Nz=Nz, n_save=3)
    assert p.weights.shape == (conv_n_params(Nz, c),) and p.cfg.layer_sizes == (Nz, H, H, Nz - 1)
    assert p.weights[c] == np.float32(0.05)


@pytest.mark.parametrize("Nz,c", [(32, 3), (64, 5)])
def test_conv_to_dense_is_the_toeplitz_network(Nz, c):
    rng = np.random.default_rng(5)
    theta = rng.standard_normal(conv_n_params(Nz, c))
    M = Nz - c + 1
    d = conv_to_dense(theta, Nz, c)
    assert conv_dense_layer_sizes(Nz, c) == (Nz, M, 4 * Nz, 4 * Nz, Nz - 1)
    assert d.shape == (M * Nz + M + theta.size - (c + 1),)
    W0 = d[:M * Nz].reshape((M, Nz), order="F")
    x = rng.standard_normal(Nz)
    w, b = theta[:c], theta[c]
    y = np.array([b + sum(w[k - 1] * x[(i + c - k) - 1] for k in range(1, c + 1)) for i in range(1, M + 1)])      # the spec, 1-based
    np.testing.assert_allclose(W0 @ x + d[M * Nz:M * Nz + M], y, rtol=1e-13, atol=1e-13)
    assert np.count_nonzero(W0) == M * c
    np.testing.assert_array_equal(d[M * Nz + M:], theta[c + 1:])


@pytest.mark.parametrize("Nz,c", [(32, 2), (32, 8), (64, 5)])
def test_conv_grad_from_dense_is_the_transpose_of_conv_to_dense(Nz, c):
    """<conv_to_dense'(θ) δ, g> = <δ, conv_grad_from_dense(g)>: conv_to_dense is linear, so its value on δ is its derivative."""
    rng = np.random.default_rng(6)
    n = conv_n_params(Nz, c)
    delta = rng.standard_normal(n)
    M = Nz - c + 1
    g = rng.standard_normal(M * Nz + M + n - (c + 1))
    lhs = conv_to_dense(delta, Nz, c) @ g
    rhs = delta @ conv_grad_from_dense(g, Nz, c)
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + 1.0)
    with pytest.raises(ValueError):
        conv_to_dense(delta[:-1], Nz, c)
    with pytest.raises(ValueError):
        conv_grad_from_dense(g[:-1], Nz, c)


@pytest.mark.parametrize("case", sorted(CPU_CHECKED))
def test_folded_oracle_gradient_agrees_with_finite_differences_on_the_filter(case):
    """All c + 1 filter entries of the three CPU-checked inputs: central differences of the oracle's loss, step 1e-6 in float64, rel < 1e-4
    (40x the worst value measured: 1e-8 ... 2.5e-6)."""
    Nz, c, kw = CPU_CHECKED[case]
    p, cfg, truth, tot, g, sol = reference(Nz, c, 3, kw_items(kw))
    # the inputs are sane for the oracle itself: scaled temperatures start within +-1.6 and stay O(10); a solve that leaves the stable regime
    # (weight_divisor = 1 with t_end = 1) reaches 1e4 ... 1e7
    assert np.isfinite(tot) and np.isfinite(g).all() and np.abs(sol).max() < 100.0
    dc = dense_cfg(cfg, c)
    sc = O.default_loss_scalings(dc)
    theta = p.weights.astype(np.float64)

    def loss(t):
        return O.loss(dc, O.solve(dc, p.x0, p.bcs, conv_to_dense(t, Nz, c)), truth, sc)[0]

    h = 1e-6
    for k in range(c + 1):
        e = np.zeros_like(theta)
        e[k] = h
        fd = (loss(theta + e) - loss(theta - e)) / (2 * h)
        print("%s entry %d: folded %.9e, finite difference %.9e, rel %.2e" % (case, k, g[k], fd, abs(g[k] - fd) / abs(fd)))
        assert abs(g[k] - fd) < 1e-4 * abs(fd), (k, g[k], fd)
    # the filter block is a visible part of the gradient, and both relu branches of the filter are exercised
    assert 1e-5 < np.linalg.norm(g[:c + 1]) / np.linalg.norm(g) < 1.0
