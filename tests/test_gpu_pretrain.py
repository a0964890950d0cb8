"""`pretrain_kernel` (csrc/engine_tile16.hip, `colnde_pretrain_flux_dev`) held to the float64 oracle directly: the loss and the GRADIENT of one
sample read out of the ADAM moments (A, at every shape of tests/pretrain_cases.py: B), the sequence semantics of a pass (C) and the refusals (D).
tests/test_pretrain.py keeps the 48-step trajectory test; ADAM's update eta m^/(sqrt(v^) + eps) is scale-invariant in g, so a trajectory cannot see
a gradient that is wrong by a factor — the moments can.

Tolerances: 10x what float32 alone costs for this arithmetic, measured WITHOUT the kernel by the float32 restatement of tests/pretrain_cases.py, largest
over all cases, rounded up to two digits (tests/test_pretrain.py::test_float32_restatement_* holds each constant below between 10x and 12x its
measurement).  Beside each: the restatement's largest error / the kernel's largest error on an MI355X."""
import ctypes

import numpy as np
import pytest

import colnde
from colnde.flux_compat import ADAM
from tests import pretrain_cases as PC

pytestmark = pytest.mark.gpu

#                      float32 restatement (CPU)   kernel (MI355X)
TOL_LOSS = 3.5e-6    # 3.47e-7  (L1_tanh)          2.59e-7  (96-400-400-31_swish)
TOL_W = 7.3e-6       # 7.30e-7  (96-600-31_relu)   1.32e-6  (fc_Nz64_7x800_lds68k)
TOL_B = 7.3e-6       # 7.26e-7  (96-600-31_relu)   1.32e-6  (fc_Nz64_7x800_lds68k)
# one pass of the real ADAM(1e-3): SEQ_ORDER, 0..7 and a single sample; largest over the layer blocks
TOL_M = 2.8e-6       # 2.71e-7                     3.99e-7
TOL_V = 4.6e-6       # 4.57e-7                     5.15e-7
TOL_THETA = 9.3e-7   # 9.24e-8  relative to |theta|: mostly the rounding of theta itself                  9.45e-8
TOL_MOVED = 6.4e-5   # 6.32e-6  relative to |theta - theta_0|, the distance the pass moved the block      6.32e-6
# exact bounds: bit equality, and one ulp for v (see test_single_sample_loss_and_gradient)

F32_TINY = float(np.finfo(np.float32).tiny)


def _t(a, dt=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(torch.device("cuda", 0))


def _np(t):
    return t.detach().cpu().numpy()


def _dev_sample(s):
    return _t(s.X), _t(s.B), _t(s.Y)


SENTINEL = 7.0      # in the moments of the nets not trained: whatever touches them shows


def _moments(s):
    m = np.full(s.cfg.n_params, SENTINEL, np.float32)
    m[s.net] = 0.0
    return m


def _others(s):
    o = np.ones(s.cfg.n_params, bool)
    o[s.net] = False
    return o


# ---- A / B ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(PC.CASES))
def test_single_sample_loss_and_gradient(case):
    """One call with one sample, zero moments, beta1 = beta2 = 0.5, beta_t = (0.5, 0.5) and eta = 0: m = g/2 exactly, so g = 2 m; v = fl(g g)/2,
    which ties v to the SAME g as m to the last bit (halving is exact; a result in the subnormal range may be flushed); theta keeps its bits."""
    s = PC.sample(case)
    loss_ref, g_ref = PC.reference(case)
    cfg = s.cfg
    X, B, Y = _dev_sample(s)
    theta, m, v = _t(s.theta), _t(_moments(s)), _t(_moments(s))
    opt = ADAM(0.0, (0.5, 0.5))
    opt.beta_t = [0.5, 0.5]
    with colnde.ColumnNDE(cfg, 1) as eng:
        loss = eng.pretrain_flux(s.k, theta, m, v, X, B, Y, None, s.gs, opt)
    theta, m, v = _np(theta), _np(m), _np(v)
    g = (np.float32(2) * m[s.net]).astype(np.float32)
    errs = PC.block_errors(cfg, g, g_ref)
    e_loss = abs(loss - loss_ref) / loss_ref
    v_ref = g * g / np.float32(2)
    ulps = float((np.abs(v[s.net].astype(np.float64) - v_ref) / np.maximum(np.spacing(v_ref), F32_TINY)).max())
    print("%s: loss %.6e rel err %.2e; gradient blocks %s; v off by %.2f ulp at most" %
          (case, loss, e_loss, " ".join("%s %.2e" % kv for kv in errs.items()), ulps))
    np.testing.assert_array_equal(theta, s.theta)                               # eta = 0, and the other nets
    assert opt.beta_t == [0.25, 0.25]
    others = _others(s)
    assert np.array_equal(m[others], np.full(others.sum(), SENTINEL, np.float32)) and np.array_equal(v[others], m[others])
    assert np.isfinite(g).all() and ulps <= 1.0
    assert e_loss < TOL_LOSS
    assert PC.worst(errs, "W") < TOL_W, errs
    assert PC.worst(errs, "b") < TOL_B, errs


# ---- C: sequence semantics -----------------------------------------------------------------------------------------------------------------
def _run(eng, s, dev, order, theta=None, m=None, v=None, opt=None, update=True):
    """One call on the device samples `dev`; the state as numpy afterwards."""
    X, B, Y = dev
    theta = _t(s.theta) if theta is None else _t(theta)
    m = _t(_moments(s)) if m is None else _t(m)
    v = _t(_moments(s)) if v is None else _t(v)
    opt = opt or ADAM(1e-3)
    od = None if order is None else _t(order, np.int32)
    loss = eng.pretrain_flux(s.k, theta, m, v, X, B, Y, od, s.gs, opt, update=update)
    return _np(theta), _np(m), _np(v), opt, loss


def _check_pass(s, got, ref, what):
    theta, m, v, opt, loss = got
    th_ref, m_ref, v_ref, bt_ref, losses_ref = ref
    cfg, net = s.cfg, s.net
    e_th, e_m, e_v = (PC.block_errors(cfg, a[net], r) for a, r in ((theta, th_ref), (m, m_ref), (v, v_ref)))
    moved = th_ref - s.theta[net]
    e_mv = {nm: float(np.linalg.norm((theta[net] - th_ref)[sl]) / np.linalg.norm(moved[sl])) for nm, sl in PC.blocks(cfg)}
    e_loss = abs(loss - np.mean(losses_ref)) / np.mean(losses_ref)
    print("%s: loss rel err %.2e; theta %.2e, per distance moved %.2e, m %.2e, v %.2e (largest over the layer blocks)" %
          (what, e_loss, max(e_th.values()), max(e_mv.values()), max(e_m.values()), max(e_v.values())))
    others = _others(s)
    np.testing.assert_array_equal(theta[others], s.theta[others])
    assert np.array_equal(m[others], np.full(others.sum(), SENTINEL, np.float32)) and np.array_equal(v[others], m[others])
    assert min(np.linalg.norm(moved[sl]) / np.linalg.norm(th_ref[sl]) for _, sl in PC.blocks(cfg)) > 1e-3      # every block moved
    np.testing.assert_allclose(opt.beta_t, bt_ref, rtol=1e-15)
    assert e_loss < TOL_LOSS                       # the mean of each sample's loss just before its own update
    assert max(e_m.values()) < TOL_M, e_m
    assert max(e_v.values()) < TOL_V, e_v
    assert max(e_th.values()) < TOL_THETA, e_th
    assert max(e_mv.values()) < TOL_MOVED, e_mv


def test_pass_with_repeated_order_follows_the_sequential_loop():
    """An order with repeats ([3, 3, 0, 1, 1, 5, 7, 2]): every visit sees the weights the visits before it left.  m and v are not scale-invariant,
    so they pin the gradients along the trajectory, not only their signs."""
    s, ref_rep, _ = PC.sequence_reference()
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        got = _run(eng, s, _dev_sample(s), PC.SEQ_ORDER)
    _check_pass(s, got, ref_rep, "repeated order")


def test_order_none_is_the_identity_order():
    s, _, ref_id = PC.sequence_reference()
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        dev = _dev_sample(s)
        a = _run(eng, s, dev, None)
        b = _run(eng, s, dev, np.arange(PC.SEQ_N))
    _check_pass(s, a, ref_id, "order = None")
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3].beta_t == b[3].beta_t and a[4] == b[4]


def test_split_pass_gives_the_bits_of_one_pass():
    """Two calls over the halves of the order, carrying m, v and the running powers (doubles): the same serial chain, so the same bits."""
    s, _, _ = PC.sequence_reference()
    order = np.asarray(PC.SEQ_ORDER)
    h = len(order) // 2
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        dev = _dev_sample(s)
        one = _run(eng, s, dev, order)
        # `order` must have one entry per sample handed over: each half gets its own sample arrays, holding its visits BACKWARDS, and an order that
        # walks them from the last to the first — the visits of the one call, in its sequence, through the order indexing
        import torch
        halves = []
        for part in (order[:h], order[h:]):
            idx = _t(part[::-1], np.int64)
            halves.append(tuple(torch.index_select(a, 0, idx).contiguous() for a in dev))
        back = lambda n: np.arange(n)[::-1]
        th, m, v, opt, l1 = _run(eng, s, halves[0], back(h))
        bt_mid = list(opt.beta_t)
        th, m, v, opt, l2 = _run(eng, s, halves[1], back(len(order) - h), theta=th, m=m, v=v, opt=opt)
    assert bt_mid[0] < 0.9 and bt_mid[1] < 0.999 and opt.beta_t[0] < bt_mid[0]
    for x, y in zip((th, m, v), one[:3]):
        np.testing.assert_array_equal(x, y)
    assert opt.beta_t == one[3].beta_t
    np.testing.assert_allclose((l1 * h + l2 * (len(order) - h)) / len(order), one[4], rtol=1e-6)     # (float32 means of float32 sums)


def test_update_false_evaluates_and_leaves_everything():
    """update=False: theta keeps its bits, the moments may be None, the running powers stay, the value is the mean loss at the given weights."""
    s, _, _ = PC.sequence_reference()
    ref = np.mean([PC.oracle_loss_grad(s, s.theta[s.net], i)[0] for i in range(PC.SEQ_N)])
    theta = _t(s.theta)
    opt = ADAM(1e-3)
    opt.beta_t = [0.81, 0.998001]
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        X, B, Y = _dev_sample(s)
        loss = eng.pretrain_flux(s.k, theta, None, None, X, B, Y, None, s.gs, opt, update=False)
        m, v = _t(_moments(s)), _t(_moments(s))
        loss_mv = eng.pretrain_flux(s.k, theta, m, v, X, B, Y, _t(PC.SEQ_ORDER, np.int32), s.gs, opt, update=False)
    ref_rep = np.mean([PC.oracle_loss_grad(s, s.theta[s.net], i)[0] for i in PC.SEQ_ORDER])
    print("update=False: loss %.6e rel err %.2e, over the repeated order %.2e" % (loss, abs(loss - ref) / ref, abs(loss_mv - ref_rep) / ref_rep))
    np.testing.assert_array_equal(_np(theta), s.theta)
    assert opt.beta_t == [0.81, 0.998001]
    np.testing.assert_array_equal(_np(m), _moments(s))           # given, but neither read nor written
    np.testing.assert_array_equal(_np(v), _moments(s))
    assert abs(loss - ref) / ref < TOL_LOSS and abs(loss_mv - ref_rep) / ref_rep < TOL_LOSS


def test_one_sample_pass_is_one_adam_step():
    """n_samples = 1 with the real ADAM(1e-3): the first step from zero moments."""
    s = PC.sample(PC.SEQ_CASE, PC.SEQ_N)
    one = PC.sample(PC.SEQ_CASE)
    assert np.array_equal(one.X[0], s.X[0]) and np.array_equal(one.theta, s.theta)
    ref = PC.sequential_pass(one, [0])
    with colnde.ColumnNDE(one.cfg, 1) as eng:
        got = _run(eng, one, _dev_sample(one), None)
    assert got[3].beta_t == [0.9 * float(np.float32(0.9)), 0.999 * float(np.float32(0.999))]
    _check_pass(one, got, ref, "one sample")


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(eng, s, theta_np, match, k=None, m="zeros", v="zeros", opt=None, exc=colnde._lib.ColndeError):
    theta = _t(theta_np)
    n = theta.numel()
    mm = _t(np.zeros(n, np.float32)) if isinstance(m, str) else m
    vv = _t(np.zeros(n, np.float32)) if isinstance(v, str) else v
    X, B, Y = _dev_sample(s)
    with pytest.raises(exc, match=match):
        eng.pretrain_flux(s.k if k is None else k, theta, mm, vv, X, B, Y, None, s.gs, opt or ADAM(1e-3))
    np.testing.assert_array_equal(_np(theta), theta_np)
    if mm is not None:
        assert not _np(mm).any() and not _np(vv).any()


@pytest.mark.parametrize("option", ["smooth_NN", "smooth_Ri", "inplace_variant"])
def test_refuses_the_options_it_does_not_cover(option):
    s = PC.sample(PC.SEQ_CASE)
    with colnde.ColumnNDE(s.cfg.with_(**{option: True}), 1) as eng:
        _refused(eng, s, s.theta, "smoothing options" if option.startswith("smooth") else "inplace_variant")


@pytest.mark.parametrize("case,k", [("fc-gs1e-2", 0), ("fc-gs1e-2", 1), ("fc_convadj-gs1e-2", 0), ("fc-gs1e-2", 3), (PC.SEQ_CASE, 3), (PC.SEQ_CASE, -1)])
def test_refuses_a_flux_type_the_model_does_not_have(case, k):
    s = PC.sample(case)
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        _refused(eng, s, s.theta, "flux_type", k=k)


def test_refuses_an_update_without_moments_and_finished_running_powers():
    s = PC.sample(PC.SEQ_CASE)
    with colnde.ColumnNDE(s.cfg, 1) as eng:
        _refused(eng, s, s.theta, "moments", m=None, v=None, exc=ValueError)                 # the wrapper ...
        theta, (X, B, Y) = _t(s.theta), _dev_sample(s)
        bt, loss = (ctypes.c_double * 2)(0.9, 0.999), ctypes.c_float(0)
        args = lambda n, mv: (eng._h, s.k, theta.data_ptr(), mv, mv, X.data_ptr(), B.data_ptr(), Y.data_ptr(), None, n, s.gs, 1e-3, 0.9, 0.999, 1e-8, bt,
                              1, ctypes.byref(loss))
        L = colnde._lib.lib()
        assert L.colnde_pretrain_flux_dev(*args(1, None)) != 0                                # ... and the library itself
        assert "moments" in L.colnde_last_error().decode()
        m = _t(np.zeros(s.cfg.n_params, np.float32))
        for n in (0, -3):                                                                     # n_samples < 1: only the C call can ask for it
            assert L.colnde_pretrain_flux_dev(*args(n, m.data_ptr())) != 0
            assert "n_samples" in L.colnde_last_error().decode()
        assert list(bt) == [0.9, 0.999] and not _np(m).any()
        np.testing.assert_array_equal(_np(theta), s.theta)
        for beta_t in ([1.0, 0.5], [0.5, 1.0], [float("nan"), 0.5]):
            opt = ADAM(1e-3)
            opt.beta_t = list(beta_t)
            _refused(eng, s, s.theta, "beta", opt=opt)


def test_refuses_ensemble_and_closure_handles():
    from colnde.nde import ColumnNDEEnsemble, ClosureColumns
    s = PC.sample(PC.SEQ_CASE)
    with ColumnNDEEnsemble(s.cfg, 1, 2) as ens:
        _refused(ens, s, s.theta, "ensemble")
    with ClosureColumns(s.cfg, 1, 1) as clo:
        _refused(clo, s, np.linspace(0.1, 0.5, clo.n_params).astype(np.float32), "closure handle")


def test_refuses_a_network_beyond_the_lds_and_states_the_bytes():
    """The one workgroup keeps three activation-sized arrays in LDS: seven hidden layers of 1,928 need 164,096 B, more than the 160 KB the call
    accepts.  (fc_Nz64_7x800_lds68k is the other side: 69,344 B, above what a kernel may take without its limit raised, runs and matches.)"""
    import torch
    cfg = PC.sample("fc_Nz64").cfg.with_(layer_sizes=(64,) + (1928,) * 7 + (63,), activations=("mish",) * 7 + ("identity",))
    need = 4 * (64 + 3 * (sum((n + 3) & ~3 for n in cfg.layer_sizes[1:]) + 4) + 3 * (cfg.Nz + 4) + 64)
    assert need == 164096 and need > 160 * 1024
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    theta, m, v = z(cfg.n_params), z(cfg.n_params), z(cfg.n_params)
    with colnde.ColumnNDE(cfg, 1) as eng:
        with pytest.raises(colnde._lib.ColndeError, match="%d B of LDS" % need):
            eng.pretrain_flux(2, theta, m, v, z(1, 64), z(1, 2), z(1, 65), None, 1e-2, ADAM(1e-3))
    assert not theta.any() and not m.any() and not v.any()
