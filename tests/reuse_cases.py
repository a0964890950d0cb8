"""The handles, problems, fresh-handle references and float64 references of tests/test_gpu_handle_reuse.py.  A helper, not a test.

A KIND is one way to create a handle, at the smallest shape at which each of its plans still has a ragged edge (17 columns: two 16-column tiles, the
second with one column; 33: two 32-column tiles).  Per kind there are two problems: P1, and P2 = P1's columns in reverse order with a truth solved from
other weights (twice the truth weights: a larger loss than P1's, so that float32 cancellation in it stays where the parity tests have it).

`fresh(kind, ...)` is what a handle created directly in a configuration returns from its first forward, loss and loss_grad; it is computed once per
configuration and process (the kernels reduce in a fixed order: test_tile16_taped_weight_gradients and its neighbours hold that) and left unchanged.
`hold(kind, ...)` applies the float64 bounds of tests/test_gpu_parity.py where the parity tests hold the configuration to float64: SOL_ATOL,
LOSS_RTOL, GRAD_REL for the wind-mixing handles (whole vector, and 4 x GRAD_REL per layer block as tests/test_gpu_wide_nets.py), FC_* for the plain fc32
handle as test_free_convection applies them, the ensemble's rows as tests/test_gpu_ensemble.py holds them.

What limits the per-block bound on these short problems (measured on an MI355X, profiles/handle_reuse_errors.json: block_rel): over three ten-minute frames
the temperature misfit sol_T - truth_T is about 1e-3 of T, so the float32 solve's own error (sol_abs 5e-7) is 1e-4 ... 6e-4 of the wT net's cotangent, in every
layer of that net and under both arithmetics alike, and it grows with the number of steps (more round-off in the solve: 9e-4 ... 2e-3 at 4 and 6 sub-steps,
where the uw and vw nets stay at 1e-5).  At the sub-step counts of KINDS the worst block is 6.1e-4 against the bound 8e-4; sequence f therefore ends at the
kind's own count (the handle is created with another one) instead of asking the bound of a step count no parity test holds."""
import functools
from types import SimpleNamespace

import numpy as np

import colnde
from colnde import synthetic
from colnde.free_convection import conv_to_dense
from colnde.nde import ENGINE_REGTILE, ENGINE_TILE16
from oracle import nde_oracle as O
from tests import conv_cases
from tests.test_gpu_closure import SETS
from tests.test_gpu_closure import _problem as closure_problem
from tests.test_gpu_ensemble import PHYS, _model_cfg
from tests.test_gpu_parity import FC_GRAD_REL, FC_LOSS_RTOL, FC_SOL_ATOL, GRAD_REL, LOSS_RTOL, SOL_ATOL, _record, _rel

BF, F32 = "bf16x3_exact", "f32_mfma"
OTHER = {BF: F32, F32: BF}
SC_WM = (1.0, 0.8, 1.2, 5e-3, 4e-3, 6e-3)
SC_FC = (0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
PH1, PH2 = PHYS[:3], PHYS[2:5]
# constants under which one RK4 step per save interval is stable (the default constants need two): the ensemble of sequence g.3 starts from these
PH_LOW = np.array([[1e-4, 0.04, 1.0, 0.25, 1.0], [5e-4, 0.03, 0.8, 0.2, 1.2], [1e-3, 0.02, 1.3, 0.3, 1.0]], np.float32)
PHYSICS = {"PH1": PH1, "PH2": PH2, "LOW": PH_LOW}

_WIDE1 = dict(layer_sizes=(96, 400, 31), activations=("mish", "identity"))
_WIDE2 = dict(layer_sizes=(96, 400, 400, 31), activations=("swish", "swish", "identity"))


def _wm(n, **kw):
    return lambda: synthetic.wind_mixing_problem(n, n_frames=4, weight_divisor=1e2, **kw)


def _ca64():
    # tests/test_gpu_lifecycle._cases' ConvectiveAdjustmentNDE case (4 RKC2 steps per save interval of 1/128) at 16 columns
    p = synthetic.free_convection_problem(16, Nz=64, n_save=5, t_end=4.0 / 128.0, convective_adjustment=True)
    p.cfg = p.cfg.with_(stepper="rkc2", substeps=4)
    return p


# family: single (one weight vector: colnde.ColumnNDE) | wm_ens | fc_ens | closure (K rows).  conv: the filter length of a colnde_create_conv handle.
# model: wm | fc.  oracle: the bounds `hold` applies (None: the parity tests hold this configuration by other means; here it is held to the fresh handle).
KINDS = {
    "netsplit": dict(make=_wm(17), kw={}, family="single", model="wm", oracle="wm"),
    "regtile": dict(make=_wm(33), kw=dict(engine=ENGINE_REGTILE), family="single", model="wm", oracle="wm"),
    "tile16": dict(make=_wm(17), kw=dict(engine=ENGINE_TILE16), family="single", model="wm", oracle="wm"),
    "tile16_l2": dict(make=_wm(17), kw=dict(engine=ENGINE_TILE16), env={"COLNDE_T16_DWLDS": "0"}, family="single", model="wm", oracle="wm"),
    "wide1_16": dict(make=_wm(16, substeps=3, **_WIDE1), kw={}, family="single", model="wm", oracle="wm"),        # one tile: 36 dW records
    "wide1_17": dict(make=_wm(17, substeps=3, **_WIDE1), kw={}, family="single", model="wm", oracle="wm"),        # two tiles: 72
    "wide2_16": dict(make=_wm(16, substeps=3, **_WIDE2), kw={}, family="single", model="wm", oracle="wm"),
    "wide2_17": dict(make=_wm(17, substeps=3, **_WIDE2), kw={}, family="single", model="wm", oracle="wm"),
    "fc32": dict(make=lambda: synthetic.free_convection_problem(33, Nz=32, n_save=5, substeps=2, t_end=0.01), kw={}, family="single", model="fc", oracle="fc"),
    "fc32_conv2": dict(make=lambda: synthetic.free_convection_conv_problem(33, 2, Nz=32, n_save=5, substeps=2, weight_divisor=10.0, t_end=1.0),
                       kw=dict(conv=2), conv=2, family="single", model="fc", oracle=None),
    "ca64_rkc2": dict(make=_ca64, kw={}, family="single", model="fc", oracle=None),
    "wm_ens": dict(make=_wm(17), kw={}, family="wm_ens", model="wm", oracle="wm_rows", K=3),
    "fc_ens": dict(make=lambda: synthetic.free_convection_problem(20, Nz=32, n_save=5, substeps=2, t_end=0.01), kw={}, family="fc_ens", model="fc",
                   oracle=None, K=2),
    "closure": dict(make=None, kw={}, family="closure", model="wm", oracle=None, K=3),
}
SINGLE = [k for k, v in KINDS.items() if v["family"] == "single"]
PLAIN_SINGLE = [k for k in SINGLE if not KINDS[k].get("conv")]            # the entry points a conv handle refuses (rhs, flux, error_estimate, choose_substeps, ...)
WM_SINGLE = [k for k in SINGLE if KINDS[k]["model"] == "wm"]
WIDE = [k for k in SINGLE if k.startswith("wide")]
ROWS = [k for k, v in KINDS.items() if v["family"] != "single"]
ALL = list(KINDS)


def scalings(kind):
    return SC_WM if KINDS[kind]["model"] == "wm" else SC_FC


def _solve64(kind, cfg, x0, bcs, w):
    c = KINDS[kind].get("conv")
    if c:
        return O.solve(conv_cases.dense_cfg(cfg, c), x0, bcs, conv_to_dense(np.asarray(w, np.float64), cfg.Nz, c))
    return O.solve(cfg, x0, bcs, w)


@functools.lru_cache(maxsize=None)
def problem(kind, which=1):
    """SimpleNamespace(cfg, n, x0, bcs, truth, w, w_truth): problem `which` (1 | 2) of a kind; w is what the handle's calls take ([K, P] for the K-row kinds)."""
    k = KINDS[kind]
    if k["family"] == "closure":
        p, _, truth = closure_problem(3)
        w, w_truth = SETS.astype(np.float32), None
    else:
        p = k["make"]()
        w_truth = p.weights_truth
        truth = None
        if k["family"] == "single":
            w = p.weights.astype(np.float32)
        else:
            w = np.stack([synthetic.make_weights(synthetic._rng(11, m), p.cfg, 1e2) for m in range(k["K"])]).astype(np.float32)
    x0, bcs = p.x0, p.bcs
    if which == 2:
        x0, bcs = np.ascontiguousarray(x0[::-1]), np.ascontiguousarray(bcs[::-1])
        truth = None
    if truth is None:
        if k["family"] == "closure":
            from tests import closure_common as C
            truth = O.solve(C.with_params(p.cfg, (3e-4, 0.05, 0.9, 0.3, 1.2)), x0, bcs, np.zeros(p.cfg.n_params)).astype(np.float32)
        else:
            truth = _solve64(kind, p.cfg, x0, bcs, w_truth if which == 1 else 2.0 * np.asarray(w_truth, np.float64)).astype(np.float32)
    for a in (x0, bcs, truth, w):
        a.setflags(write=False)
    return SimpleNamespace(cfg=p.cfg, n=x0.shape[0], x0=x0, bcs=bcs, truth=truth, w=w)


def open_handle(kind, ma=BF, substeps=None, physics="PH1"):
    """A handle of the kind, no problem set.  substeps: in the configuration's place; physics: the wind-mixing ensemble's constants (a key of PHYSICS)."""
    k, p = KINDS[kind], problem(kind)
    cfg = p.cfg if substeps is None else p.cfg.with_(substeps=substeps)
    if k["family"] == "wm_ens":
        return colnde.ColumnNDEEnsemble(cfg, p.n, k["K"], physics=PHYSICS[physics], matrix_arithmetic=ma)
    if k["family"] == "fc_ens":
        return colnde.FreeConvectionEnsemble(cfg, p.n, k["K"], matrix_arithmetic=ma)
    if k["family"] == "closure":
        return colnde.ClosureColumns(cfg, p.n, k["K"])
    return colnde.ColumnNDE(cfg, p.n, matrix_arithmetic=ma, **k["kw"])


def set_problem(h, p, device=False, truth=True):
    if device:
        import torch
        x0, bcs, tr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p.x0, p.bcs, p.truth))
        h.set_problem(x0, bcs, tr if truth else None)
        torch.cuda.synchronize()
    else:
        h.set_problem(p.x0, p.bcs, p.truth if truth else None)


def grad_row(h, kind, w):
    """loss_grad as one float32 row [grad; terms(6); total] (K rows: the library's [K, P + 8])"""
    r = h.loss_grad(w, scalings(kind))
    if KINDS[kind]["family"] != "single":
        return np.asarray(r)
    total, terms, g = r
    return np.concatenate([g, terms, np.float32([total])]).astype(np.float32)


def loss_row(h, kind, w):
    r = h.loss(w, scalings(kind))
    if KINDS[kind]["family"] != "single":
        return np.asarray(r)
    return np.concatenate([r[1], np.float32([r[0]])]).astype(np.float32)


def run(h, kind, w):
    """(sol, loss row, loss_grad row) of the handle as it stands"""
    return np.asarray(h.forward(w)), loss_row(h, kind, w), grad_row(h, kind, w)


def same(got, want, what=""):
    """bit equality of two `run` results (or any two tuples of arrays)"""
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, i, float(np.abs(a.astype(np.float64) - b).max()))


@functools.lru_cache(maxsize=None)
def fresh(kind, which=1, ma=BF, substeps=None, gcols=None, physics="PH1", schedule=None):
    """SimpleNamespace(res = run(...), plan) of a handle created in exactly this configuration that makes only these calls.  Call it with the kind's
    environment in force (the test module's fixture sets it)."""
    p = problem(kind, which)
    with open_handle(kind, ma, substeps, physics) as h:
        if schedule is not None:
            h.set_schedule(schedule)
        if gcols is not None:
            h.set_global_columns(gcols)
        set_problem(h, p)
        res = run(h, kind, p.w)
        plan = h.plan() if KINDS[kind]["family"] != "closure" else None
    for a in res:
        a.setflags(write=False)
    return SimpleNamespace(res=res, plan=plan)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(kind, which=1, substeps=None, physics="PH1"):
    """[(total, terms, grad, sol)] per model (one entry for a single handle), float64"""
    k, p = KINDS[kind], problem(kind, which)
    cfg = p.cfg if substeps is None else p.cfg.with_(substeps=substeps)
    sc = np.array(scalings(kind), np.float64)
    if k["family"] == "wm_ens":
        return [O.loss_and_grad(_model_cfg(cfg, PHYSICS[physics][m]), p.x0, p.bcs, p.w[m], p.truth, sc) for m in range(k["K"])]
    return [O.loss_and_grad(cfg, p.x0, p.bcs, p.w, p.truth, sc)]


def _layer_blocks(cfg):
    sizes, off = cfg.layer_sizes, 0
    for net in range(cfg.n_nets):
        for a, b in zip(sizes[:-1], sizes[1:]):
            for n in (a * b, b):
                yield net, a, b, off, off + n
                off += n
    assert off == cfg.n_params


def hold(kind, res, which=1, substeps=None, physics="PH1", tag=""):
    """The float64 bounds on a `run` result whose configuration the parity tests hold to float64 (module docstring); records the distances."""
    how = KINDS[kind]["oracle"]
    if how is None:
        return
    sol, lrow, grow = res
    refs = oracle(kind, which, substeps, physics)
    sol_atol, loss_rtol, grad_rel = (FC_SOL_ATOL, FC_LOSS_RTOL, FC_GRAD_REL) if how == "fc" else (SOL_ATOL, LOSS_RTOL, GRAD_REL)
    cfg = problem(kind).cfg
    P = cfg.n_params
    for m, (tot, terms, g, sol64) in enumerate(refs):
        s, l, r = (sol, lrow, grow) if how != "wm_rows" else (sol[m], lrow[m], grow[m])
        errs = dict(sol_abs=np.abs(s - sol64).max(), loss_rel=abs(r[P + 6] - tot) / abs(tot), loss_only_rel=abs(l[6] - tot) / abs(tot), grad_rel=_rel(r[:P], g))
        blocks = [(net, a, b, lo, hi) for net, a, b, lo, hi in _layer_blocks(cfg)] if how != "fc" else []
        live = [blk for blk in blocks if np.linalg.norm(g[blk[3]:blk[4]]) > 0]
        if live:                                           # the worst layer block of every net (tests/test_gpu_wide_nets.py)
            errs["block_rel"] = max(_rel(r[lo:hi], g[lo:hi]) for _, _, _, lo, hi in live)
        _record("handle_reuse/%s/%s%s" % (kind, tag or "final", "/model%d" % m if how == "wm_rows" else ""), **errs)
        assert errs["sol_abs"] < sol_atol, (kind, tag, m, errs)
        assert np.isclose(r[P + 6], tot, rtol=loss_rtol) and np.isclose(l[6], tot, rtol=loss_rtol), (kind, tag, m, errs)
        assert errs["grad_rel"] < grad_rel, (kind, tag, m, errs)
        if how != "fc":
            np.testing.assert_allclose(r[P:P + 6], terms, rtol=10 * loss_rtol, atol=0)
        for net, a, b, lo, hi in blocks:
            if np.linalg.norm(g[lo:hi]) > 0:
                assert _rel(r[lo:hi], g[lo:hi]) < 4 * grad_rel, (kind, tag, m, net, a, b, hi - lo, errs)
            else:                                          # a block the configuration pins (zero_weights): exactly zero on the GPU too
                assert not r[lo:hi].any(), (kind, tag, m, net, a, b, hi - lo)


# ---- the embedding calls a handle serves (sequence c) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wm_embed_state():
    from tests import wm_embed_common as W
    s = W.embed_inputs(synthetic.wind_mixing_problem(200, n_frames=3, weight_divisor=1.0))
    for a in s:
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def fc_embed_state(Nz):
    from tests import fc_embed_restatement as R
    s = R.switch_robust_case(Nz, 200)
    for a in s:
        a.setflags(write=False)
    return s


def embed_call(kind, n):
    """(method, args, kwargs, arrays) of the embedding call a handle of the kind serves on the first n of 200 columns, or None (the closure handle
    serves none): `arrays` names the array arguments — positions in args, keys in kwargs, ("halos", i) for the members of that pair — so that a caller
    can put device tensors in their place (tests/stream_cases.py).
    Single wind-mixing handles: wm_embedded as K = 1 (forcing, step and faces; the wide networks through the generic kernel).  The wind-mixing
    ensemble: wm_embedded for its K models, each with its own state, halo and constants.  Plain fc32 handles: fc_embedded_step with the face
    diagnosis; the conv handle (K = 1) and the free-convection ensemble: fc_embedded.  What a K-model handle keeps from one call to the next — the
    per-model constants, the packed images — differs between the 200-column and the 1-column call (other constants, other weights)."""
    k, p = KINDS[kind], problem(kind)
    c = lambda a: np.ascontiguousarray(a[:n])
    if k["family"] == "closure":
        return None
    if k["model"] == "wm":
        from tests import wm_embed_common as W
        u, v, T, top = wm_embed_state()
        K = k.get("K", 1)
        shift = np.arange(K, dtype=np.float32)[:, None, None] * np.float32(0.01)
        uK, vK, TK = (np.ascontiguousarray(c(a)[None] + shift) for a in (u, v, T))
        halo = np.ascontiguousarray(np.stack([uK[:, :, 0] - 1e-3, vK[:, :, 0] + 2e-3, TK[:, :, 0] + 0.01], axis=1).astype(np.float32))
        if k["family"] == "single":
            w, params = p.w[None], [W.mpp_params()]
        else:
            w = p.w
            params = [tuple(float(x) for x in row) + W.mpp_params()[5:] for row in (PH2 if n == 200 else PH1)]
        return ("wm_embedded", [w, uK, vK, TK, np.ascontiguousarray(top[:, :n]), W.LZ], dict(dt=60.0, params=params, halo_bottom=halo),
                [0, 1, 2, 3, 4, "halo_bottom"])
    T, top, hb, ht = fc_embed_state(p.cfg.Nz)
    if k["family"] == "single" and not k.get("conv"):
        return "fc_embedded_step", [p.w, c(T), c(top), 1000.0, 600.0, 10.0], dict(halos=(c(hb), c(ht)), diagnose=True), [0, 1, 2, ("halos", 0), ("halos", 1)]
    K = k.get("K", 1)
    if k.get("conv"):                                  # K = 1
        w = np.ascontiguousarray((p.w if n == 200 else np.float32(0.5) * p.w)[None])
    else:
        w = np.ascontiguousarray(p.w if n == 200 else p.w[::-1])
    shift = np.arange(K, dtype=np.float32)[:, None, None] * np.float32(0.01)
    TK = np.ascontiguousarray(c(T)[None] + shift)
    hbK, htK = (np.ascontiguousarray(np.repeat(c(a)[None], K, axis=0)) for a in (hb, ht))
    return "fc_embedded", [w, TK, c(top), 1000.0, 10.0], dict(dt=600.0, halos=(hbK, htK)), [0, 1, 2, ("halos", 0), ("halos", 1)]


def flat(r):
    """what an embedding call returns (a tuple of arrays, or a named tuple of such groups, None for a group not asked for) as one flat tuple"""
    out = []
    for part in r:
        out.extend(part if isinstance(part, (tuple, list)) else [part])
    return tuple(a for a in out if a is not None)


def embed(h, kind, n):
    """The call of `embed_call` on the handle with host arrays, as a flat tuple of arrays, or None (the closure handle)."""
    call = embed_call(kind, n)
    if call is None:
        return None
    name, args, kwargs, _ = call
    return flat(getattr(h, name)(*args, **kwargs))


# ---- refusals by design ------------------------------------------------------------------------------------------------------------------------------
def refusal(kind):
    """the words with which the single-model entry points refuse a handle of this kind (api_internal.h: SINGLE_MODEL_ONLY, PLAIN_NETWORK_ONLY)"""
    k = KINDS[kind]
    if k["family"] == "closure":
        return "this is a closure handle"
    if k["family"] != "single":
        return r"this handle holds an ensemble of \d+ models: use colnde_ensemble_"
    assert k.get("conv")
    return r"does not cover the convolutional first layer of a colnde_create_conv handle \(conv=%d\)" % k["conv"]


def raw_refused(h, name, match):
    """The entry point `name`, called with null pointers and zeros behind the handle, is refused with `match`: the refusals by the kind of the handle
    come before anything else is looked at."""
    import ctypes
    import pytest
    from colnde import _lib
    fn = getattr(h._L, name)
    args = [h._h] + [0 if t in (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double) else None for t in fn.argtypes[1:]]
    with pytest.raises(_lib.ColndeError, match=match):
        _lib.check(fn(*args))
