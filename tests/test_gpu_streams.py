"""Every device entry point on a non-default stream computes the bits of a fresh handle on the null stream.

include/colnde.h: a `_dev` call is "enqueued on the handle's stream and NOT synchronised"; colnde_set_stream is part of the ABI; every Python method
takes torch's current stream before it launches; a Julia caller never runs on the null stream at all.  The rest of the suite runs with torch's current
stream as the null stream, which orders itself against everything and so hides a launch, fill or upload issued off the handle's stream.  Here the calls
run on non-blocking side streams behind LATE INPUTS (tests/stream_cases.py): the tensors a call reads hold stale but valid data until a delay on the
side stream has passed, so work issued anywhere else reads something other than what the caller put there.  Results are held to
reuse_cases.fresh (np.array_equal) and, where the parity tests hold the configuration to float64, to their bounds (reuse_cases.hold).

What the sequences found is in DESIGN §4e-bis.  Calls held to "returned while the delay was still running" on a warmed handle: set_problem_dev,
forward_dev, loss_dev, loss_grad_dev, adam_step_dev and the ensembles' and the closure handle's twins, rhs_dev, flux_dev, loss_per_tstep_dev, the
embedding calls and the column operations."""
import numpy as np
import pytest

from tests import reuse_cases as R
from tests import stream_cases as SC
from tests.reuse_cases import BF, F32, KINDS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _environment_of_the_kind(request, monkeypatch):
    """COLNDE_* switches of the handle kind, before any handle of the test (fresh ones included) is created"""
    kind = getattr(request.node, "callspec", None) and request.node.callspec.params.get("kind")
    for k, v in (KINDS[kind].get("env", {}) if kind else {}).items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def streams():
    """two non-blocking side streams, created (and used) once"""
    return SC.side_streams()


def _warm(kind, which=2):
    """the handle has run problem `which` on the null stream: tapes, plans and images exist"""
    def warm(h):
        p = R.problem(kind, which)
        R.set_problem(h, p)
        R.run(h, kind, p.w)
    return warm


def _make(kind, ma=BF):
    return lambda: R.open_handle(kind, ma)


# ---- the power of the harness: a mis-ordered caller is seen -----------------------------------------------------------------------------------------
def test_power_a_producer_on_a_side_stream_is_not_seen_from_the_null_stream(streams):
    """The producer (delay, late copies) runs on S, the handle stays on the null stream: the library reads the stale (valid, finite) P2 data and the
    result is NOT the fresh handle's.  So torch's side streams are unordered against the null stream on this runtime, and the harness sees a launch
    that is not on the caller's stream."""
    import torch
    S, kind = streams[0], "netsplit"
    late = SC.Late(**SC.problem_pairs(kind))

    def side(h, late, seconds, body):
        with torch.cuda.stream(S):
            ev = late.arrive(seconds)
        got = body(h, late.dev, SC.Still(ev))                              # torch's current stream: the null stream
        return got

    got, ref = SC.late_inputs(S, _make(kind), late, lambda h, t, still: SC.run_dev(h, kind, t, still), warm=_warm(kind), tag="power", side=side)
    want = R.fresh(kind, 1).res
    R.same(SC.rows(kind, ref), want, "null stream")
    got = SC.rows(kind, got)
    assert all(np.isfinite(a).all() for a in got)
    assert not any(np.array_equal(a, b) for a, b in zip(got, want)), "a producer on a side stream was ordered before launches on the null stream"
    # what it read instead: P2's columns under half the weights
    stale = SC.Late(**SC.problem_pairs(kind))
    with R.open_handle(kind) as h:
        R.same(got, SC.rows(kind, SC.to_numpy(SC.run_dev(h, kind, stale.dev, SC.Still()))), "the stale inputs")


# ---- a. a warmed handle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ma", [(k, BF) for k in R.ALL] + [(k, F32) for k in R.WM_SINGLE])
def test_a_warmed_handle(streams, kind, ma):
    late = SC.Late(**SC.problem_pairs(kind))
    got, ref = SC.late_inputs(streams[0], _make(kind, ma), late, lambda h, t, still: SC.run_dev(h, kind, t, still), warm=_warm(kind), tag="a/%s/%s" % (kind, ma))
    want = R.fresh(kind, 1, BF if KINDS[kind]["family"] == "closure" else ma).res
    R.same(SC.rows(kind, ref), want, "null stream, device tensors")
    R.same(SC.rows(kind, got), want, "side stream, late inputs")
    R.hold(kind, SC.rows(kind, got), tag="streams/a/%s" % ma)


# ---- b. a cold handle --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ALL)
def test_b_cold_handle(streams, kind):
    """The handle's very first calls run on the side stream behind the delay: lazy allocations, tape planning, table and macro uploads, the RKC table,
    the activation rows, the conv and ensemble images.  Wide kinds: then rhs and flux on 70 columns — more than the handle has, so the activation-row
    slab of 3 x 96-400-400-31 grows while the stream is in use."""
    p = R.problem(kind)
    pairs = SC.problem_pairs(kind)
    wide = kind in R.WIDE
    if wide:
        reps = -(-70 // p.n)
        x70, b70 = (np.ascontiguousarray(np.concatenate([a] * reps)[:70]) for a in (p.x0, p.bcs))
        pairs.update(x70=(x70, x70[::-1]), b70=(b70, b70[::-1]))
    late = SC.Late(**pairs)

    def body(h, t, still):
        res = SC.run_dev(h, kind, t, still)
        if wide:
            res += (h.rhs(t["x70"], t["w"], t["b70"], 0.0), h.flux(t["x70"], t["w"], t["b70"], 0.0))
        return res

    got, ref = SC.late_inputs(streams[0], _make(kind), late, body, tag="b/%s" % kind, first_only=True)
    want = R.fresh(kind, 1).res
    R.same(SC.rows(kind, ref[:3]), want, "null stream, device tensors")
    R.same(SC.rows(kind, got[:3]), want, "side stream, late inputs, cold handle")
    R.hold(kind, SC.rows(kind, got[:3]), tag="streams/b")
    if wide:
        assert all(np.isfinite(a).all() for a in got[3:])
        R.same(got[3:], (ref[3], ref[4]), "rhs and flux at 70 columns")
        with R.open_handle(kind) as f:                                     # ... which are a fresh handle's from host arrays
            R.same(got[3:], (f.rhs(x70, p.w, b70, 0.0), f.flux(x70, p.w, b70, 0.0)), "rhs and flux at 70 columns against a fresh handle")


# ---- c. diagnostics and column operations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PLAIN_SINGLE)
def test_c_diagnostics(streams, kind):
    p = R.problem(kind)
    late = SC.Late(**SC.problem_pairs(kind))

    def body(h, t, still):
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
        dx = h.rhs(t["x0"], t["w"], t["bcs"], 0.0)
        still("rhs_dev")
        fl = h.flux(t["x0"], t["w"], t["bcs"], 0.0)
        still("flux_dev")
        lpt = h.loss_per_tstep(t["w"])
        still("loss_per_tstep_dev")
        return dx, fl, lpt

    def warm(h):
        _warm(kind)(h)
        body(h, late.dev, SC.Still())

    got, ref = SC.late_inputs(streams[0], _make(kind), late, body, warm=warm, tag="c/diagnostics/%s" % kind)
    R.same(got, ref, "side stream against null stream")
    with R.open_handle(kind) as f:                                         # the host twins of a fresh handle: what test_gpu_parity holds to float64
        R.set_problem(f, p)
        R.same(got, (f.rhs(p.x0, p.w, p.bcs, 0.0), f.flux(p.x0, p.w, p.bcs, 0.0), f.loss_per_tstep(p.w)), "side stream against the host twins")


@pytest.mark.parametrize("kind", [k for k in R.ALL if KINDS[k]["family"] != "closure"])
def test_c_embedding(streams, kind):
    """wm_embedded (single wind-mixing handles as K = 1, the ensemble), fc_embedded_step with the face diagnosis (plain fc32), fc_embedded (conv,
    free-convection ensemble) at 200 columns with every array argument late; the handle has made the same call once on the stale data."""
    name, pairs, call = SC.embed_pairs(kind)
    late = SC.Late(**pairs)

    def body(h, t, still):
        r = call(h, t)
        still(name)
        return r

    got, ref = SC.late_inputs(streams[0], _make(kind), late, body, warm=lambda h: body(h, late.dev, SC.Still()), tag="c/embedding/%s" % kind)
    assert all(np.isfinite(a).all() for a in got)
    R.same(got, ref, "side stream against null stream")
    with R.open_handle(kind) as f:
        R.same(got, R.embed(f, kind, 200), "side stream against the host twin of a fresh handle")


@pytest.mark.parametrize("kind", ["netsplit", "fc32"])
def test_c_column_operations(streams, kind):
    from tests import wm_embed_common as W
    u, v, T, _ = R.wm_embed_state()
    Nz = R.problem(kind).cfg.Nz
    assert T.shape[1] == Nz
    hb, ht = np.ascontiguousarray(T[:, 0] + np.float32(0.01)), np.ascontiguousarray(T[:, -1] - np.float32(0.01))
    halo3 = np.ascontiguousarray(np.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] + 0.01]).astype(np.float32))
    late = SC.Late(**{k: (a, SC.half(a)) for k, a in dict(u=u, v=v, T=T, hb=hb, ht=ht, halo3=halo3).items()})
    dz = W.LZ / Nz

    def body(h, t, still):
        ca = h.convective_adjustment(t["T"], 600.0, dz, 10.0, halo_bottom=t["hb"], halo_top=t["ht"])
        still("convective_adjustment_dev")
        step = h.implicit_diffusion(t["u"], t["v"], t["T"], 60.0, dz, W.mpp_params(), halo_bottom=t["halo3"])
        still("implicit_diffusion_dev")
        cg = h.coarse_grain(t["T"], 8, "center")
        still("coarse_grain_dev")
        zs, ms = h.zscore(t["T"])
        still("zscore_stats_dev, scale_dev")
        return (ca,) + tuple(step) + (cg, zs, ms)

    got, ref = SC.late_inputs(streams[0], _make(kind), late, body, warm=lambda h: body(h, late.dev, SC.Still()), tag="c/column_operations/%s" % kind)
    assert all(np.isfinite(a).all() for a in got)
    R.same(got, ref, "side stream against null stream")
    with R.open_handle(kind) as f:                                         # the host twins (tests/test_gpu_column_step_paths.py holds them to float64)
        R.same(got[:4], (f.convective_adjustment(T, 600.0, dz, 10.0, halo_bottom=hb, halo_top=ht),)
               + tuple(f.implicit_diffusion(u, v, T, 60.0, dz, W.mpp_params(), halo_bottom=halo3)), "side stream against the host twins")


# ---- d. training steps without a host synchronisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["netsplit", "fc32", "wm_ens", "fc_ens"])
def test_d_training_steps(streams, kind):
    """Three iterations of loss_grad and adam_step (the ensembles' with per-model rates; the free-convection ensemble's with causal_penalty, and
    column_loss at the end) enqueued on the side stream with nothing in between: weights and moments are the null stream's, bit for bit."""
    single = KINDS[kind]["family"] == "single"
    pairs = SC.problem_pairs(kind)
    if not single:
        K = KINDS[kind]["K"]
        pairs["etas"] = (SC.ETAS[:K], SC.half(SC.ETAS[:K]))
        if kind == "fc_ens":
            pairs["coeff"] = (SC.COEFF[:K], SC.half(SC.COEFF[:K]))
    late = SC.Late(**pairs)
    train = SC.train_single if single else SC.train_rows

    def body(h, t, still):
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
        return train(h, kind, t, still)

    got, ref = SC.late_inputs(streams[0], _make(kind), late, body, warm=_warm(kind), tag="d/%s" % kind)
    assert all(np.isfinite(a).all() for a in got)
    R.same(got, ref, "three training steps: side stream against null stream")
    assert not np.array_equal(got[0], R.problem(kind).w)


# ---- e. the stream changed between calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["netsplit", "fc32", "wm_ens", "closure"])
def test_e_problem_on_one_stream_solve_on_another(streams, kind):
    """set_problem (device) on A behind late inputs, forward / loss / loss_grad under stream B: colnde_set_stream drains A before it takes B, so the
    copies the handle made on A have landed.  (The weights are the caller's own tensor, read on B: they are in place before.)"""
    import torch
    A, B = streams
    late = SC.Late(**SC.problem_pairs(kind, weights=False))
    w = torch.from_numpy(R.problem(kind).w.copy()).cuda()

    def body(h, t, still):
        return SC.run_dev(h, kind, dict(t, w=w), still)

    def side(h, late, seconds, body):
        with torch.cuda.stream(A):
            still = SC.Still(late.arrive(seconds))
            h.set_problem(late["x0"], late["bcs"], late["truth"])
            still("set_problem_dev")
        with torch.cuda.stream(B):
            got = SC.run_dev(h, kind, dict(late.dev, w=w), SC.Still(), set_problem=False)
        A.synchronize()
        B.synchronize()
        return got

    got, ref = SC.late_inputs(A, _make(kind), late, body, warm=_warm(kind), tag="e/problem_then_solve/%s" % kind, side=side)
    want = R.fresh(kind, 1).res
    R.same(SC.rows(kind, ref), want, "null stream")
    R.same(SC.rows(kind, got), want, "problem on A, solve on B")
    R.hold(kind, SC.rows(kind, got), tag="streams/e")


@pytest.mark.parametrize("kind", ["netsplit", "fc32", "wm_ens", "closure"])
def test_e_gradient_on_one_stream_update_on_another(streams, kind):
    """loss_grad on A behind late inputs, adam_step under stream B (the closure handle: the library's ADAM on set 0's constants, from set 0's row)."""
    import torch
    A, B = streams
    family = KINDS[kind]["family"]
    pairs = SC.problem_pairs(kind)
    if family == "wm_ens":
        pairs["etas"] = (SC.ETAS[:KINDS[kind]["K"]], SC.half(SC.ETAS[:KINDS[kind]["K"]]))
    late = SC.Late(**pairs)
    sc = R.scalings(kind)

    def grad(h, t, still):
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
        out = h.loss_grad(t["w"], sc)
        still("loss_grad_dev")
        return out

    def update(h, t, out):
        w = t["w"]
        if family == "wm_ens":
            m, v = torch.zeros_like(w), torch.zeros_like(w)
            h.adam_step(w, out, m, v, t["etas"])
        else:
            w, g = (w[0], out[0]) if family == "closure" else (w, out)
            m, v = torch.zeros_like(w), torch.zeros_like(w)
            h.adam_step(w, g, m, v, SC.ETA)
        return t["w"], m, v, out

    def side(h, late, seconds, body):
        with torch.cuda.stream(A):
            out = grad(h, late.dev, SC.Still(late.arrive(seconds)))
        with torch.cuda.stream(B):
            got = update(h, late.dev, out)
        A.synchronize()
        B.synchronize()
        return got

    got, ref = SC.late_inputs(A, _make(kind), late, lambda h, t, still: update(h, t, grad(h, t, still)), warm=_warm(kind),
                              tag="e/gradient_then_update/%s" % kind, side=side)
    R.same(got, ref, "gradient on A, update on B, against the null stream")
    R.same((got[3][:-1] if family == "single" else got[3],), (R.fresh(kind, 1).res[2],), "the gradient")
    assert not np.array_equal(got[0], R.problem(kind).w)


# ---- f. the host-array twins on a side stream -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["netsplit", "fc32"])
def test_f_host_twins_synchronise_the_side_stream(streams, kind):
    """h.set_stream(S) explicitly, unrelated delay work queued on S, then the NumPy paths: each returns the fresh handle's bits and has waited for S
    (an event recorded behind the delay has completed on return)."""
    import torch
    S = streams[0]
    p = R.problem(kind)
    want = R.fresh(kind, 1).res
    seconds = 4.0 * SC.floor_seconds()

    def behind_a_delay(call):
        with torch.cuda.stream(S):
            SC.delay(seconds)
            ev = torch.cuda.Event()
            ev.record()
        r = call()
        assert ev.query(), "a host-array call returned before its stream had drained"
        return r

    with R.open_handle(kind) as h:
        h.set_stream(S.cuda_stream)
        behind_a_delay(lambda: R.set_problem(h, p))
        sol = behind_a_delay(lambda: h.forward(p.w))
        lrow = behind_a_delay(lambda: R.loss_row(h, kind, p.w))
        grow = behind_a_delay(lambda: R.grad_row(h, kind, p.w))
        R.same((sol, lrow, grow), want, "host arrays on a side stream")
        e = behind_a_delay(lambda: R.embed(h, kind, 200))
        S.synchronize()
    with R.open_handle(kind) as f:
        R.same(e, R.embed(f, kind, 200), "the embedding call with host arrays on a side stream")
    R.hold(kind, (sol, lrow, grow), tag="streams/f")


# ---- g. two handles on two streams ------------------------------------------------------------------------------------------------------------------------
def test_g_two_handles_two_streams(streams):
    """A net-split handle on S1 with P1 and an fc32 handle on S2 with P2, their calls enqueued alternately with no synchronisation: with the null
    stream three streams, under the four hardware queues a process gets by default."""
    import torch
    S1, S2 = streams
    k1, k2 = "netsplit", "fc32"
    l1 = SC.Late(**SC.problem_pairs(k1))
    p2, p1_of_2 = R.problem(k2, 2), R.problem(k2, 1)
    l2 = SC.Late(x0=(p2.x0, p1_of_2.x0), bcs=(p2.bcs, p1_of_2.bcs), truth=(p2.truth, p1_of_2.truth), w=(p2.w, SC.half(p2.w)))
    seconds = 4.0 * 2.0 * SC.floor_seconds()
    with SC.two(R.open_handle(k1), R.open_handle(k2)) as (h1, h2):
        _warm(k1, 2)(h1)
        _warm(k2, 1)(h2)
        torch.cuda.synchronize()
        r1, r2 = [], []
        with SC.no_gc():
            with torch.cuda.stream(S1):
                st1 = SC.Still(l1.arrive(seconds))
            with torch.cuda.stream(S2):
                st2 = SC.Still(l2.arrive(seconds))
            for step in ("set_problem", "forward", "loss", "loss_grad"):
                for S, h, kind, t, st, r in ((S1, h1, k1, l1, st1, r1), (S2, h2, k2, l2, st2, r2)):
                    with torch.cuda.stream(S):
                        if step == "set_problem":
                            h.set_problem(t["x0"], t["bcs"], t["truth"])
                        elif step == "forward":
                            r.append(h.forward(t["w"]))
                        else:
                            r.append(getattr(h, step)(t["w"], R.scalings(kind)))
                        st("%s_dev of the %s handle" % (step, kind))
        S1.synchronize()
        S2.synchronize()
        g1, g2 = SC.rows(k1, SC.to_numpy(r1)), SC.rows(k2, SC.to_numpy(r2))
    R.same(g1, R.fresh(k1, 1).res, "net-split handle on S1")
    R.same(g2, R.fresh(k2, 2).res, "fc32 handle on S2")
    R.hold(k1, g1, tag="streams/g")
    R.hold(k2, g2, which=2, tag="streams/g")
