"""The late-inputs harness of tests/test_gpu_streams.py.  A helper, not a test.

include/colnde.h promises that a `_dev` entry point enqueues its work on the handle's stream.  On torch's default (null) stream that cannot be
seen: the null stream orders itself against everything.  Here a call runs under `torch.cuda.stream(S)` on a non-blocking side stream S, and the
device tensors it reads are filled LATE, in stream order:

    S:  delay | copy_(real data from pinned memory, non_blocking) | event | the library's calls ...

Until the copies run the tensors hold stale but valid data (the kind's other problem P2, half the weights: finite, inside every stability bound — a
kernel never reads poison).  Whatever the library issues off S — a launch, a fill, an upload on the null stream — runs during the delay and reads the
stale data or misses a write, and the result differs from the bits of a fresh handle on the null stream (reuse_cases.fresh), which the caller of
`late_inputs` compares.  The condition that gives this its power is an event, not a number: behind the copies an event is recorded, and after a call
that the header documents as not synchronising has returned, `event.query()` must still be False (`still`); a delay that ran out fails the test.

The delay: `torch.cuda._sleep` (a chain of matmuls where torch has none), calibrated once per process with HIP events; its length is four times the host
time the same calls took to enqueue on the null stream on a handle in the same state (time.perf_counter), and never less than four times the
enqueue time of the longest warmed sequence (`floor_seconds`: problem, solve, loss, gradient and three training steps on the net-split handle), so that a
slow host still has everything enqueued before the inputs arrive.  Both go to the errors record (tests/test_gpu_parity._record)."""
import contextlib
import functools
import gc
import time

import numpy as np

from tests import reuse_cases as R
from tests.reuse_cases import KINDS
from tests.test_gpu_parity import _record


def _torch():
    import torch
    return torch


# ---- the delay -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matmul_operand():
    torch = _torch()
    return torch.ones((512, 512), dtype=torch.float32, device="cuda")


def _spin(units):
    """`units` of delay on the current stream"""
    torch = _torch()
    if units <= 0:
        return
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        a = _matmul_operand()
        for _ in range(int(units)):
            a.mm(a)


@functools.lru_cache(maxsize=None)
def units_per_ms():
    """units of `_spin` per millisecond of device time: measured once with HIP events, on a run of at least 5 ms"""
    torch = _torch()
    n = 1_000_000 if hasattr(torch.cuda, "_sleep") else 16
    _spin(n)
    torch.cuda.synchronize()
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _spin(n)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 5.0:
            break
        n *= 4
    assert ms > 0.0
    _record("streams/delay_calibration", units=n, ms=ms, units_per_ms=n / ms)
    return n / ms


def delay(seconds):
    """a delay of that length on the current stream"""
    _spin(max(1, int(seconds * 1e3 * units_per_ms())))


# ---- tensors whose data arrives late ----------------------------------------------------------------------------------------------------------------
class Late:
    """Device tensors `dev[name]` that hold `stale` data until `arrive` copies the real data in, in stream order, from pinned host memory.  The
    tensors are views of ONE device buffer (each 256-byte aligned) and arrive with ONE copy: every copy that waits behind the delay keeps a copy
    engine of its own, and an engine's first use costs the host milliseconds to tens of milliseconds (measured: 6 and 62 ms) — more than any delay
    sized by a warmed enqueue time."""
    ALIGN = 64                                                             # floats

    def __init__(self, **pairs):
        torch = _torch()
        self.shape, self.off, n = {}, {}, 0
        for name, (real, stale) in pairs.items():
            real, stale = np.ascontiguousarray(real), np.ascontiguousarray(stale)
            assert real.shape == stale.shape and real.dtype == stale.dtype == np.float32 and np.isfinite(stale).all(), name
            assert not np.array_equal(real, stale) or name == "bcs", name
            self.shape[name], self.off[name] = real.shape, n
            n += -(-real.size // self.ALIGN) * self.ALIGN
        real_all, stale_all = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for name, (real, stale) in pairs.items():
            o, k = self.off[name], np.asarray(real).size
            real_all[o:o + k], stale_all[o:o + k] = np.asarray(real).ravel(), np.asarray(stale).ravel()
        self.stale = torch.from_numpy(stale_all)
        self.pin = torch.from_numpy(real_all).pin_memory()
        self.all = self.stale.cuda()
        self.dev = {name: self.all[o:o + int(np.prod(self.shape[name]))].view(self.shape[name]) for name, o in self.off.items()}
        torch.cuda.synchronize()

    def __getitem__(self, name):
        return self.dev[name]

    def reset(self):
        """the stale data again (blocking)"""
        self.all.copy_(self.stale)
        _torch().cuda.synchronize()

    def arrive(self, seconds=0.0):
        """On the current stream: the delay, the copy, and an event behind it (returned)."""
        torch = _torch()
        if seconds > 0.0:
            delay(seconds)
        self.all.copy_(self.pin, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev


def half(a):
    """stale data for an array: half of it (weights, constants, ocean states and fluxes stay valid under it)"""
    return (np.float32(0.5) * np.asarray(a, np.float32)).astype(np.float32)


def problem_pairs(kind, weights=True):
    """x0, bcs, truth: P1 over P2; w: P1's weights over half of them"""
    p1, p2 = R.problem(kind, 1), R.problem(kind, 2)
    pairs = dict(x0=(p1.x0, p2.x0), bcs=(p1.bcs, p2.bcs), truth=(p1.truth, p2.truth))
    if weights:
        pairs["w"] = (p1.w, half(p1.w))
    return pairs


class Still:
    """`still(name)`: the call `name`, documented as not synchronising, has returned — the late inputs must not have arrived yet.  first_only: only the
    first call is held to that (a cold handle allocates, plans and uploads in the later ones, and may wait for the stream there)."""

    def __init__(self, event=None, first_only=False, exempt=()):
        self.event, self.first_only, self.exempt, self.calls, self.t0 = event, first_only, tuple(exempt), [], time.perf_counter()

    def __call__(self, name):
        self.calls.append(name)
        if self.event is None or name in self.exempt or (self.first_only and len(self.calls) > 1):
            return
        assert not self.event.query(), ("the late inputs had arrived when %s returned (call %d of the sequence, %.2f ms after the delay was enqueued): the "
                                        "call waited for the stream, or the delay ran out — either way nothing is shown"
                                        % (name, len(self.calls), 1e3 * (time.perf_counter() - self.t0)))


def to_numpy(res):
    torch = _torch()
    return tuple(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in res)


@functools.lru_cache(maxsize=None)
def floor_seconds():
    """Host seconds to enqueue the longest warmed sequence on the null stream: the problem from device tensors, forward, loss, loss_grad and three
    training steps on the net-split handle."""
    torch = _torch()
    kind = "netsplit"
    late = Late(**problem_pairs(kind))

    def body(h):
        run_dev(h, kind, late.dev, Still())
        train_single(h, kind, late.dev, Still())

    with R.open_handle(kind) as h:
        R.set_problem(h, R.problem(kind, 2))
        body(h)
        torch.cuda.synchronize()
        dt = 0.0
        for _ in range(5):                                                 # the slowest of five: the host is not always equally quick
            late.reset()
            t0 = time.perf_counter()
            late.arrive()
            body(h)
            dt = max(dt, time.perf_counter() - t0)
            torch.cuda.synchronize()
    _record("streams/floor", enqueue_seconds=dt, delay_seconds=4 * dt)
    return dt


def side_streams():
    """Two non-blocking side streams that have been used before a test relies on them (a stream's first delay and the first use of a copy engine
    each cost the host milliseconds, which no delay sized by a warmed enqueue time covers); the delay is calibrated and the floor measured before."""
    torch = _torch()
    units_per_ms()
    floor_seconds()
    ss = torch.cuda.Stream(), torch.cuda.Stream()
    # copies of 256 B, 32 KiB and 1 MiB (the runtime moves small and large ones by different means), eight of each waiting at once behind a delay on
    # one stream while the other stream copies too: the copy engines the tests can meet have had their first use
    waiting, moving = ([Late(x=(np.ones(n, np.float32), np.zeros(n, np.float32))) for n in (64, 8192, 262144) for _ in range(8)] for _ in range(2))
    for a, b in (ss, ss[::-1]):
        with torch.cuda.stream(a):
            delay(16.0 * floor_seconds())
            for l in waiting:
                l.arrive()
        with torch.cuda.stream(b):
            for l in moving:
                l["x"].clone()
                l.arrive()
        a.synchronize()
        b.synchronize()
    return ss


@contextlib.contextmanager
def no_gc():
    """no garbage collection between a delay and the calls behind it: a collection is a host pause the delay was not sized for"""
    on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if on:
            gc.enable()


def late_inputs(S, make, late, body, warm=None, tag="", first_only=False, exempt=(), side=None):
    """The sequence `body(h, late.dev, still)` behind late inputs on the side stream S, and the same on the null stream.
    make(): a new handle (a context manager); warm(h): what it has done before, on the null stream.  The null-stream run comes first, on a handle of
    its own in the same state: it is timed for the delay and its results are returned as the reference.  side(h, late, seconds, body): another way
    to run the side-stream part than `with torch.cuda.stream(S): arrive; body` (sequences e, f and the power check).
    Returns (got, ref): tuples of NumPy arrays."""
    torch = _torch()
    with make() as h0:
        if warm:
            warm(h0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        late.arrive()
        ref = body(h0, late.dev, Still())
        enq = time.perf_counter() - t0
        torch.cuda.synchronize()
        ref = to_numpy(ref)
    late.reset()
    seconds = 4.0 * max(enq, floor_seconds())
    with make() as h:
        if warm:
            warm(h)
        torch.cuda.synchronize()
        with no_gc():
            if side is not None:
                got = side(h, late, seconds, body)
            else:
                with torch.cuda.stream(S):
                    still = Still(late.arrive(seconds), first_only, exempt)
                    got = body(h, late.dev, still)
                assert still.calls, "the sequence never said which call must not wait"
        S.synchronize()
        torch.cuda.synchronize()
        got = to_numpy(got)
    _record("streams/%s" % tag, enqueue_seconds=enq, delay_seconds=seconds)
    return got, ref


# ---- the sequences' bodies ----------------------------------------------------------------------------------------------------------------------------
def rows(kind, res):
    """(sol, loss, loss_grad) of the device calls as reuse_cases.run's rows: a single handle's [terms(6); total; 0] and [grad; terms(6); total; 0] lose
    the trailing 0, the K-row kinds keep the library's rows"""
    sol, l, g = res
    if KINDS[kind]["family"] != "single":
        return sol, l, g
    return sol, l[:7], g[:-1]


def run_dev(h, kind, t, still, set_problem=True):
    """reuse_cases.run through the `_dev` paths: the problem and the weights from the device tensors t"""
    sc = R.scalings(kind)
    if set_problem:
        h.set_problem(t["x0"], t["bcs"], t["truth"])
        still("set_problem_dev")
    sol = h.forward(t["w"])
    still("forward_dev")
    l = h.loss(t["w"], sc)
    still("loss_dev")
    g = h.loss_grad(t["w"], sc)
    still("loss_grad_dev")
    return sol, l, g


ETA = 1e-3
ETAS = np.float32([1e-3, 3e-3, 3e-4])              # per-model rates of the ensembles (the first K)
COEFF = np.float32([1e-4, 3e-4])                   # per-model causal-penalty coefficients of the free-convection ensemble


def train_single(h, kind, t, still, steps=3):
    """`steps` iterations of loss_grad and ColumnNDE.adam_step on t["w"] (in place) with no synchronisation: (w, m, v, last result)"""
    torch = _torch()
    w = t["w"]
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    out = torch.empty(w.numel() + 8, dtype=torch.float32, device=w.device)
    b1t, b2t = 0.9, 0.999
    for _ in range(steps):
        h.loss_grad(w, R.scalings(kind), out=out)
        still("loss_grad_dev")
        h.adam_step(w, out, m, v, ETA, beta_t=(b1t, b2t))
        still("adam_step_dev")
        b1t, b2t = b1t * 0.9, b2t * 0.999
    return w, m, v, out


def train_rows(h, kind, t, still, steps=3):
    """The same for an ensemble: per-model rates t["etas"]; the free-convection ensemble adds causal_penalty to every gradient and ends with column_loss"""
    torch = _torch()
    w = t["w"]
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    out = torch.empty((w.shape[0], w.shape[1] + 8), dtype=torch.float32, device=w.device)
    b1t, b2t = 0.9, 0.999
    fc = KINDS[kind]["family"] == "fc_ens"
    for _ in range(steps):
        h.loss_grad(w, R.scalings(kind), out=out)
        still("ensemble_loss_grad_dev")
        if fc:
            h.causal_penalty(w, t["coeff"], out)
            still("ensemble_causal_penalty_dev")
        h.adam_step(w, out, m, v, t["etas"], beta_t=(b1t, b2t))
        still("ensemble_adam_step_dev")
        b1t, b2t = b1t * 0.9, b2t * 0.999
    res = (w, m, v, out)
    if fc:
        sol = h.forward(w)
        still("ensemble_forward_dev")
        res += (sol, h.column_loss(sol))
        still("ensemble_column_loss_dev")
    return res


def embed_pairs(kind, n=200):
    """the array arguments of reuse_cases.embed_call as Late pairs (real over half of it), and how to call with the device tensors in their place"""
    name, args, kwargs, arrays = R.embed_call(kind, n)
    key = lambda a: "a_%s" % ("_".join(str(x) for x in a) if isinstance(a, tuple) else a)
    get = lambda a: args[a] if isinstance(a, int) else kwargs[a[0]][a[1]] if isinstance(a, tuple) else kwargs[a]
    pairs = {key(a): (get(a), half(get(a))) for a in arrays}

    def call(h, t):
        ar, kw = list(args), dict(kwargs)
        for a in arrays:
            if isinstance(a, int):
                ar[a] = t[key(a)]
            elif isinstance(a, tuple):
                pair = list(kw[a[0]])
                pair[a[1]] = t[key(a)]
                kw[a[0]] = tuple(pair)
            else:
                kw[a] = t[key(a)]
        return R.flat(getattr(h, name)(*ar, **kw))

    return name, pairs, call


@contextlib.contextmanager
def two(a, b):
    with a as x, b as y:
        yield x, y
