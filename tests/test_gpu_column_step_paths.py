"""The kernels either side of the hot path (csrc/column_ops.hip) on the paths the callers' pointers select: `launch_convective_adjustment` and
`launch_mpp_diffusion` run their LDS-tiled kernels only at Nz in {16, 32, 64} with every pointer 16-byte aligned and the one-thread-per-column
generic kernels otherwise; `launch_mpp_diagnose_flux` sets `vec_in` / `vec_out` from the alignment and runs `mpp_diagnose_flux_kernel<0>` (run-time
Nz, LDS attribute per launch) at any other Nz.  A contiguous view at an odd float offset of a larger buffer passes `ColumnNDE._chk_dev` — an interior
slice of a state with halos is such a view — so every side of those choices is a supported call.

Every case here goes through `offset_view`: a flat device buffer filled with a sentinel, the array copied in at a chosen float offset.  The helper
asserts the address bits the dispatch reads, so a case cannot be vacuous about the kernel it selected; after every call the head and the tail of
every output buffer must still hold the sentinel bit for bit, and every input that is not an output must equal its clone.

References and tolerances are the ones these entry points already carry: `orc.convective_adjustment` at 2e-5 max|want| (tests/test_column_ops.py),
`orc.modified_pacanowski_philander_step` at (2e-5, 2e-5, 2e-6) of the range (same file), `diagnose_baseline_flux` of tests/wm_diag_restatement.py at
`BASE_BOUND` (tests/test_gpu_wm_diag.py).  The fallback paths get the bound of the tiled one.  Inputs: `_columns`, `_uvT` (test_column_ops) and
`_case` (test_gpu_wm_diag); float32 and float64 take the same `Ri > 0` branch on every face (`_same_branches`, asserted), and the sign of
T[k+1] − T[k−1] is exact in float32, so no case is left out for sitting on a branch.

The flux diagnosis at Nz outside {16, 32, 64} has no `BASE_BOUND` entry.  `DIAG_RT_BOUND` below holds 10 x the largest max|gpu − f64| / max|f64|
measured on an MI355X over n in {1, 130}, aligned and offset, halo given and absent; every run records them again (COLNDE_RECORD_ERRORS=1), with the
tiled-vs-fallback differences, which are recorded and not asserted (separate kernels: the compiler may contract them differently).  On the MI355X
every one of those differences was exactly zero: at Nz = 16, 32, 64 the generic kernels returned the tiled kernels' bits, and the scalar copies of
the diagnosis (`vec_in = 0`, `vec_out = 0`) the vector copies' bits."""
import functools

import numpy as np
import pytest

from colnde import synthetic
from oracle import nde_oracle as orc
from tests import wm_diag_restatement as R
from tests import wm_embed_common as W
from tests.test_column_ops import MPP, _columns, _mpp_params, _uvT
from tests.test_gpu_parity import _record
from tests.test_gpu_wm_diag import BASE_BOUND, FIELDS, _case, _same_branches

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
TILED_NZ = (16, 32, 64)
RT_NZ = (4, 5, 127, 128)                       # the ends of the accepted range and an odd size next to each
N_BATCH = 130                                  # two full 64-column blocks and a ragged one of two columns
CA_DT, CA_K = 1200.0, 10.0                     # as test_gpu_convective_adjustment_matches_oracle
MPP_DT = 60.0                                  # as test_gpu_implicit_diffusion_matches_oracle
MPP_TOL = (2e-5, 2e-5, 2e-6)

# mpp_diagnose_flux_kernel<0>, (uw, vw, wT) per (Nz, ca): 10 x the value measured on an MI355X (in the comment beside each row: the largest over the
# cases of test_diagnosis_at_run_time_nz), but never looser than the loosest BASE_BOUND entry of the same ca, (2.29e-7, 3.07e-6, 3.69e-6) for both:
# the entries marked * are held at that cap, 5.3 to 7.5 x what was measured.
DIAG_RT_BOUND = {
    (4, 0): (8.34e-11, 1.17e-6, 1.77e-8),      # 8.34e-12, 1.17e-7, 1.77e-9
    (4, 1): (8.34e-11, 1.17e-6, 1.77e-8),      # 8.34e-12, 1.17e-7, 1.77e-9
    (5, 0): (4.34e-9, 3.07e-6, 5.45e-7),       # 4.34e-10, 4.12e-7 *, 5.45e-8
    (5, 1): (4.34e-9, 3.07e-6, 5.45e-7),       # 4.34e-10, 4.12e-7 *, 5.45e-8
    (20, 0): (1.33e-7, 1.38e-6, 2.88e-6),      # 1.33e-8, 1.38e-7, 2.88e-7
    (20, 1): (1.33e-7, 1.38e-6, 1.64e-6),      # 1.33e-8, 1.38e-7, 1.64e-7
    (127, 0): (2.29e-7, 1.30e-6, 9.72e-7),     # 4.30e-8 *, 1.30e-7, 9.72e-8
    (127, 1): (2.29e-7, 1.30e-6, 8.83e-9),     # 4.30e-8 *, 1.30e-7, 8.83e-10
    (128, 0): (2.29e-7, 1.33e-6, 7.54e-7),     # 3.30e-8 *, 1.33e-7, 7.54e-8
    (128, 1): (2.29e-7, 1.33e-6, 2.04e-8),     # 3.30e-8 *, 1.33e-7, 2.04e-9
}


# ---------------------------------------------------------------------------------------------- the offset-view helper
def offset_view(a, off, head=16, tail=160, fill=SENTINEL):
    """(buf, view): one flat device buffer filled with `fill`, `a` copied in at float offset head + off; view is contiguous, of a's shape, and its
    address has the bits (4 off) % 16 the dispatch reads (asserted).  The tail is longer than the longest row (129 faces)."""
    import torch
    a = np.array(a, dtype=np.float32, order="C")                                # (a copy: the shared inputs are read-only)
    assert head % 4 == 0 and off >= 0
    buf = torch.full((head + off + a.size + tail,), fill, dtype=torch.float32, device="cuda")
    view = buf[head + off:head + off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and tuple(view.shape) == a.shape
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 * off) % 16
    return buf, view


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def guards_intact(buf, view, fill=SENTINEL):
    """The floats of buf before and behind view still hold the sentinel, bit for bit."""
    start = (view.data_ptr() - buf.data_ptr()) // 4
    raw = _bits(buf)
    want = int(np.float32(fill).view(np.int32))
    return bool((raw[:start] == want).all()) and bool((raw[start + view.numel():] == want).all())


class _Call:
    """The device arrays of one call: outputs keep their guard buffers, inputs a clone taken before the call."""

    def __init__(self):
        self.outs, self.ins = [], []

    def inp(self, a, off=0):
        if a is None:
            return None
        _, v = offset_view(a, off)
        self.ins.append((v, v.clone()))
        return v

    def out(self, shape, off=0):
        buf, v = offset_view(np.full(shape, np.nan, np.float32), off)        # NaN: an element the kernel leaves out shows
        self.outs.append((buf, v))
        return v

    def inout(self, a, off=0):
        buf, v = offset_view(a, off)
        self.outs.append((buf, v))
        return v

    def check(self):
        import torch
        torch.cuda.synchronize()
        for buf, v in self.outs:
            assert guards_intact(buf, v), "an output's head or tail was written"
        for v, c in self.ins:
            assert torch.equal(_bits(v), _bits(c)), "an input was modified"


@pytest.fixture(scope="module")
def handle():
    """One handle per Nz for the whole module (any model kind: only Nz is the handle's; small layers keep creation cheap at Nz = 128)."""
    import colnde
    made = {}

    def get(Nz):
        if Nz not in made:
            made[Nz] = colnde.ColumnNDE(_handle_cfg(Nz), 1)
        return made[Nz]
    yield get
    for h in made.values():
        h.close()


def _handle_cfg(Nz):
    return synthetic.free_convection_problem(1, Nz=Nz, n_save=2, layer_sizes=(Nz, 8, 8, Nz - 1)).cfg


def _frozen(*arrs):
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, dict):
            _frozen(*a.values())
        elif isinstance(a, (tuple, list)):
            _frozen(*a)
    return arrs


def _rel(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


# ---------------------------------------------------------------------------------------------- convective adjustment
CA_ALIGN = ((0, 0), (1, 0), (0, 2), (3, 3))                                   # float offsets of (T, out)


def _ca_kernel(Nz, off_T, off_out):
    return "tiled" if Nz in TILED_NZ and off_T % 4 == 0 and off_out % 4 == 0 else "generic"


def _few_levels(gen, n, Nz, *args):
    """The generator's columns; at Nz < 16 the deepest Nz levels of its 32-level columns.  Its own 4- and 5-level columns have no unstable cell (6.7
    and 5 K per level under 1.5 K of noise; 0.1 K per level under 0.02 K), so neither the adjustment nor the `Ri > 0` switch would run there."""
    if Nz >= 16:
        return gen(n, Nz, *args)
    a = gen(n, 32, *args)
    return tuple(np.ascontiguousarray(x[:, :Nz]) for x in a) if isinstance(a, tuple) else np.ascontiguousarray(a[:, :Nz])


def _unstable_cells(T):
    """κ's switch with the zero-gradient halos: the sign of T[k+1] − T[k−1], exact in float32."""
    ext = np.concatenate([T[:, :1], T, T[:, -1:]], axis=1)
    return ext[:, 2:] - ext[:, :-2] < 0


@functools.lru_cache(maxsize=None)
def _ca_inputs(Nz, n):
    """(T, halo_bottom, halo_top, dz, {halo: float64 reference}, stable T): computed once, shared, read-only.  Every batch, and the lone column (the
    first column of the N_BATCH batch that has both), holds unstable and stable cells."""
    if n == 1:
        T, hb, ht = _ca_inputs(Nz, N_BATCH)[:3]
        u = _unstable_cells(T)
        j = int(np.argmax(u.any(axis=1) & ~u.all(axis=1)))
        T, hb, ht = T[j:j + 1].copy(), hb[j:j + 1].copy(), ht[j:j + 1].copy()
    else:
        rng = np.random.default_rng(300 + Nz + n)
        T = _few_levels(_columns, n, Nz)
        hb = (T[:, 0] + rng.standard_normal(n)).astype(np.float32)
        ht = (T[:, -1] + rng.standard_normal(n)).astype(np.float32)
    u = _unstable_cells(T)
    assert u.any() and not u.all()
    dz = 2000.0 / Nz
    want = {0: orc.convective_adjustment(T, CA_DT, dz, CA_K), 1: orc.convective_adjustment(T, CA_DT, dz, CA_K, hb, ht)}
    return _frozen(T, hb, ht, dz, want, _few_levels(_columns, n, Nz, False))


def _run_ca(nde, T, hb, ht, dz, off_T, off_out, in_place=False):
    c = _Call()
    Td = c.inout(T, off_T) if in_place else c.inp(T, off_T)
    out = Td if in_place else c.out(T.shape, off_out)
    r = nde.convective_adjustment(Td, CA_DT, dz, CA_K, c.inp(hb), c.inp(ht), out=out)
    assert r is out
    c.check()
    return out.cpu().numpy()


def _check_ca(nde, Nz, n, aligns):
    T, hb, ht, dz, want, Ts = _ca_inputs(Nz, n)
    for halo in (0, 1):
        got = {}
        for off_T, off_out in aligns:
            kern = _ca_kernel(Nz, off_T, off_out)
            g = _run_ca(nde, T, hb if halo else None, ht if halo else None, dz, off_T, off_out)
            err = _rel(g, want[halo])
            print("convective_adjustment Nz=%d n=%d halo=%d T+%d out+%d -> %s: rel err %.3e" % (Nz, n, halo, off_T, off_out, kern, err))
            _record("column_step/convadj/%s/%d/%d/%d/%d%d" % (kern, Nz, n, halo, off_T, off_out), rel=err)
            assert np.abs(g - want[halo]).max() <= 2e-5 * np.abs(want[halo]).max(), (kern, off_T, off_out, err)
            got[(off_T, off_out)] = g
        if _ca_kernel(Nz, 0, 0) == "tiled" and (0, 0) in got:
            d = max(_rel(g, got[(0, 0)].astype(np.float64)) for k, g in got.items() if k != (0, 0))
            print("convective_adjustment Nz=%d n=%d halo=%d: tiled vs generic %.3e of max|out|" % (Nz, n, halo, d))
            _record("column_step/convadj/tiled_vs_generic/%d/%d/%d" % (Nz, n, halo), rel=d)
    for off_T, off_out in (aligns[0], aligns[-1]):                            # stable columns come back bit for bit, on both paths
        assert np.array_equal(_run_ca(nde, Ts, None, None, dz, off_T, off_out), Ts), _ca_kernel(Nz, off_T, off_out)


@pytest.mark.parametrize("n", [1, 65, 130, 257])                              # 257: the generic kernel's blocks are 256 columns wide
@pytest.mark.parametrize("Nz", TILED_NZ)
def test_convective_adjustment_both_paths(handle, Nz, n):
    _check_ca(handle(Nz), Nz, n, CA_ALIGN)


@pytest.mark.parametrize("n", [1, N_BATCH])
@pytest.mark.parametrize("Nz", RT_NZ)
def test_convective_adjustment_at_the_ends_of_the_range(handle, Nz, n):
    _check_ca(handle(Nz), Nz, n, ((0, 0), (1, 1)))


# ---------------------------------------------------------------------------------------------- implicit diffusion
# float offsets of (u, v, T, u_out, v_out, T_out): the dispatch ORs the six pointers, so one stray pointer must be enough
MPP_ALIGN = {"aligned": (0,) * 6, "v+1": (0, 1, 0, 0, 0, 0), "T_out+2": (0, 0, 0, 0, 0, 2), "all+3": (3,) * 6}


def _mpp_kernel(Nz, offs):
    return "tiled" if Nz in TILED_NZ and all(o % 4 == 0 for o in offs) else "generic"


@functools.lru_cache(maxsize=None)
def _mpp_inputs(Nz, n):
    """(u, v, T, halo_bottom [3, n], dz, {(ca, halo): float64 reference}): computed once, shared, read-only.  Every batch takes both `Ri > 0`
    branches among its interior faces."""
    rng = np.random.default_rng(100 + Nz + n)
    u, v, T = _few_levels(_uvT, n, Nz, rng)
    dz = 256.0 / Nz
    hb = np.stack([u[:, 0] - 1e-3, v[:, 0] + 2e-3, T[:, 0] + np.where(np.arange(n) % 2, 0.01, -0.01)]).astype(np.float32)
    want = {}
    for halo in (0, 1):
        interior = _same_branches(u, v, T, dz, (hb, None) if halo else None)[:, 1:Nz]
        assert n == 1 or (interior.any() and not interior.all())
        for ca in (False, True):
            want[(ca, halo)] = orc.modified_pacanowski_philander_step(u, v, T, MPP_DT, dz, convective_adjustment=ca, halo_bottom=hb if halo else None, **MPP)
    return _frozen(u, v, T, hb, dz, want)


def _run_mpp(nde, u, v, T, hb, dz, params, ca, offs, in_place=False):
    c = _Call()
    ins = tuple((c.inout if in_place else c.inp)(a, o) for a, o in zip((u, v, T), offs[:3]))
    outs = ins if in_place else tuple(c.out(T.shape, o) for o in offs[3:])
    r = nde.implicit_diffusion(ins[0], ins[1], ins[2], MPP_DT, dz, params, ca, c.inp(hb), out=outs)
    assert all(a is b for a, b in zip(r, outs))
    c.check()
    return tuple(o.cpu().numpy() for o in outs)


def _check_mpp(nde, Nz, n, aligns):
    u, v, T, hb, dz, want = _mpp_inputs(Nz, n)
    for ca in (False, True):
        for halo in (0, 1):
            got = {}
            for name, offs in aligns.items():
                kern = _mpp_kernel(Nz, offs)
                g = _run_mpp(nde, u, v, T, hb if halo else None, dz, _mpp_params(), ca, offs)
                errs = [_rel(a, w) for a, w in zip(g, want[(ca, halo)])]
                print("implicit_diffusion Nz=%d n=%d ca=%d halo=%d %s -> %s: rel err u %.3e v %.3e T %.3e" % ((Nz, n, ca, halo, name, kern) + tuple(errs)))
                _record("column_step/mpp_diffusion/%s/%d/%d/%d/%d/%s" % (kern, Nz, n, ca, halo, name), u=errs[0], v=errs[1], T=errs[2])
                for a, w, tol in zip(g, want[(ca, halo)], MPP_TOL):
                    assert np.isfinite(a).all()
                    assert np.abs(a - w).max() <= tol * np.abs(w).max(), (kern, name, np.abs(a - w).max(), np.abs(w).max())
                assert np.array_equal(g[2][:, 0], T[:, 0])                    # T′[1] = T_bottom, bit for bit
                got[name] = g
            if _mpp_kernel(Nz, (0,) * 6) == "tiled" and "aligned" in got:
                d = [max(_rel(g[f], got["aligned"][f].astype(np.float64)) for k, g in got.items() if k != "aligned") for f in range(3)]
                print("implicit_diffusion Nz=%d n=%d ca=%d halo=%d: tiled vs generic u %.3e v %.3e T %.3e of max|out|" % ((Nz, n, ca, halo) + tuple(d)))
                _record("column_step/mpp_diffusion/tiled_vs_generic/%d/%d/%d/%d" % (Nz, n, ca, halo), u=d[0], v=d[1], T=d[2])
    names = list(aligns)
    for name in (names[0], names[-1]):                                        # nothing to diffuse: a bit-identical pass-through, on both paths
        z = _run_mpp(nde, u, v, T, None, dz, (0.0, 0.0, 1.0, 0.25, 1.0, MPP["alpha"], MPP["g"]), False, aligns[name])
        assert all(np.array_equal(a, b) for a, b in zip(z, (u, v, T))), _mpp_kernel(Nz, aligns[name])


@pytest.mark.parametrize("n", [1, 65, N_BATCH])
@pytest.mark.parametrize("Nz", TILED_NZ)
def test_implicit_diffusion_both_paths(handle, Nz, n):
    _check_mpp(handle(Nz), Nz, n, MPP_ALIGN)


@pytest.mark.parametrize("n", [1, N_BATCH])
@pytest.mark.parametrize("Nz", RT_NZ)
def test_implicit_diffusion_at_the_ends_of_the_range(handle, Nz, n):
    _check_mpp(handle(Nz), Nz, n, {"aligned": (0,) * 6, "all+1": (1,) * 6})


# ---------------------------------------------------------------------------------------------- flux diagnosis
DG_ALIGN = ((0, 0), (1, 0), (0, 1), (1, 1))                                   # float offsets of (u, v, T) and of (uw, vw, wT)


def _dg_kernel(Nz, off_in, off_out):
    return "%s/vec_in=%d/vec_out=%d" % ("<%d>" % Nz if Nz in TILED_NZ else "<0>", int(Nz % 4 == 0 and off_in % 4 == 0), int(off_out % 4 == 0))


@functools.lru_cache(maxsize=None)
def _dg_inputs(Nz, n):
    """(u, v, T, top [3, n], halo_bottom [3, n], dz, {(ca, halo): float64 reference}): the first n of N_BATCH columns; shared, read-only."""
    _, (u, v, T, top, hb, _) = _case(n, Nz, N_BATCH)
    dz = W.LZ / Nz
    want = {}
    for halo in (0, 1):
        halos = (hb, None) if halo else None
        _same_branches(u, v, T, dz, halos)
        for ca in (0, 1):
            want[(ca, halo)] = R.diagnose_baseline_flux(u, v, T, top, dz, W.MPP, bool(ca), halos)
    return _frozen(u, v, T, top, hb, dz, want)


def _dg_errors(got, want, batch):
    """max|gpu − f64| over the n columns given / max|f64| over the N_BATCH columns they are the first of, per field.  BASE_BOUND is relative to the
    field's largest face over a batch of columns (77 there); the first column on its own has no such scale — its vw, whose top flux is zero, is
    all cancellation, and a float32 NumPy run of the restatement is itself 2e-5 of that column's own max|vw| away from float64.  So every n is held
    to the absolute tolerance the same columns get inside the batch; at n = N_BATCH this is `_errors` of tests/test_gpu_wm_diag.py."""
    return [float(np.abs(g.astype(np.float64) - w).max() / np.abs(b).max()) for g, w, b in zip(got, want, batch)]


def _run_dg(nde, u, v, T, top, hb, dz, ca, off_in, off_out):
    c = _Call()
    ins = tuple(c.inp(a, off_in) for a in (u, v, T))
    outs = tuple(c.out((T.shape[0], T.shape[1] + 1), off_out) for _ in range(3))
    r = nde.mpp_diagnose_flux(ins[0], ins[1], ins[2], c.inp(top), dz, W.mpp_params(), ca, c.inp(hb), faces_out=outs)
    assert all(a is b for a, b in zip(r, outs))
    c.check()
    return tuple(o.cpu().numpy() for o in outs)


def _check_dg(nde, Nz, n, aligns, bounds):
    u, v, T, top, hb, dz, want = _dg_inputs(Nz, n)
    batch = _dg_inputs(Nz, N_BATCH)[-1]
    worst = {}
    for ca in (0, 1):
        for halo in (0, 1):
            got = {}
            for off_in, off_out in aligns:
                kern = _dg_kernel(Nz, off_in, off_out)
                g = _run_dg(nde, u, v, T, top, hb if halo else None, dz, ca, off_in, off_out)
                errs = _dg_errors(g, want[(ca, halo)], batch[(ca, halo)])
                print("mpp_diagnose_flux Nz=%d n=%d ca=%d halo=%d in+%d out+%d -> %s: rel err uw %.3e vw %.3e wT %.3e"
                      % ((Nz, n, ca, halo, off_in, off_out, kern) + tuple(errs)))
                _record("column_step/mpp_diagnose_flux/%s/%d/%d/%d/%d/%d%d" % (kern, Nz, n, ca, halo, off_in, off_out), **dict(zip(FIELDS, errs)))
                worst[ca] = [max(a, b) for a, b in zip(worst.get(ca, (0.0,) * 3), errs)]
                for k in range(3):
                    assert g[k].shape == (n, Nz + 1) and np.isfinite(g[k]).all()
                    assert np.array_equal(g[k][:, -1], top[k])                # the top face IS the given top flux, bit for bit
                for nm, e, b in zip(FIELDS, errs, bounds[(Nz, ca)]):
                    assert e <= b, (kern, nm, e, b)
                got[(off_in, off_out)] = g
            if (0, 0) in got and len(got) > 1:
                d = [max(_rel(g[f], got[(0, 0)][f].astype(np.float64)) for k, g in got.items() if k != (0, 0)) for f in range(3)]
                print("mpp_diagnose_flux Nz=%d n=%d ca=%d halo=%d: vector vs scalar copies uw %.3e vw %.3e wT %.3e of max|out|" % ((Nz, n, ca, halo) + tuple(d)))
                _record("column_step/mpp_diagnose_flux/vec_vs_scalar/%d/%d/%d/%d" % (Nz, n, ca, halo), **dict(zip(FIELDS, d)))
    for ca, w in worst.items():
        print("mpp_diagnose_flux Nz=%d n=%d ca=%d: worst rel err uw %.3e vw %.3e wT %.3e" % ((Nz, n, ca) + tuple(w)))


@pytest.mark.parametrize("n", [1, 65, N_BATCH])
@pytest.mark.parametrize("Nz", TILED_NZ)
def test_diagnosis_vector_and_scalar_copies(handle, Nz, n):
    _check_dg(handle(Nz), Nz, n, DG_ALIGN, BASE_BOUND)


@pytest.mark.parametrize("n", [1, N_BATCH])
@pytest.mark.parametrize("Nz", RT_NZ + (20,))
def test_diagnosis_at_run_time_nz(handle, Nz, n):
    _check_dg(handle(Nz), Nz, n, ((0, 0), (1, 1)), DIAG_RT_BOUND)


def test_diagnosis_at_128_levels_twice_on_a_fresh_handle():
    """3 * 64 * 129 * 4 = 99,072 bytes of LDS, above the 64 KB default: the attribute is set per launch, so the first call of a fresh handle and the
    one after it must both succeed, with the same bits."""
    import colnde
    Nz, n = 128, N_BATCH
    u, v, T, top, hb, dz, want = _dg_inputs(Nz, n)
    with colnde.ColumnNDE(_handle_cfg(Nz), 1) as nde:
        a = _run_dg(nde, u, v, T, top, hb, dz, 1, 0, 0)
        b = _run_dg(nde, u, v, T, top, hb, dz, 1, 0, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for nm, e, bd in zip(FIELDS, _dg_errors(a, want[(1, 1)], want[(1, 1)]), DIAG_RT_BOUND[(Nz, 1)]):
        assert e <= bd, (nm, e, bd)


# ---------------------------------------------------------------------------------------------- in place on the fallback path
@pytest.mark.parametrize("Nz", TILED_NZ)
def test_in_place_on_the_fallback_path(handle, Nz):
    """out = T and out = (u, v, T) on offset views (the generic kernels): the bits of the out-of-place result of the same path, tails intact."""
    nde, n = handle(Nz), N_BATCH
    T, hb, ht, dz, _, _ = _ca_inputs(Nz, n)
    assert _ca_kernel(Nz, 1, 1) == "generic"
    apart = _run_ca(nde, T, hb, ht, dz, 1, 1)
    assert np.array_equal(_run_ca(nde, T, hb, ht, dz, 1, 1, in_place=True), apart) and not np.array_equal(apart, T)
    u, v, T, hb, dz, _ = _mpp_inputs(Nz, n)
    offs = (3,) * 6
    assert _mpp_kernel(Nz, offs) == "generic"
    for ca in (False, True):
        apart = _run_mpp(nde, u, v, T, hb, dz, _mpp_params(), ca, offs)
        same = _run_mpp(nde, u, v, T, hb, dz, _mpp_params(), ca, offs, in_place=True)
        assert all(np.array_equal(a, b) for a, b in zip(same, apart)) and not np.array_equal(apart[0], u)


# ---------------------------------------------------------------------------------------------- a column's answer does not depend on where it sits
@pytest.mark.parametrize("path", ["tiled", "fallback"])
@pytest.mark.parametrize("Nz", TILED_NZ)
def test_a_column_alone_equals_the_column_in_the_batch(handle, Nz, path):
    """Column 5 (a full block) and column 129 (the ragged block) of a batch of 130 with halos against the same column and its halo cells run alone:
    one kernel, one sweep, so the bits — this pins the [3][n_col] indexing of the halo and of the top flux."""
    nde, n, off = handle(Nz), N_BATCH, 0 if path == "tiled" else 1
    one = lambda a, c: np.ascontiguousarray(a[c:c + 1])
    one3 = lambda a, c: np.ascontiguousarray(a[:, c:c + 1])
    T, hb, ht, dz, _, _ = _ca_inputs(Nz, n)
    assert _ca_kernel(Nz, off, off) == ("tiled" if path == "tiled" else "generic")
    batch = _run_ca(nde, T, hb, ht, dz, off, off)
    for c in (5, 129):
        assert np.array_equal(_run_ca(nde, one(T, c), one(hb, c), one(ht, c), dz, off, off)[0], batch[c]), c
    u, v, T, hb, dz, _ = _mpp_inputs(Nz, n)
    batch = _run_mpp(nde, u, v, T, hb, dz, _mpp_params(), True, (off,) * 6)
    for c in (5, 129):
        alone = _run_mpp(nde, one(u, c), one(v, c), one(T, c), one3(hb, c), dz, _mpp_params(), True, (off,) * 6)
        assert all(np.array_equal(a[0], b[c]) for a, b in zip(alone, batch)), c
    u, v, T, top, hb, dz, _ = _dg_inputs(Nz, n)
    batch = _run_dg(nde, u, v, T, top, hb, dz, 1, off, off)
    for c in (5, 129):
        alone = _run_dg(nde, one(u, c), one(v, c), one(T, c), one3(top, c), one3(hb, c), dz, 1, off, off)
        assert all(np.array_equal(a[0], b[c]) for a, b in zip(alone, batch)), c


# ---------------------------------------------------------------------------------------------- tails for the flat kernels of the same file
def _adam_reference(th, g, m, v, eta):
    return orc.adam_step(th.astype(np.float64), g.astype(np.float64), m.astype(np.float64), v.astype(np.float64), eta, (0.9, 0.999), 1e-8, (0.9, 0.999))[:3]


def _assert_adam(got, want):
    # the tolerances of test_gpu_adam_step_matches_oracle_over_several_steps
    np.testing.assert_allclose(got[0], want[0], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-5, atol=1e-12)


def test_adam_step_leaves_the_tails(handle):
    nde, n = handle(32), 1000                                                 # three full blocks of 256 and a ragged one
    assert n % 256 != 0
    rng = np.random.default_rng(61)
    th, g = rng.standard_normal(n).astype(np.float32), (1e-3 * rng.standard_normal(n)).astype(np.float32)
    m, v = (1e-4 * rng.standard_normal(n)).astype(np.float32), (1e-6 * rng.random(n)).astype(np.float32)
    c = _Call()
    thd, md, vd, gd = c.inout(th), c.inout(m), c.inout(v), c.inp(g)
    nde.adam_step(thd, gd, md, vd, 1e-2, (0.9, 0.999), 1e-8, beta_t=(0.9, 0.999))
    c.check()
    _assert_adam([t.cpu().numpy() for t in (thd, md, vd)], _adam_reference(th, g, m, v, 1e-2))


@functools.lru_cache(maxsize=None)
def _fc_ensemble_problem(Nz, n):
    p = synthetic.free_convection_problem(n, Nz=Nz, n_save=5, substeps=2, t_end=0.01)
    rng = np.random.default_rng(62 + Nz)
    truth = (19.5 + rng.standard_normal((n, 5, Nz))).astype(np.float32)
    return _frozen(p.cfg, p.x0, p.bcs, truth)


def test_ensemble_adam_step_leaves_the_tails_and_the_loss_slots():
    """K = 3; the gradient is read at stride n + 8 from the result rows, whose eight loss slots (and every other entry) stay as they were."""
    import colnde
    cfg, x0, bcs, truth = _fc_ensemble_problem(32, 9)
    K = 3
    rng = np.random.default_rng(63)
    with colnde.FreeConvectionEnsemble(cfg, 9, K) as e:
        n = e.n_params
        assert n % 256 != 0
        th = rng.standard_normal((K, n)).astype(np.float32)
        res = (1e-3 * rng.standard_normal((K, n + 8))).astype(np.float32)
        res[:, n:] = 1e3 + np.arange(8 * K).reshape(K, 8)                     # loss slots: a gradient read at stride n would meet these
        m, v = (1e-4 * rng.standard_normal((K, n))).astype(np.float32), (1e-6 * rng.random((K, n))).astype(np.float32)
        etas = np.array([1e-2, 3e-3, 1e-3], np.float32)
        c = _Call()
        thd, md, vd, rd, ed = c.inout(th), c.inout(m), c.inout(v), c.inp(res), c.inp(etas)
        e.adam_step(thd, rd, md, vd, ed, (0.9, 0.999), 1e-8, beta_t=(0.9, 0.999))
        c.check()
        got = [t.cpu().numpy() for t in (thd, md, vd)]
    for k in range(K):
        _assert_adam([a[k] for a in got], _adam_reference(th[k], res[k, :n], m[k], v[k], float(etas[k])))


@pytest.mark.parametrize("rows,N,n", [(3, 100, 20), (2, 50, 7)])
def test_coarse_grain_leaves_the_tail(handle, rows, N, n):
    from colnde import _lib
    nde = handle(32)
    x = np.random.default_rng(64 + n).standard_normal((rows, N)).astype(np.float32)
    c = _Call()
    xd, out = c.inp(x), c.out((rows, n))
    nde.use_torch_stream()
    _lib.check(nde._L.colnde_coarse_grain_dev(nde._h, xd.data_ptr(), rows, N, n, 1, out.data_ptr()))
    c.check()
    got = out.cpu().numpy()
    np.testing.assert_allclose(got, orc.coarse_grain_linear_interpolation_face(x, n), rtol=2e-6, atol=2e-6)     # test_data_prep's tolerance
    assert np.array_equal(got[:, 0], x[:, 0]) and np.array_equal(got[:, -1], x[:, -1])


def test_scale_leaves_the_tail(handle):
    from colnde import _lib
    nde, count = handle(32), 257                                              # one full block of 256 and one value
    data = (np.random.default_rng(65).random(count) * 3.0 + 17.0).astype(np.float32)
    want, mu, sigma = orc.zero_mean_unit_variance(data)
    c = _Call()
    xd, ms, out = c.inp(data), c.out((2,)), c.out((count,))
    nde.use_torch_stream()
    _lib.check(nde._L.colnde_zscore_stats_dev(nde._h, xd.data_ptr(), count, ms.data_ptr()))
    _lib.check(nde._L.colnde_scale_dev(nde._h, xd.data_ptr(), count, ms.data_ptr(), out.data_ptr()))
    c.check()
    ms = ms.cpu().numpy()
    assert np.isclose(ms[0], mu, rtol=1e-6) and np.isclose(ms[1], sigma, rtol=1e-6)                              # test_data_prep's tolerances
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("Nz,n", [(32, 9), (64, 5)])
def test_ensemble_column_loss_leaves_the_tail(Nz, n):
    import colnde
    from colnde import _lib
    cfg, x0, bcs, truth = _fc_ensemble_problem(Nz, n)
    K = 3
    assert (K * n * 5) % (256 // Nz) != 0                                     # the last block of 256 / Nz rows is ragged
    sol = (truth[None] + 0.1 * np.random.default_rng(66 + Nz).standard_normal((K,) + truth.shape)).astype(np.float32)
    with colnde.FreeConvectionEnsemble(cfg, n, K) as e:
        e.set_problem(x0, bcs, truth)
        c = _Call()
        sd, out = c.inp(sol), c.out((K, n, 5))
        e.use_torch_stream()
        _lib.check(e._L.colnde_ensemble_column_loss_dev(e._h, sd.data_ptr(), out.data_ptr()))
        c.check()
        got = out.cpu().numpy()
    ref = ((sol.astype(np.float64) - truth.astype(np.float64)[None]) ** 2).mean(axis=3)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0.0)                 # test_gpu_fc_ensemble.test_column_loss's tolerance
