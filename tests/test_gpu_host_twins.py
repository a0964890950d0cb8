"""The host-array entry points that stage their arrays through one device scratch per call (csrc/api_internal.h: HostStage) against their `_dev`
forms: the same bits as the device call on torch tensors holding the same inputs, and the scratch given back after every call.

One table over the eight staged twins — flux, loss_per_tstep, implicit_diffusion, wm_infer_dz_flux / wm_embedded_step, wm_diagnose_flux /
wm_embedded_step_flux, ensemble_wm_embedded (K = 2), mpp_diagnose_flux, fc_embedded_step / fc_diagnose_wT — at n = 1 column (the least every kernel
takes) and n = 33 (one past a 32-column tile; 33 x 33 face values and 3 x 33 halo values are no multiple of four floats, so the blocks behind them
start on a 16-byte boundary only because the scratch puts them there), with the optional halos absent and with all of them present.  Shapes and inputs
are those of the embedding tests: Nz = 32 wind-mixing 96-50-20-31 (tests/test_gpu_wm_diag.py, tests/test_gpu_wm_ens_embed.py) and Nz = 32 fc32
(tests/test_gpu_fc_embed.py)."""
import numpy as np
import pytest

from tests import wm_embed_common as W
from tests.test_gpu_fc_embed import DT as FC_DT, LZ as FC_LZ, _case as fc_case
from tests.test_gpu_wm_diag import DT, _case as wm_case
from tests.test_gpu_wm_ens_embed import ens_case

pytestmark = pytest.mark.gpu

SIZES = (1, 33)
K_ENS = 2
FC_K = 10.0
REPEATS = 20


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()               # (a copy: the shared inputs are read-only)


def _host(a):
    return a


def _flat(r):
    """every array of a (nested) result, as NumPy"""
    if r is None:
        return []
    if isinstance(r, (tuple, list)):
        return [a for part in r for a in _flat(part)]
    return [r if isinstance(r, np.ndarray) else r.cpu().numpy()]


# ---- the table: name -> (handle(n), [call(nde, n, halo, X), ...]); X puts an input array where the call under test takes it from ---------------
def _wm_handle(n):
    import colnde
    return colnde.ColumnNDE(wm_case(n)[0].cfg, 4)                                    # (the handle's own column count is unrelated to n)


def _problem_handle(n):
    """a handle of n columns with a problem and truth trajectories set (loss_per_tstep works on the handle's own columns)"""
    import colnde
    p = wm_case(n)[0]
    x0, bcs = np.ascontiguousarray(p.x0[:n]), np.ascontiguousarray(p.bcs[:n])
    nde = colnde.ColumnNDE(p.cfg, n)
    nde.set_problem(x0, bcs)
    nde.set_problem(x0, bcs, nde.forward(p.weights_truth))
    return nde


def _flux(nde, n, halo, X):
    p = wm_case(n)[0]
    return nde.flux(X(p.x0[:n]), X(p.weights), X(p.bcs[:n]), 0.02)


def _loss_per_tstep(nde, n, halo, X):
    return nde.loss_per_tstep(X(wm_case(n)[0].weights))


def _implicit_diffusion(nde, n, halo, X):
    _, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.implicit_diffusion(X(u), X(v), X(T), DT, W.LZ / 32, W.mpp_params(), True, X(hb) if halo else None)


def _wm_infer_dz_flux(nde, n, halo, X):
    p, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.wm_infer_dz_flux(X(p.weights_truth), X(u), X(v), X(T), X(top), W.LZ)


def _wm_embedded_step(nde, n, halo, X):
    p, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.wm_embedded_step(X(p.weights_truth), X(u), X(v), X(T), X(top), W.LZ, DT, W.mpp_params(), True, X(hb) if halo else None)


def _wm_diagnose_flux(nde, n, halo, X):
    p, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.wm_diagnose_flux(X(p.weights_truth), X(u), X(v), X(T), X(top), W.LZ, W.mpp_params(), True, (X(hb), X(ht)) if halo else None)


def _wm_embedded_step_flux(nde, n, halo, X):
    p, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.wm_embedded_step_flux(X(p.weights_truth), X(u), X(v), X(T), X(top), W.LZ, DT, W.mpp_params(), True, (X(hb), X(ht)) if halo else None)


def _ens_handle(n):
    import colnde
    return colnde.ColumnNDEEnsemble(ens_case(K_ENS, n)[0].cfg, 8, K_ENS)


def _ens_call(step, flux):
    def call(ens, n, halo, X):
        _, w, u, v, T, top, hb, ht, params = ens_case(K_ENS, n)
        return ens.wm_embedded(X(w), X(u), X(v), X(T), X(top), W.LZ, DT if step else None, params, True, X(hb) if halo else None, X(ht) if halo else None,
                               step=step, flux=flux)
    return call


def _mpp_diagnose_flux(nde, n, halo, X):
    _, (u, v, T, top, hb, ht) = wm_case(n)
    return nde.mpp_diagnose_flux(X(u), X(v), X(T), X(top), W.LZ / 32, W.mpp_params(), True, X(hb) if halo else None)


def _fc_handle(n):
    import colnde
    return colnde.ColumnNDE(fc_case(32, n)[0], 4)


def _fc_call(step, diag):
    def call(nde, n, halo, X):
        _, w, (T, top, hb, ht) = fc_case(32, n)
        halos = (X(hb), X(ht)) if halo else None
        if step:
            return nde.fc_embedded_step(X(w), X(T), X(top), FC_LZ, FC_DT, FC_K, halos, diagnose=diag)
        return nde.fc_diagnose_wT(X(w), X(T), X(top), FC_LZ, FC_K, halos)
    return call


# (takes halos, handle, calls)
TWINS = {
    "flux": (False, _wm_handle, [_flux]),
    "loss_per_tstep": (False, _problem_handle, [_loss_per_tstep]),
    "implicit_diffusion": (True, _wm_handle, [_implicit_diffusion]),
    "wm_infer_dz_flux/wm_embedded_step": (True, _wm_handle, [_wm_infer_dz_flux, _wm_embedded_step]),
    "wm_diagnose_flux/wm_embedded_step_flux": (True, _wm_handle, [_wm_diagnose_flux, _wm_embedded_step_flux]),
    "ensemble_wm_embedded": (True, _ens_handle, [_ens_call(s, f) for s in (True, False) for f in (True, False)]),
    "mpp_diagnose_flux": (True, _wm_handle, [_mpp_diagnose_flux]),
    "fc_embedded_step/fc_diagnose_wT": (True, _fc_handle, [_fc_call(True, False), _fc_call(True, True), _fc_call(False, True)]),
}
CASES = [(name, n, halo) for name, (halos, _, _) in TWINS.items() for n in SIZES for halo in ((False, True) if halos else (False,))]


@pytest.mark.parametrize("name,n,halo", CASES)
def test_host_arrays_give_the_bits_of_the_device_call(name, n, halo):
    import torch
    _, handle, calls = TWINS[name]
    with handle(n) as nde:
        for call in calls:
            host = _flat(call(nde, n, halo, _host))
            dev = call(nde, n, halo, _dev)
            torch.cuda.synchronize()
            dev = _flat(dev)
            assert len(host) == len(dev) and len(host) >= 1
            for i, (a, b) in enumerate(zip(host, dev)):
                assert a.shape == b.shape and a.size >= n and np.isfinite(a).all(), (name, call.__name__, i, a.shape)
                assert np.array_equal(a, b), (name, call.__name__, i, float(np.abs(a - b).max()))


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("name", sorted(TWINS))
def test_repeated_host_calls_give_their_scratch_back(name):
    """tests/test_gpu_lifecycle.py's check for handles, for the per-call scratch: the free device memory after 20 host-array calls is the figure
    before them (the first call of each kind is made beforehand: the handle's own buffers, the runtime's code objects)."""
    halos, handle, calls = TWINS[name]
    with handle(33) as nde:
        for call in calls:
            for halo in ((False, True) if halos else (False,)):
                call(nde, 33, halo, _host)
                before = _free_bytes()
                for _ in range(REPEATS):
                    call(nde, 33, halo, _host)
                after = _free_bytes()
                assert after == before, (name, call.__name__, halo, before - after)
