"""The embedding half of `ColumnNDE`: what an ocean model calls every iteration with a trained network — inference, the steps either side of it,
the wind-mixing and free-convection embedded steps and the saved-state flux diagnoses (csrc/api_embed.hip).

The validators and the result tuples are module-level (no GPU needed); the methods are the mix-in `EmbeddingMixin`, which `nde.ColumnNDE` inherits.
Each method checks its torch tensors or converts its numpy arrays in a branch of its own, then writes the ABI argument list once: `_marshal` gives
the pointer function, the allocator and the symbol (`name + "_dev"` for tensors) of the kind at hand.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._arrays import _dtype_name, _f32, _is_torch, _ptr, _span, check_ensemble_arrays


def _overlap(a, b):
    (pa, na), (pb, nb) = _span(a), _span(b)
    return pa < pb + nb and pb < pa + na


def _check_shape(name, a, shape):
    if tuple(a.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(a.shape)))


def _marshal(nde, like):
    """How arrays of `like`'s kind reach the ABI: (P, empty, sym).  P(a) is the pointer argument of a (None: NULL), empty(a, shape=None) an
    uninitialised array like a (of another shape), sym(name) the entry point: name + "_dev" for device tensors, name for host arrays."""
    if _is_torch(like):
        import torch
        return ((lambda a: a.data_ptr() if a is not None else None),
                (lambda a, shape=None: torch.empty_like(a) if shape is None else torch.empty(shape, dtype=a.dtype, device=a.device)),
                (lambda name: getattr(nde._L, name + "_dev")))
    return _ptr, (lambda a, shape=None: np.empty_like(a) if shape is None else np.empty(shape, np.float32)), (lambda name: getattr(nde._L, name))


def _opt_f32(a):
    return _f32(a) if a is not None else None


def check_wm_embed_arrays(Nz: int, n: int, state, top_flux, halo_bottom=None, dz_out=None, out=None):
    """Shape and alias rules of `wm_infer_dz_flux` / `wm_embedded_step` (no GPU needed): state = (u, v, T) each [n, Nz], top_flux [3, n],
    halo_bottom [3, n] or None, dz_out = three [n, Nz] arrays that overlap NOTHING, out = three [n, Nz] arrays each of which may be
    exactly its own input (in place) and overlaps nothing else."""
    names = ("u", "v", "T")
    if len(state) != 3:
        raise ValueError("state must be (u, v, T)")
    for nm, a in zip(names, state):
        _check_shape(nm, a, (n, Nz))
    if tuple(top_flux.shape) != (3, n):
        raise ValueError("top_flux: expected shape %s (uw, vw, wT at the top face), got %s" % ((3, n), tuple(top_flux.shape)))
    if halo_bottom is not None:
        _check_shape("halo_bottom", halo_bottom, (3, n))
    inputs = [(nm, a) for nm, a in zip(names, state)] + [("top_flux", top_flux)] + ([("halo_bottom", halo_bottom)] if halo_bottom is not None else [])
    outputs = []
    for label, arrs, tags in (("dz_out", dz_out, ("dz_uw", "dz_vw", "dz_wT")), ("out", out, ("u_out", "v_out", "T_out"))):
        if arrs is None:
            continue
        if len(arrs) != 3:
            raise ValueError("%s must be three arrays" % label)
        for tg, a in zip(tags, arrs):
            _check_shape(tg, a, (n, Nz))
            outputs.append((tg, a))
    own = {"u_out": "u", "v_out": "v", "T_out": "T"}
    for i, (to, o) in enumerate(outputs):
        for ti, a in inputs:
            if _overlap(o, a) and not (own.get(to) == ti and _span(o) == _span(a)):
                raise ValueError("%s overlaps %s: the dz arrays may alias nothing, an output only its own input (in place)" % (to, ti))
        for tj, b in outputs[i + 1:]:
            if _overlap(o, b):
                raise ValueError("%s overlaps %s" % (to, tj))


def check_wm_diag_arrays(Nz: int, n: int, state, top_flux, halos=None, faces_out=None, dz_out=None, out=None):
    """Shape and alias rules of `wm_diagnose_flux` / `wm_embedded_step_flux` / `mpp_diagnose_flux` (no GPU needed): those of
    `check_wm_embed_arrays` for state, top_flux, dz_out and out; halos = None or (halo_bottom, halo_top), each [3, n] or None; faces_out =
    three [n, Nz + 1] arrays (uw, vw, wT) that overlap nothing."""
    if halos is not None and len(halos) != 2:
        raise ValueError("halos must be (halo_bottom, halo_top); either may be None")
    hb, ht = halos if halos is not None else (None, None)
    check_wm_embed_arrays(Nz, n, state, top_flux, hb, dz_out, out)
    if ht is not None:
        _check_shape("halo_top", ht, (3, n))
    if faces_out is None:
        return
    if len(faces_out) != 3:
        raise ValueError("faces_out must be three arrays (uw, vw, wT)")
    tags = ("uw", "vw", "wT")
    for tg, a in zip(tags, faces_out):
        _check_shape(tg, a, (n, Nz + 1))
    others = list(zip(("u", "v", "T"), state)) + [("top_flux", top_flux)] + [(nm, a) for nm, a in (("halo_bottom", hb), ("halo_top", ht)) if a is not None]
    others += list(zip(("dz_uw", "dz_vw", "dz_wT"), dz_out or ())) + list(zip(("u_out", "v_out", "T_out"), out or ()))
    for i, (tg, a) in enumerate(zip(tags, faces_out)):
        for nm, b in others + list(zip(tags[i + 1:], faces_out[i + 1:])):
            if _overlap(a, b):
                raise ValueError("%s overlaps %s: the face arrays may alias nothing" % (tg, nm))


def check_fc_embed_arrays(Nz: int, n: int, T, top_flux, halos=None, dz_out=None, T_out=None, faces_out=None):
    """Shape and alias rules of `fc_embedded_step` / `fc_diagnose_wT` (no GPU needed): T [n, Nz], top_flux [n], halos = None or
    (halo_bottom, halo_top), each [n] or None; dz_out [n, Nz] and faces_out [n, Nz + 1] overlap nothing, T_out [n, Nz] may be exactly T
    (in place) and overlaps nothing else."""
    _check_shape("T", T, (n, Nz))
    _check_shape("top_flux", top_flux, (n,))
    if halos is not None and len(halos) != 2:
        raise ValueError("halos must be (halo_bottom, halo_top); either may be None")
    inputs = [("T", T), ("top_flux", top_flux)]
    for nm, a in zip(("halo_bottom", "halo_top"), halos if halos is not None else ()):
        if a is not None:
            _check_shape(nm, a, (n,))
            inputs.append((nm, a))
    outputs = []
    for nm, a, shape in (("dz_out", dz_out, (n, Nz)), ("T_out", T_out, (n, Nz)), ("faces_out", faces_out, (n, Nz + 1))):
        if a is not None:
            _check_shape(nm, a, shape)
            outputs.append((nm, a))
    for i, (to, o) in enumerate(outputs):
        for ti, a in inputs:
            if _overlap(o, a) and not (to == "T_out" and ti == "T" and _span(o) == _span(a)):
                raise ValueError("%s overlaps %s: only T_out may alias an input, and only T itself (in place)" % (to, ti))
        for tj, b in outputs[i + 1:]:
            if _overlap(o, b):
                raise ValueError("%s overlaps %s" % (to, tj))


class FcEnsembleEmbedded(NamedTuple):
    """What `fc_embedded` returns: dz_wT (∂z_wT_NN of T as given) and T_new (T′), each [K, n, Nz], or None (step=False); faces (wT_NN − κ ∂T/∂z of the
    state as given) [K, n, Nz + 1], or None (faces=False)."""
    dz_wT: Optional[object]
    T_new: Optional[object]
    faces: Optional[object]


def check_fc_ens_embed_arrays(n_models: int, n_params: int, Nz: int, weights, T, top_flux, dt=None, halos=None, step: bool = True, faces: bool = True,
                              dz_out=None, T_out=None):
    """Shape, dtype and group rules of `fc_embedded` (no GPU needed), raised before any library call: weights [K, n_params] (n_params the HANDLE's
    count — `fc_ensemble_n_params(cfg, conv)`: a conv ensemble does not take vectors of the plain length) or None; T [K, n, Nz] with n >= 1;
    top_flux [n], shared by the members; halos = None or (halo_bottom, halo_top), each [K, n] or None; every array float32; at least one of step
    and faces; step=True needs dt > 0; dz_out and T_out [K, n, Nz] (caller-owned outputs of the step) are one group: both or neither.  Returns n."""
    K = int(n_models)
    if K < 1:
        raise ValueError("n_models must be >= 1, got %d" % K)
    if weights is not None and tuple(weights.shape) != (K, int(n_params)):
        raise ValueError("weights: expected shape %s for %d models (n_params is the handle's count: a conv member's vector leads with its filter), got %s"
                         % ((K, int(n_params)), K, tuple(weights.shape)))
    if len(tuple(T.shape)) != 3 or int(T.shape[0]) != K or int(T.shape[2]) != Nz or int(T.shape[1]) < 1:
        raise ValueError("T: expected shape (%d, n, %d) for %d models with n >= 1, got %s" % (K, Nz, K, tuple(T.shape)))
    n = int(T.shape[1])
    if tuple(top_flux.shape) != (n,):
        raise ValueError("top_flux: expected shape %s (shared by the members), got %s" % ((n,), tuple(top_flux.shape)))
    if halos is not None and len(halos) != 2:
        raise ValueError("halos must be (halo_bottom, halo_top); either may be None")
    named = [("weights", weights), ("T", T), ("top_flux", top_flux)]
    for nm, a in zip(("halo_bottom", "halo_top"), halos if halos is not None else ()):
        if a is not None:
            _check_shape(nm, a, (K, n))
        named.append((nm, a))
    for nm, a in named:
        if a is not None and _dtype_name(a) != "float32":
            raise ValueError("%s: expected float32, got %s" % (nm, _dtype_name(a)))
    if (dz_out is None) != (T_out is None):
        raise ValueError("dz_out and T_out are one output group (the step): give both or neither, got only %s" % ("dz_out" if T_out is None else "T_out"))
    if dz_out is not None and not step:
        raise ValueError("dz_out / T_out are the step's outputs: step=False writes none")
    for nm, a in (("dz_out", dz_out), ("T_out", T_out)):
        if a is not None:
            _check_shape(nm, a, (K, n, Nz))
    if not step and not faces:
        raise ValueError("nothing to compute: step (dz_wT, T′) and faces are the two output groups — ask for at least one")
    if step and (dt is None or not float(dt) > 0.0):
        raise ValueError("step=True takes the adjustment step and needs dt > 0, got dt = %r (step=False: the faces of the state as given)" % (dt,))
    return n


class WmEnsembleEmbedded(NamedTuple):
    """What `ColumnNDEEnsemble.wm_embedded` returns: dz = (∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), each [K, n, Nz]; state = (u′, v′, T′), each [K, n, Nz], or
    None (step=False); faces = (uw, vw, wT), each [K, n, Nz + 1], or None (flux=False)."""
    dz: tuple
    state: Optional[tuple]
    faces: Optional[tuple]


def check_wm_ens_embed_arrays(n_models: int, n_params: int, Nz: int, weights, state, top_flux, dt=None, params=None, halo_bottom=None, halo_top=None,
                              step: bool = True):
    """Shape and argument rules of `ColumnNDEEnsemble.wm_embedded` (no GPU needed), raised before any library call: weights [K, n_params]; state =
    (u, v, T), each [K, n, Nz]; top_flux [3, n], shared by the models; halo_bottom, halo_top [K, 3, n] or None; params [K, 7] or None; step=True
    needs dt > 0.  Per model the rules are those of `check_wm_diag_arrays`.  Returns n."""
    K = int(n_models)
    check_ensemble_arrays(K, n_params, weights=weights)
    if len(state) != 3:
        raise ValueError("state must be (u, v, T)")
    T = state[2]
    if len(T.shape) != 3 or T.shape[0] != K:
        raise ValueError("T: expected shape (%d, n, %d) for %d models, got %s" % (K, Nz, K, tuple(T.shape)))
    n = int(T.shape[1])
    for nm, a in zip(("u", "v", "T"), state):
        if tuple(a.shape) != (K, n, Nz):
            raise ValueError("%s: expected shape %s for %d models, got %s" % (nm, (K, n, Nz), K, tuple(a.shape)))
    for nm, a in (("halo_bottom", halo_bottom), ("halo_top", halo_top)):
        if a is not None and tuple(a.shape) != (K, 3, n):
            raise ValueError("%s: expected shape %s for %d models, got %s" % (nm, (K, 3, n), K, tuple(a.shape)))
    for k in range(K):
        check_wm_diag_arrays(Nz, n, tuple(a[k] for a in state), top_flux,
                             (None if halo_bottom is None else halo_bottom[k], None if halo_top is None else halo_top[k]))
    if params is not None and tuple(np.shape(params)) != (K, 7):
        raise ValueError("params: expected shape %s (nu0, nu_minus, dRi, Ric, Pr, alpha, g per model), got %s" % ((K, 7), tuple(np.shape(params))))
    if step and (dt is None or not float(dt) > 0.0):
        raise ValueError("step=True takes the implicit step and needs dt > 0, got dt = %r (step=False: the ∂z arrays and the faces of the state as given)" % (dt,))
    return n


class EmbeddingMixin:
    """The embedding methods of `ColumnNDE` (which provides cfg, n_params, _h, _L, _chk_dev and use_torch_stream)."""

    def _chk_devs(self, tensors, shape):
        for t in tensors:
            if t is not None:
                self._chk_dev(t, shape)

    # ---- embedded inference ---------------------------------------------------------------------------
    def infer_dz_wT(self, weights, T, top_flux, Lz: float):
        """+∂z wT, what `compute_neural_network_forcing!` stores in `params.∂z_wT_NN` (double_gyre_nn.jl:165); `infer_forcing` is its negative (:135)."""
        return self.infer_forcing(weights, T, top_flux, Lz, _dz_wT=True)

    def infer_forcing(self, weights, T, top_flux, Lz: float, _dz_wT: bool = False):
        Nz = self.cfg.Nz
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            self._chk_dev(T, (n, Nz))
            self._chk_dev(top_flux, (n,))
            self._chk_dev(weights, (self.n_params,))
            self.use_torch_stream()
        else:
            T = _f32(T)
            n = T.shape[0]
            T = _f32(T, (n, Nz))
            top_flux = _f32(top_flux, (n,))
            weights = _f32(weights, (self.n_params,))
        out = empty(T)
        fn = sym("colnde_infer_dz_wT" if _dz_wT else "colnde_infer_forcing")
        _lib.check(fn(self._h, P(weights), P(T), P(top_flux), float(Lz), P(out), n))
        return out

    # ---- the steps either side of the hot path --------------------------------------------
    def convective_adjustment(self, T, dt: float, dz: float, K: float, halo_bottom=None, halo_top=None, out=None):
        """`convective_adjustment!(model, Δt, K)` (free_convection/double_gyre_nn.jl:27-62) on [n][Nz] columns."""
        Nz = self.cfg.Nz
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            self._chk_dev(T, (n, Nz))
            self._chk_devs((halo_bottom, halo_top), (n,))
            if out is None:
                out = empty(T)
            self._chk_dev(out, (n, Nz))
            self.use_torch_stream()
        else:
            T = _f32(T)
            n = T.shape[0]
            T = _f32(T, (n, Nz))
            halo_bottom = _f32(halo_bottom, (n,)) if halo_bottom is not None else None
            halo_top = _f32(halo_top, (n,)) if halo_top is not None else None
            out = empty(T)
        _lib.check(sym("colnde_convective_adjustment")(self._h, P(T), P(halo_bottom), P(halo_top), float(dt), float(dz), float(K), P(out), n))
        return out

    def implicit_diffusion(self, u, v, T, dt: float, dz: float, params, convective_adjustment: bool = False, halo_bottom=None, out=None):
        """`modified_pacanowski_philander!(model, constants, Δt, p, convective_adjustment)` (wind_mixing/src/NDE_oceananigans.jl:61-101)
        on [n][Nz] columns of u, v, T.  params = (ν₀, ν₋, ΔRi, Riᶜ, Pr, α, g); halo_bottom [3][n] or None.  Returns (u′, v′, T′);
        `out` = a triple of device tensors (each may be its own input: in place)."""
        Nz = self.cfg.Nz
        pr = (ctypes.c_float * 7)(*[float(x) for x in params])
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            self._chk_devs((u, v, T), (n, Nz))
            self._chk_devs((halo_bottom,), (3, n))
            if out is None:
                out = tuple(empty(T) for _ in range(3))
            for a in out:
                self._chk_dev(a, (n, Nz))
            self.use_torch_stream()
        else:
            T = _f32(T)
            n = T.shape[0]
            u, v, T = _f32(u, (n, Nz)), _f32(v, (n, Nz)), _f32(T, (n, Nz))
            halo_bottom = _f32(halo_bottom, (3, n)) if halo_bottom is not None else None
            out = tuple(empty(T) for _ in range(3))
        _lib.check(sym("colnde_implicit_diffusion")(self._h, P(u), P(v), P(T), P(halo_bottom), float(dt), float(dz), pr, int(bool(convective_adjustment)),
                                                    *map(P, out), n))
        return out

    # ---- wind-mixing embedding ------------------------------------------------------------------------
    def wm_infer_dz_flux(self, weights, u, v, T, top_flux, Lz: float, dz_out=None):
        """`NN_uw_forcing`, `NN_vw_forcing`, `NN_wT_forcing` (wind_mixing/src/NDE_oceananigans.jl:288-329) as `progress_neural_network`
        stores them (:393-400): (∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), each [n][Nz] = +∂z(flux); the forcing is its negative.  u, v, T [n][Nz]
        in the ocean model's units (k = 0 deepest), top_flux [3][n] = uw, vw, wT at the top face.  numpy arrays or device tensors
        (`dz_out`: three device tensors that alias nothing)."""
        return self._wm_embed(weights, u, v, T, top_flux, Lz, dz_out, None)

    def wm_embedded_step(self, weights, u, v, T, top_flux, Lz: float, dt: float, params, convective_adjustment: bool = False, halo_bottom=None,
                         dz_out=None, out=None):
        """`progress_neural_network` (wind_mixing/src/NDE_oceananigans.jl:380-405) in one launch: the three ∂z arrays of the state AS
        GIVEN, then `modified_pacanowski_philander!` on that state (Δz = Lz/Nz; params, halo_bottom as `implicit_diffusion`).
        Returns ((∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), (u′, v′, T′)); `out` tensors may be their own inputs (in place)."""
        return self._wm_embed(weights, u, v, T, top_flux, Lz, dz_out, (float(dt), params, bool(convective_adjustment), halo_bottom, out))

    def _wm_embed(self, weights, u, v, T, top_flux, Lz, dz_out, step):
        Nz = self.cfg.Nz
        dt, params, ca, halo_bottom, out = step if step is not None else (0.0, None, False, None, None)
        pr = (ctypes.c_float * 7)(*[float(x) for x in params]) if step is not None else None
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            check_wm_embed_arrays(Nz, n, (u, v, T), top_flux, halo_bottom, dz_out, out)
            self._chk_devs((u, v, T), (n, Nz))
            self._chk_dev(top_flux, (3, n))
            self._chk_dev(weights, (self.n_params,))
            self._chk_devs((halo_bottom,), (3, n))
            dz_out = tuple(dz_out) if dz_out is not None else tuple(empty(T) for _ in range(3))
            if step is not None:
                out = tuple(out) if out is not None else tuple(empty(T) for _ in range(3))
            self._chk_devs(dz_out + (out if step is not None else ()), (n, Nz))
            self.use_torch_stream()
        else:
            if dz_out is not None or out is not None:
                raise ValueError("dz_out / out are for device tensors; host arrays are returned")
            T = _f32(T)
            n = T.shape[0]
            u, v, T = _f32(u), _f32(v), _f32(T)
            top_flux = _f32(top_flux)
            halo_bottom = _opt_f32(halo_bottom)
            check_wm_embed_arrays(Nz, n, (u, v, T), top_flux, halo_bottom)
            weights = _f32(weights, (self.n_params,))
            dz_out = tuple(empty(T) for _ in range(3))
            out = tuple(empty(T) for _ in range(3)) if step is not None else None
        if step is None:
            _lib.check(sym("colnde_wm_infer_dz_flux")(self._h, P(weights), P(u), P(v), P(T), P(top_flux), float(Lz), *map(P, dz_out), n))
            return dz_out
        _lib.check(sym("colnde_wm_embedded_step")(self._h, P(weights), P(u), P(v), P(T), P(top_flux), P(halo_bottom), float(Lz), dt, pr, int(ca),
                                                  *map(P, dz_out), *map(P, out), n))
        return dz_out, out

    def wm_diagnose_flux(self, weights, u, v, T, top_flux, Lz: float, params, convective_adjustment: bool = False, halos=None, faces_out=None):
        """`diagnose_NN_flux_uw`, `_vw`, `_wT` (wind_mixing/src/NDE_oceananigans.jl:226-286): the total fluxes (uw, vw, wT), each [n][Nz+1]
        (face 0 the bottom), of the state as given: [0; inv(scaling).(NN) .- inv(scaling)(0); top] − ν ∂z φ with the diffusivities of
        `implicit_diffusion` (params, convective_adjustment as there; Δz = Lz/Nz).  halos = None or (halo_bottom, halo_top), each [3][n] or
        None (zero-gradient fill).  numpy arrays or device tensors (`faces_out`: three device tensors that alias nothing)."""
        return self._wm_diag(weights, u, v, T, top_flux, Lz, None, params, convective_adjustment, halos, faces_out, None, None)

    def wm_embedded_step_flux(self, weights, u, v, T, top_flux, Lz: float, dt: float, params, convective_adjustment: bool = False, halos=None,
                              dz_out=None, out=None, faces_out=None):
        """`wm_embedded_step` and `wm_diagnose_flux` of the same state as given in one call (one read of the state): returns
        ((∂z_uw_NN, ∂z_vw_NN, ∂z_wT_NN), (u′, v′, T′), (uw, vw, wT)).  The step reads halos[0] only; `out` tensors may be their own inputs."""
        return self._wm_diag(weights, u, v, T, top_flux, Lz, float(dt), params, convective_adjustment, halos, faces_out, dz_out, out)

    def _wm_diag(self, weights, u, v, T, top_flux, Lz, dt, params, ca, halos, faces_out, dz_out, out):
        Nz = self.cfg.Nz
        step = dt is not None
        pr = (ctypes.c_float * 7)(*[float(x) for x in params])
        if halos is not None and len(halos) != 2:
            raise ValueError("halos must be (halo_bottom, halo_top); either may be None")
        hb, ht = halos if halos is not None else (None, None)
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            check_wm_diag_arrays(Nz, n, (u, v, T), top_flux, halos, faces_out, dz_out, out)
            self._chk_devs((u, v, T), (n, Nz))
            self._chk_dev(top_flux, (3, n))
            self._chk_dev(weights, (self.n_params,))
            self._chk_devs((hb, ht), (3, n))
            faces_out = tuple(faces_out) if faces_out is not None else tuple(empty(T, (n, Nz + 1)) for _ in range(3))
            if step:
                dz_out = tuple(dz_out) if dz_out is not None else tuple(empty(T) for _ in range(3))
                out = tuple(out) if out is not None else tuple(empty(T) for _ in range(3))
            self._chk_devs(faces_out, (n, Nz + 1))
            self._chk_devs((dz_out + out) if step else (), (n, Nz))
            self.use_torch_stream()
        else:
            if dz_out is not None or out is not None or faces_out is not None:
                raise ValueError("dz_out / out / faces_out are for device tensors; host arrays are returned")
            T = _f32(T)
            n = T.shape[0]
            u, v, T, top_flux = _f32(u), _f32(v), _f32(T), _f32(top_flux)
            hb, ht = _opt_f32(hb), _opt_f32(ht)
            check_wm_diag_arrays(Nz, n, (u, v, T), top_flux, None if halos is None else (hb, ht))
            weights = _f32(weights, (self.n_params,))
            faces_out = tuple(empty(T, (n, Nz + 1)) for _ in range(3))
            if step:
                dz_out, out = tuple(empty(T) for _ in range(3)), tuple(empty(T) for _ in range(3))
        if not step:
            _lib.check(sym("colnde_wm_diagnose_flux")(self._h, P(weights), P(u), P(v), P(T), P(top_flux), P(hb), P(ht), float(Lz), pr, int(bool(ca)),
                                                      *map(P, faces_out), n))
            return faces_out
        _lib.check(sym("colnde_wm_embedded_step_flux")(self._h, P(weights), P(u), P(v), P(T), P(top_flux), P(hb), P(ht), float(Lz), dt, pr, int(bool(ca)),
                                                       *map(P, dz_out), *map(P, out), *map(P, faces_out), n))
        return dz_out, out, faces_out

    def wm_embedded(self, weights, u, v, T, top_flux, Lz: float, dt=None, params=None, convective_adjustment: bool = False, halo_bottom=None,
                    halo_top=None, step: bool = True, flux: bool = True) -> "WmEnsembleEmbedded":
        """One embedded iteration of ALL K models in one launch (`colnde_ensemble_wm_embedded`): per model what `wm_embedded_step_flux` (step and
        flux), `wm_embedded_step` (step), `wm_diagnose_flux` and `wm_infer_dz_flux` (flux; the ∂z arrays are always returned) give for that model's
        weights, state and constants, bit for bit — on a `ColumnNDEEnsemble`, and on a single `ColumnNDE` as K = 1: the one embedding call that
        deploys three networks of ANY layer sizes 96-…-31 and activations (Nz = 32; `describe()`: wm_embed=generic_f32), where the four
        single-model calls above cover 96-50-20-31 alone.  weights [K, n_params]; u, v, T [K, n, Nz], each model its own state; top_flux [3, n],
        shared; halo_bottom, halo_top [K, 3, n] or None; params [K, 7] = (nu0, nu_minus, dRi, Ric, Pr, alpha, g) per model, or None: the handle's
        physics with cfg.alpha, cfg.g.  numpy arrays or torch device tensors (all of one kind)."""
        Nz, K = self.cfg.Nz, int(getattr(self, "n_models", 1))
        n = check_wm_ens_embed_arrays(K, self.n_params, Nz, weights, (u, v, T), top_flux, dt, params, halo_bottom, halo_top, step)
        pr = None if params is None else (ctypes.c_float * (7 * K))(*[float(x) for x in np.asarray(params, dtype=np.float64).reshape(-1)])
        dtv = float(dt) if step else 0.0
        ca = int(bool(convective_adjustment))
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            self._chk_dev(weights, (K, self.n_params))
            self._chk_devs((u, v, T), (K, n, Nz))
            self._chk_dev(top_flux, (3, n))
            self._chk_devs((halo_bottom, halo_top), (K, 3, n))
            self.use_torch_stream()
        else:
            weights = _f32(weights, (K, self.n_params))
            u, v, T, top_flux = _f32(u), _f32(v), _f32(T), _f32(top_flux)
            halo_bottom, halo_top = _opt_f32(halo_bottom), _opt_f32(halo_top)
        dz = tuple(empty(T) for _ in range(3))
        st = tuple(empty(T) for _ in range(3)) if step else None
        fc = tuple(empty(T, (K, n, Nz + 1)) for _ in range(3)) if flux else None
        _lib.check(sym("colnde_ensemble_wm_embedded")(self._h, P(weights), P(u), P(v), P(T), P(top_flux), P(halo_bottom), P(halo_top), float(Lz), dtv, pr, ca,
                                                      *map(P, dz), *map(P, st or (None,) * 3), *map(P, fc or (None,) * 3), n))
        return WmEnsembleEmbedded(dz, st, fc)

    def mpp_diagnose_flux(self, u, v, T, top_flux, dz: float, params, convective_adjustment: bool = False, halo_bottom=None, faces_out=None):
        """`diagnose_baseline_flux_uw`, `_vw`, `_wT` (wind_mixing/src/NDE_oceananigans.jl:157-191): (uw, vw, wT), each [n][Nz+1], of the
        diffusivity-only model: −ν ∂z u, −ν ∂z v, −νT ∂z T with the top face replaced by top_flux [3][n].  params, halo_bottom as
        `implicit_diffusion`; no networks, any Nz.  numpy arrays or device tensors."""
        Nz = self.cfg.Nz
        pr = (ctypes.c_float * 7)(*[float(x) for x in params])
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            check_wm_diag_arrays(Nz, n, (u, v, T), top_flux, (halo_bottom, None), faces_out)
            self._chk_devs((u, v, T), (n, Nz))
            self._chk_dev(top_flux, (3, n))
            self._chk_devs((halo_bottom,), (3, n))
            faces_out = tuple(faces_out) if faces_out is not None else tuple(empty(T, (n, Nz + 1)) for _ in range(3))
            self._chk_devs(faces_out, (n, Nz + 1))
            self.use_torch_stream()
        else:
            if faces_out is not None:
                raise ValueError("faces_out is for device tensors; host arrays are returned")
            T = _f32(T)
            n = T.shape[0]
            u, v, T, top_flux = _f32(u), _f32(v), _f32(T), _f32(top_flux)
            halo_bottom = _opt_f32(halo_bottom)
            check_wm_diag_arrays(Nz, n, (u, v, T), top_flux, (halo_bottom, None))
            faces_out = tuple(empty(T, (n, Nz + 1)) for _ in range(3))
        _lib.check(sym("colnde_mpp_diagnose_flux")(self._h, P(u), P(v), P(T), P(top_flux), P(halo_bottom), float(dz), pr, int(bool(convective_adjustment)),
                                                   *map(P, faces_out), n))
        return faces_out

    # ---- free-convection embedding --------------------------------------------------------------------
    def fc_embedded_step(self, weights, T, top_flux, Lz: float, dt: float, K: float, halos=None, diagnose: bool = False, dz_out=None, T_out=None,
                         faces_out=None):
        """`progress_neural_network` of the free-convection embedding (free_convection/src/oceananigans_nn.jl:153-165) in one launch: the
        stored ∂z_wT_NN of T AS GIVEN, then `convective_adjustment!(model, Δt, K)` on it (Δz = Lz/Nz), and with `diagnose` (or `faces_out`)
        `diagnose_wT_NN` (:100-118) of the state as given.  T [n][Nz] in the units `infer_dz_wT` takes, top_flux [n], halos = None or
        (halo_bottom, halo_top).  numpy arrays or device tensors (`dz_out`, `T_out`, `faces_out`: device tensors; `T_out` may be `T`).
        Returns (∂z_wT_NN, T′) or (∂z_wT_NN, T′, wT_faces [n][Nz+1])."""
        return self._fc_embed(weights, T, top_flux, Lz, float(dt), K, halos, bool(diagnose) or faces_out is not None, dz_out, T_out, faces_out)

    def fc_diagnose_wT(self, weights, T, top_flux, Lz: float, K: float, halos=None, faces_out=None):
        """`diagnose_wT_NN` (free_convection/src/oceananigans_nn.jl:100-118): wT_NN − κ ∂T/∂z on the Nz + 1 faces, κ = K where the face
        gradient is negative; [n][Nz+1].  Arguments as `fc_embedded_step`."""
        return self._fc_embed(weights, T, top_flux, Lz, None, K, halos, True, None, None, faces_out)

    def _fc_embed(self, weights, T, top_flux, Lz, dt, K, halos, diag, dz_out, T_out, faces_out):
        Nz = self.cfg.Nz
        step = dt is not None
        hb, ht = halos if halos is not None else (None, None)
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            n = T.shape[0]
            check_fc_embed_arrays(Nz, n, T, top_flux, halos, dz_out, T_out, faces_out)
            self._chk_dev(T, (n, Nz))
            self._chk_dev(top_flux, (n,))
            self._chk_dev(weights, (self.n_params,))
            self._chk_devs((hb, ht), (n,))
            if step and dz_out is None:
                dz_out = empty(T)
            if step and T_out is None:
                T_out = empty(T)
            if diag and faces_out is None:
                faces_out = empty(T, (n, Nz + 1))
            self._chk_devs((dz_out, T_out), (n, Nz))
            self._chk_devs((faces_out,), (n, Nz + 1))
            self.use_torch_stream()
        else:
            if dz_out is not None or T_out is not None or faces_out is not None:
                raise ValueError("dz_out / T_out / faces_out are for device tensors; host arrays are returned")
            T = _f32(T)
            n = T.shape[0]
            top_flux = _f32(top_flux)
            hb, ht = _opt_f32(hb), _opt_f32(ht)
            check_fc_embed_arrays(Nz, n, T, top_flux, None if halos is None else (hb, ht))
            weights = _f32(weights, (self.n_params,))
            faces_out = empty(T, (n, Nz + 1)) if diag else None
            if step:
                dz_out, T_out = empty(T), empty(T)
        if not step:
            _lib.check(sym("colnde_fc_diagnose_wT")(self._h, P(weights), P(T), P(top_flux), P(hb), P(ht), float(Lz), float(K), P(faces_out), n))
            return faces_out
        _lib.check(sym("colnde_fc_embedded_step")(self._h, P(weights), P(T), P(top_flux), P(hb), P(ht), float(Lz), dt, float(K), P(dz_out), P(T_out),
                                                  P(faces_out), n))
        return (dz_out, T_out, faces_out) if diag else (dz_out, T_out)

    def fc_embedded(self, weights, T, top_flux, Lz: float, K: float, dt=None, halos=None, step: bool = True, faces: bool = True, dz_out=None,
                    T_out=None) -> "FcEnsembleEmbedded":
        """One embedded iteration of ALL members in one launch (`colnde_ensemble_fc_embedded`): per member what `fc_embedded_step` (step) and
        `fc_diagnose_wT` (faces) give for that member's weights and state — on a `FreeConvectionEnsemble`, plain or conv, and on a single
        `ColumnNDE` as K = 1, plain or `conv=c`: the one embedding call that runs a `--conv` network.  weights [K, n_params], or None: the
        operand images the previous call on this handle packed (an embedding calls with fixed weights); T [K, n, Nz], each member its own
        state; top_flux [n], shared; halos = None or (halo_bottom, halo_top), each [K, n] or None; step=True needs dt > 0.  numpy arrays or
        torch device tensors (all of one kind; `dz_out` and `T_out`, device tensors given together, receive the step — `T_out` may be `T`: in
        place).  Returns `FcEnsembleEmbedded(dz_wT, T_new, faces)`."""
        Nz, Km = self.cfg.Nz, int(getattr(self, "n_models", 1))
        n = check_fc_ens_embed_arrays(Km, self.n_params, Nz, weights, T, top_flux, dt, halos, step, faces, dz_out, T_out)
        hb, ht = halos if halos is not None else (None, None)
        dtv = float(dt) if step else 0.0
        P, empty, sym = _marshal(self, T)
        if _is_torch(T):
            self._chk_devs((weights,), (Km, self.n_params))
            self._chk_dev(T, (Km, n, Nz))
            self._chk_dev(top_flux, (n,))
            self._chk_devs((hb, ht), (Km, n))
            self._chk_devs((dz_out, T_out), (Km, n, Nz))
            self.use_torch_stream()
        else:
            if dz_out is not None or T_out is not None:
                raise ValueError("dz_out / T_out are for device tensors; host arrays are returned")
            weights = _f32(weights, (Km, self.n_params)) if weights is not None else None
            T, top_flux = _f32(T), _f32(top_flux)
            hb, ht = _opt_f32(hb), _opt_f32(ht)
        dz = (dz_out if dz_out is not None else empty(T)) if step else None
        Tn = (T_out if T_out is not None else empty(T)) if step else None
        fc = empty(T, (Km, n, Nz + 1)) if faces else None
        _lib.check(sym("colnde_ensemble_fc_embedded")(self._h, P(weights), P(T), P(top_flux), P(hb), P(ht), float(Lz), dtv, float(K), P(dz), P(Tn), P(fc), n))
        return FcEnsembleEmbedded(dz, Tn, fc)
