"""What nde.py and embed.py share about arrays: numpy conversion, pointers, the torch-or-numpy question, and the ensemble shape check."""
import ctypes

import numpy as np


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(a.shape)))
    return a


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _span(a):
    """(address, bytes) of a numpy array or a torch tensor."""
    if _is_torch(a):
        return a.data_ptr(), a.numel() * a.element_size()
    return a.ctypes.data, a.nbytes


def _dtype_name(a) -> str:
    return str(a.dtype).replace("torch.", "")


def check_ensemble_arrays(n_models: int, n_params: int, weights=None, physics=None, etas=None):
    """Shape checks of an ensemble's per-model arrays (no GPU needed): weights [K, n_params], physics [K, 5] (PHYSICS_KEYS), etas [K]."""
    K = int(n_models)
    if K < 1:
        raise ValueError("n_models must be >= 1, got %d" % K)
    for name, a, shape in (("weights", weights, (K, n_params)), ("physics", physics, (K, 5)), ("etas", etas, (K,))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError("%s: expected shape %s for %d models, got %s" % (name, shape, K, tuple(a.shape)))
