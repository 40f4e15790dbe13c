"""The host tables of the feature modules, one definition each: the stamp of an unchanged tensor, the bounded cache, an
index table as checked int32 and its pointer for the C ABI, the vertex -> (face, corner) CSR, buffers following the input."""
import ctypes

import numpy as np
import torch

from . import _lib

_CTYPES = {np.dtype(np.int32): ctypes.c_int32, np.dtype(np.float32): ctypes.c_float}      # host_ptr's dtypes


def stamp(*tensors):
    """``(id, _version, data_ptr)`` per tensor: equal for the same objects, unwritten and not re-pointed.  An ``id`` is the
    object's only while it lives: whoever stores a stamp stores the tensors next to it (``Cache.keep`` does)."""
    return tuple((id(t), t._version, t.data_ptr()) for t in tensors)


class Cache(dict):
    """key -> (held, value): a module's tables of constant inputs.  Once it holds more than 16 entries it is cleared before
    the next insert (a cleared table is built again on next use).  ``held`` are the objects the key was stamped from."""

    def find(self, key):
        return self.get(key, (None, None))[1]

    def keep(self, key, value, *held):
        if len(self) > 16:
            self.clear()
        self[key] = (held, value)
        return value


def host_i32(what, name, x, shape):
    """An index table as a contiguous int32 numpy array of ``shape`` (None: any length)."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.dtype.kind not in 'iu' and a.size:
        raise ValueError('%s: %s must hold integers (it is %s)' % (what, name, a.dtype))
    a = a.astype(np.int64)
    if a.ndim != len(shape) or any(s is not None and a.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError('%s: %s must be %s (it is %s)' % (
            what, name, '[' + ', '.join('n' if s is None else str(s) for s in shape) + ']', a.shape))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError('%s: %s does not fit int32' % (what, name))
    return np.ascontiguousarray(a, dtype=np.int32)


def host_ptr(a):
    """An int32 or float32 host array (any other dtype: KeyError) for the C ABI, NULL when it is empty; a parameter bound
    as ``c_void_p`` and one bound as ``POINTER(c_int32)`` both take it."""
    return a.ctypes.data_as(ctypes.POINTER(_CTYPES[a.dtype])) if a.size else None


def vertex_faces(faces, V):
    """The vertex -> (face, corner) CSR of the checked int32 ``faces`` [F, 3]: ``offsets [V + 1]`` and ``entries
    [max(3 F, 1)]`` (``3 * face + corner``, ascending per vertex), numpy int32.  The library refuses an index not in [0, V)."""
    F, offsets = faces.shape[0], np.zeros(V + 1, dtype=np.int32)
    entries = np.zeros(max(3 * F, 1), dtype=np.int32)
    _lib.MESH.check(_lib.load().exa_mesh_vertex_faces(V, F, host_ptr(faces), host_ptr(offsets), host_ptr(entries)))
    return offsets, entries


def face_tables(faces, V, device):
    """``(faces, offsets, entries)`` of ``vertex_faces`` as tensors on ``device``."""
    return tuple(torch.from_numpy(a).to(device) for a in (faces,) + vertex_faces(faces, V))


def follow(module, names, device):
    """The non-persistent buffers ``names`` of a module that was never moved follow its input to ``device``."""
    if getattr(module, names[0]).device != device:
        for name in names:
            setattr(module, name, getattr(module, name).to(device))
