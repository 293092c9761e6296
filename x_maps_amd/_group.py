"""What the group objects' Python classes share (esl_init.EslInit, mc3d.Mc3d, esl_optim.EslOptim, esl_filter.EslFilter; the C side:
csrc/host/xm_group.hpp): the owner of the native object, the pointer of an optional array, and the stacking of a caller's maps into
the one contiguous array a group call takes.  Nothing here loads the library by itself."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

T_DTYPES = {np.dtype(np.float32): N.XM_T_FLOAT32, np.dtype(np.float64): N.XM_T_FLOAT64}


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class GroupObject:
    """Owns the object an xm_*_create made: _create(name, device, cfg) in the subclass's __init__, close() / with / __del__ here."""
    _destroy = None  # the destroy symbol's name

    def _create(self, create: str, device: int, cfg) -> None:
        self._lib = N.load_library()
        self._h = None
        h = C.c_void_p()
        N.check(getattr(self._lib, create)(int(device), C.byref(cfg), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stack(maps, dtype=None, what: str = "surfaces") -> np.ndarray:
    """one array of a 3-D array, a 2-D array or a list of 2-D arrays (an empty list: ValueError)"""
    if isinstance(maps, np.ndarray):
        return maps if maps.ndim == 3 else maps[None]
    arrs = [np.asarray(a) for a in maps]
    if not arrs:
        raise ValueError(f"no {what}")
    if dtype is None:
        dtype = np.float32 if all(a.dtype == np.float32 for a in arrs) else np.float64
    return np.stack([a.astype(dtype, copy=False) for a in arrs])


def surface_group(surfaces, h: int, w: int) -> np.ndarray:
    """A caller's time surfaces as the contiguous (n, h, w) array of a group call: float32 if every one is float32, else float64."""
    grp = _stack(surfaces)
    if grp.ndim != 3 or grp.shape[1:] != (h, w) or grp.shape[0] == 0:
        raise ValueError(f"time surfaces must be (n, {h}, {w}), got {grp.shape}")
    if grp.dtype not in T_DTYPES:
        grp = grp.astype(np.float64)
    return np.ascontiguousarray(grp)


def map_group(maps, h: int, w: int, dtype, what: str = "maps") -> np.ndarray:
    """A caller's maps (depth_init, depth_optim) as the contiguous (n, h, w) array of `dtype`."""
    grp = _stack(maps, dtype, what)
    if grp.ndim != 3 or grp.shape[1:] != (h, w) or grp.shape[0] == 0:
        raise ValueError(f"{what} must be (n, {h}, {w}), got {grp.shape}")
    return np.ascontiguousarray(grp, dtype=dtype)


def stats_dtype(struct) -> np.dtype:
    """the numpy dtype of a _native.py stats struct (names, offsets and itemsize as ctypes lays it out): a device buffer of them,
    copied back as bytes, is read with .view(stats_dtype(N.xm_..._stats))"""
    names, formats, offsets = [], [], []
    for name, ctype in struct._fields_:
        shape = ()
        while hasattr(ctype, "_length_"):  # (an array field)
            shape, ctype = shape + (ctype._length_,), ctype._type_
        base = np.dtype(ctype).newbyteorder("<")
        names.append(name)
        formats.append((base, shape) if shape else base)
        offsets.append(getattr(struct, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": C.sizeof(struct)})
