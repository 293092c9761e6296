"""ESL's ground truth on the GPU: the two filters behind the depth optimisation (python/eval/compute_depth_esl.py:243-244:
cv2.bilateralFilter(depth_optim, 5, 3, 3), then esl_utilities.py:194-224 denoise_tv(mu=0.5)), which write
esl/depth_optim_filtered -- the file every row of the reference's evaluation table is scored against.  depth_optim maps in,
depth_optim_filtered maps out, in one device call per group (xm_esl_filter_maps; kernels in csrc/xmaps_eslfilter.hpp): a
float32 bilateral filter, then split Bregman in float64 around scipy's lsqr, restated, with the reference's swapped dims.

PINNED against the reference's own denoise_tv on the installed scipy's lsqr (golden G14): its call, the dims swap, every
parameter, the solver.  UNPINNED: pylops' loop, stacking, stencil and threshold, its float32 operator dtype, and cv2's bilateral
filter; include/xmaps.h holds the contract both stages are built to.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._group import GroupObject, map_group, ptr as _ptr

NITER_OUTER, NITER_INNER, ITER_LIM = 20, 10, 5  # esl_utilities.py:208-209, :222
NO_BILATERAL, NO_TV = N.XM_ESL_FILTER_NO_BILATERAL, N.XM_ESL_FILTER_NO_TV


class EslFilterStats:
    __slots__ = ("lo", "hi", "final_norm", "n_outer", "n_lsqr", "sum_itn", "istop_count")

    def __init__(self, c):
        self.lo, self.hi, self.final_norm = float(c.lo), float(c.hi), float(c.final_norm)
        self.n_outer, self.n_lsqr, self.sum_itn = int(c.n_outer), int(c.n_lsqr), int(c.sum_itn)
        self.istop_count = tuple(int(v) for v in c.istop_count)

    def __repr__(self):
        return (f"EslFilterStats(lo={self.lo!r}, hi={self.hi!r}, final_norm={self.final_norm!r}, n_outer={self.n_outer}, "
                f"n_lsqr={self.n_lsqr}, sum_itn={self.sum_itn}, istop_count={self.istop_count})")


class EslFilter(GroupObject):
    """with EslFilter(width, height) as flt: res = flt.filter_maps(depth_optim)

    Keyword parameters default to the reference's call (0 = default): d, sigma_color, sigma_space, mu, lambda0, lambda1,
    niter_outer, niter_inner, iter_lim, tol, tau, damp; flags: NO_BILATERAL | NO_TV runs one stage alone."""
    _destroy = "xm_esl_filter_destroy"

    def __init__(self, width: int, height: int, device: int = 0, flags: int = 0, **params):
        self.width, self.height, self.flags = int(width), int(height), int(flags)
        ints = {k: int(params.pop(k, 0)) for k in ("d", "niter_outer", "niter_inner", "iter_lim")}
        dbl = {k: float(params.pop(k, 0.0)) for k in ("sigma_color", "sigma_space", "mu", "lambda0", "lambda1", "tol", "tau", "damp")}
        if params:
            raise TypeError(f"unknown parameters: {sorted(params)}")
        self.n_calls = (ints["niter_outer"] or NITER_OUTER) * (ints["niter_inner"] or NITER_INNER)
        cfg = N.xm_esl_filter_config(C.sizeof(N.xm_esl_filter_config), self.width, self.height, self.flags, ints["d"], ints["niter_outer"],
                                     ints["niter_inner"], ints["iter_lim"], dbl["sigma_color"], dbl["sigma_space"], dbl["mu"],
                                     dbl["lambda0"], dbl["lambda1"], dbl["tol"], dbl["tau"], dbl["damp"])
        self._create("xm_esl_filter_create", device, cfg)

    def filter_maps(self, depth_optim, want_bilateral: bool = False, want_trips: bool = False):
        """A group of depth_optim maps (a list of [height][width] arrays or one 3-D array, float32) in ONE device call ->
        [(depth_optim_filtered f64 [height][width], bilateral f32 | None, trips u8 [niter_outer * niter_inner] | None,
        EslFilterStats)] per map.  trips: lsqr's iterations of every inner call, 0xFF where none ran."""
        grp = map_group(depth_optim, self.height, self.width, np.float32)
        n = grp.shape[0]
        out = np.full(grp.shape, np.nan, np.float64)
        bil = np.full(grp.shape, np.nan, np.float32) if want_bilateral and not self.flags & NO_BILATERAL else None
        trips = np.full((n, self.n_calls), 0xFF, np.uint8) if want_trips else None
        st = (N.xm_esl_filter_stats * n)()
        N.check(self._lib.xm_esl_filter_maps(self._h, _ptr(grp), n, N.XM_MEM_HOST, _ptr(out), _ptr(bil), _ptr(trips),
                                             C.cast(st, C.c_void_p)))
        return [(out[i], None if bil is None else bil[i], None if trips is None else trips[i], EslFilterStats(st[i])) for i in range(n)]

    def maps_device(self, depth_optim_ptr, n: int, filtered_ptr, bilateral_ptr=None, trips_ptr=None, stats_ptr=None):
        """the same on device memory of this object's device (raw pointers; synchronous); depth_optim_ptr may be the buffer
        EslOptim.time_surfaces_device has just filled"""
        N.check(self._lib.xm_esl_filter_maps(self._h, depth_optim_ptr, int(n), N.XM_MEM_DEVICE, filtered_ptr, bilateral_ptr, trips_ptr,
                                             stats_ptr))

    def last_launches(self) -> int:
        v = C.c_uint64()
        N.check(self._lib.xm_esl_filter_last_launches(self._h, C.byref(v)))
        return int(v.value)
