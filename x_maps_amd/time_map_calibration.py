"""Calibrate the projector time map from a white-frame recording, on the GPU (kernels in csrc/xmaps_timecal.hpp, the entries
xm_timecal_* of include/xmaps.h).

The paper's recipe (section 3.3, "Time map calibration"): project a white image onto a plane; build several camera time maps,
normalise each to (0, 1) and average them per pixel; make a binary map and find the projected frame's corners; warp the irregular
quadrilateral to the projector's width x height with a projective transformation; interpolate missing values linearly between
actual lines.  The reference ships no code for this step: the arithmetic is this build's definition (include/xmaps.h spells it
out), pinned bit for bit to the NumPy oracle of tests/time_cal_cases.py.

    cal = TimeMapCalibrator((cam_w, cam_h))
    cal.add_surfaces(surfaces)            # or cal.add_frames(engine, frames)
    cal.mean(min_share=0.5)               # ValueError when no usable corners are found (solve(corners=...) still works)
    time_map, stats = cal.solve((proj_w, proj_h))
    tables = calibration.build_tables(cp, projector_time_map=time_map)

Accumulate, mean, corners, warp and fill run on the device; the homography -- an 8 x 8 solve -- stays on the host.  Corner finding
takes the extreme core pixels along the two diagonals: a quadrilateral rotated near 45 degrees needs `corners=`.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native as N

# the 8 symmetries of the square: which of the camera corners (TL, TR, BR, BL) the projector corners (0, 0), (W-1, 0), (W-1, H-1),
# (0, H-1) take.  0 is the identity, 1 .. 3 rotate, 4 .. 7 mirror.
CORNER_ORDERS = ((0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (1, 0, 3, 2), (0, 3, 2, 1), (3, 2, 1, 0), (2, 1, 0, 3))


@dataclass
class TimeCalStats:
    n_added: int = 0
    n_skipped: int = 0
    n_valid: int = 0
    n_core: int = 0
    corners: Optional[tuple] = None  # ((x, y) x 4: TL, TR, BR, BL) as detected; None without a core pixel
    n_missing: int = 0
    n_unfilled: int = 0
    min_count: int = 0
    h: Optional[np.ndarray] = None   # the homography solve() used
    corner_error: Optional[str] = None  # why the detected corners are unusable (mean(need_corners=False))

    @property
    def n_used(self) -> int:
        return self.n_added - self.n_skipped


def homography(src, dst) -> np.ndarray:
    """h[9] with h8 = 1 and dst ~ h (src, 1) for four point pairs: np.linalg.solve on the usual 8 x 8 system"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2):
        raise ValueError("four (x, y) pairs on each side")
    A = np.zeros((8, 8), np.float64)
    b = np.zeros(8, np.float64)
    for i in range(4):
        u, v = float(src[i, 0]), float(src[i, 1])
        x, y = float(dst[i, 0]), float(dst[i, 1])
        A[2 * i] = (u, v, 1.0, 0.0, 0.0, 0.0, -u * x, -v * x)
        A[2 * i + 1] = (0.0, 0.0, 0.0, u, v, 1.0, -u * y, -v * y)
        b[2 * i], b[2 * i + 1] = x, y
    return np.concatenate((np.linalg.solve(A, b), (1.0,)))


def check_corners(corners) -> None:
    """ValueError unless the four points are distinct and TL -> TR -> BR -> BL is strictly convex (the device entry's rule; for
    integer points in integer arithmetic)"""
    c = [(p[0], p[1]) for p in corners]
    if len(c) != 4:
        raise ValueError("four corners: TL, TR, BR, BL")
    if len(set(c)) != 4:
        raise ValueError("two corners coincide")
    cross = []
    for k in range(4):
        p, q, r = c[k], c[(k + 1) % 4], c[(k + 2) % 4]
        cross.append((q[0] - p[0]) * (r[1] - q[1]) - (q[1] - p[1]) * (r[0] - q[0]))
    if not (all(v > 0 for v in cross) or all(v < 0 for v in cross)):
        raise ValueError("the corner quadrilateral is not strictly convex")


class TimeMapCalibrator:
    def __init__(self, cam_size, device: int = 0):
        self.cam_w, self.cam_h = int(cam_size[0]), int(cam_size[1])
        self._lib = N.load_library()
        self._tc = C.c_void_p()
        N.check(self._lib.xm_timecal_create(int(device), self.cam_w, self.cam_h, C.byref(self._tc)))
        self.stats = TimeCalStats()

    def close(self):
        if getattr(self, "_tc", None):
            self._lib.xm_timecal_destroy(self._tc)
            self._tc = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- accumulate ----
    def reset(self):
        N.check(self._lib.xm_timecal_reset(self._tc))
        self.stats = TimeCalStats()

    def _counts(self):
        a, s = C.c_uint64(), C.c_uint64()
        N.check(self._lib.xm_timecal_counts(self._tc, C.byref(a), C.byref(s)))
        self.stats.n_added, self.stats.n_skipped = int(a.value), int(s.value)

    def add_surfaces(self, arrays):
        """camera time surfaces [n][cam_h][cam_w] (or one [cam_h][cam_w]), float32 or float64, 0 = no event, in this order"""
        a = np.asarray(arrays)
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("a time surface is float32 or float64")
        a = np.ascontiguousarray(a)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (self.cam_h, self.cam_w):
            raise ValueError(f"surfaces must be [n][{self.cam_h}][{self.cam_w}], not {a.shape}")
        if len(a):
            N.check(self._lib.xm_timecal_add_surfaces(self._tc, C.c_void_p(a.ctypes.data),
                                                     N.XM_T_FLOAT32 if a.dtype == np.float32 else N.XM_T_FLOAT64, len(a), N.XM_MEM_HOST))
        self._counts()

    def add_frames(self, engine, frames, select="first", max_group: int = 64):
        """frames of events (EventCD arrays) through XMapsEngine.frames_to_time_surfaces, float64 surfaces, in this order"""
        frames = list(frames)
        for k in range(0, len(frames), max_group):
            surf, _ = engine.frames_to_time_surfaces(frames[k:k + max_group], select=select, dtype=np.float64)
            self.add_surfaces(surf)

    KERNELS = ("k_surf_extrema", "k_tcal_accumulate", "k_tcal_mean", "k_tcal_corners", "k_tcal_warp", "k_tcal_fill")

    def kernel_ms(self) -> dict:
        """the kernels' device times of the last calls that ran them (HIP events around each launch), in ms"""
        ms = (C.c_float * 6)()
        N.check(self._lib.xm_timecal_kernel_ms(self._tc, ms))
        return dict(zip(self.KERNELS, (float(v) for v in ms)))

    # ---- mean, corners ----
    def _take(self, st: N.xm_timecal_stats):
        s = self.stats
        s.n_added, s.n_skipped, s.n_valid, s.n_core = int(st.n_added), int(st.n_skipped), int(st.n_valid), int(st.n_core)
        s.corners = tuple((int(st.corners[k][0]), int(st.corners[k][1])) for k in range(4)) if st.n_core else None
        s.n_missing, s.n_unfilled = int(st.n_missing), int(st.n_unfilled)

    def mean(self, min_share: float = 0.5, want_arrays: bool = False, need_corners: bool = True):
        """valid = a pixel seen in at least min_count = max(1, ceil(min_share * surfaces used)) surfaces; the mean there; the four
        corners.  Returns the stats (want_arrays: (mean float64, valid bool, stats)).  ValueError when no usable corners are found
        (need_corners=False: stats.corner_error names the reason instead); the mean stays in the object either way, so
        solve(corners=...) can follow."""
        self._counts()
        min_count = max(1, int(math.ceil(min_share * self.stats.n_used)))
        mean = np.empty((self.cam_h, self.cam_w), np.float64) if want_arrays else None
        valid = np.empty((self.cam_h, self.cam_w), np.uint8) if want_arrays else None
        st = N.xm_timecal_stats()
        rc = self._lib.xm_timecal_mean(self._tc, min_count, None if mean is None else C.c_void_p(mean.ctypes.data),
                                       None if valid is None else C.c_void_p(valid.ctypes.data), N.XM_MEM_HOST, C.byref(st))
        if rc in (N.XM_OK, N.XM_ERR_INVALID):  # (the arguments are sound: XM_ERR_INVALID is the corner verdict, given after the stats)
            self._take(st)
            self.stats.min_count = min_count
            self.stats.corner_error = N.last_error() if rc else None
        if rc != N.XM_ERR_INVALID or need_corners:
            N.check(rc)
        return (mean, valid.astype(bool), self.stats) if want_arrays else self.stats

    def set_mean(self, mean, valid):
        """the state mean() leaves, from arrays of the caller's own (the warp as a stage)"""
        m = np.ascontiguousarray(mean, np.float64)
        v = np.ascontiguousarray(np.asarray(valid).astype(np.uint8))
        if m.shape != (self.cam_h, self.cam_w) or v.shape != m.shape:
            raise ValueError(f"mean and valid must be [{self.cam_h}][{self.cam_w}]")
        st = N.xm_timecal_stats()
        rc = self._lib.xm_timecal_set_mean(self._tc, C.c_void_p(m.ctypes.data), C.c_void_p(v.ctypes.data), N.XM_MEM_HOST, C.byref(st))
        if rc in (N.XM_OK, N.XM_ERR_INVALID):
            self._take(st)
            self.stats.corner_error = N.last_error() if rc else None
        N.check(rc)
        return self.stats

    # ---- warp, fill ----
    def warp(self, h, proj_size, want_present: bool = False):
        """warp and fill with a homography of the caller's (projector pixel -> camera position): the float32 map [proj_h][proj_w]"""
        W, H = int(proj_size[0]), int(proj_size[1])
        hh = np.ascontiguousarray(h, np.float64).ravel()
        if hh.shape != (9,):
            raise ValueError("h has nine entries")
        out = np.empty((H, W), np.float32)
        present = np.empty((H, W), np.uint8) if want_present else None
        st = N.xm_timecal_stats()
        N.check(self._lib.xm_timecal_warp(self._tc, hh.ctypes.data_as(C.POINTER(C.c_double)), W, H, C.c_void_p(out.ctypes.data),
                                          None if present is None else C.c_void_p(present.ctypes.data), N.XM_MEM_HOST, C.byref(st)))
        self.stats.n_missing, self.stats.n_unfilled = int(st.n_missing), int(st.n_unfilled)
        self.stats.h = hh.copy()
        return (out, present.astype(bool)) if want_present else out

    def solve(self, proj_size, corners=None, corner_order: int = 0):
        """(the projector-space time map float32 [proj_h][proj_w], stats) after mean().  corners = four (x, y) pairs TL, TR, BR, BL
        in the camera image instead of the detected ones; corner_order = which symmetry of the square maps them to the projector's
        corners (CORNER_ORDERS; 0 = TL is projector (0, 0))."""
        if not 0 <= int(corner_order) < 8:
            raise ValueError("corner_order is one of the 8 symmetries of the square: 0 .. 7")
        if corners is None:
            if self.stats.corners is None or self.stats.corner_error:
                raise ValueError(self.stats.corner_error or "no corners: mean() comes first")
            corners = self.stats.corners
        corners = [(float(p[0]), float(p[1])) for p in corners]
        check_corners(corners)
        W, H = int(proj_size[0]), int(proj_size[1])
        src = ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))
        h = homography(src, [corners[k] for k in CORNER_ORDERS[int(corner_order)]])
        return self.warp(h, (W, H)), self.stats
