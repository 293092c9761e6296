"""ESL's depth optimisation on the GPU: the point-wise refinement behind ESL-init (python/eval/compute_depth_esl.py:104-129
depth_optimization, :232-236 its caller), which writes esl/depth_optim.  Camera time surfaces and their depth_init maps in,
depth_optim maps out: normalise, fill the empty pixels with 1 / v'[0][0], and per pixel with an initial depth one bounded scalar
minimisation (scipy's minimize_scalar(method="bounded"), restated) of the patch distance between the camera's time surface and the
projector's at the pixel's projection -- in one device call per group of surfaces (xm_esl_optim_time_surfaces; kernels in
csrc/xmaps_esloptim.hpp).

In scope: this solver.  The bilateral filter and the TV denoiser behind it (:243-244), hence esl/depth_optim_filtered, the
evaluation's ground truth: x_maps_amd/esl_filter.py, which takes this module's device buffer as it is.

PINNED against the reference's own depth_optimization on the installed scipy (golden G13): the solver, the cost with its truncation
and patch norm, the fill and the bounds.  UNPINNED: undistortPoints, Rodrigues and projectPoints against a real cv2 (DESIGN.md
section 5); they are calibration.py's geometry.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._group import T_DTYPES as _T_DTYPES, GroupObject, map_group, ptr as _ptr, surface_group
from .calibration import CamProjCalibrationParams, rodrigues, stereo_rectify
from .esl_init import get_projector_time_surface

WINDOW_SIZE, MAX_ITER, XATOL = 3, 500, 1e-5  # compute_depth_esl.py:151; scipy's _minimize_scalar_bounded


def make_rt(R, T) -> np.ndarray:
    """Rt[12] = {R' row-major, t}: esl_utilities.py:144-146 keeps the rotation and the translation in a float32 matrix;
    project_and_backproject_punkt sends the rotation through cv2.Rodrigues and cv2.projectPoints turns the vector back into a
    matrix.  Both in float64, once."""
    R32 = np.asarray(R, np.float64).astype(np.float32).astype(np.float64)
    t32 = np.asarray(T, np.float64).reshape(3).astype(np.float32).astype(np.float64)
    return np.concatenate((rodrigues(rodrigues(R32)).ravel(), t32))


def build_esl_optim_tables(cp: CamProjCalibrationParams, window_size: int = WINDOW_SIZE) -> dict:
    """What depth_optimization takes from loadCalibParams (esl_utilities.py:124-150), from a from_ESL_yaml object: the two pinhole
    models as they are, Rt (make_rt), and P1[0, 3] from the same stereo_rectify call and assignment as build_esl_init_tables."""
    size = (cp.rect_image_width, cp.rect_image_height)
    _, _, _, P1, _ = stereo_rectify(cp.projector_K, cp.projector_D, cp.camera_K, cp.camera_D, size, cp.cam2proj_R, cp.cam2proj_T)
    return {
        "cam_w": cp.camera_width, "cam_h": cp.camera_height, "proj_w": cp.projector_width, "proj_h": cp.projector_height,
        "window_size": window_size, "p1_03": float(P1[0, 3]),
        "cam_K": np.asarray(cp.camera_K, np.float64), "cam_D": np.asarray(cp.camera_D, np.float64).ravel()[:5],
        "proj_K": np.asarray(cp.projector_K, np.float64), "proj_D": np.asarray(cp.projector_D, np.float64).ravel()[:5],
        "Rt": make_rt(cp.cam2proj_R, cp.cam2proj_T),
        "proj_surface": get_projector_time_surface(cp.projector_width, cp.projector_height),
    }


class EslOptimStats:
    __slots__ = ("n_optimised", "n_evals", "n_hit_limit", "n_bad_bounds", "lo", "hi")

    def __init__(self, c):
        self.n_optimised, self.n_evals = int(c.n_optimised), int(c.n_evals)
        self.n_hit_limit, self.n_bad_bounds = int(c.n_hit_limit), int(c.n_bad_bounds)
        self.lo, self.hi = float(c.lo), float(c.hi)

    def __repr__(self):
        return (f"EslOptimStats(n_optimised={self.n_optimised}, n_evals={self.n_evals}, n_hit_limit={self.n_hit_limit}, "
                f"n_bad_bounds={self.n_bad_bounds}, lo={self.lo!r}, hi={self.hi!r})")


class EslOptim(GroupObject):
    """with EslOptim(tables) as opt: res = opt.depths_from_time_surfaces(surfaces, depth_init)

    tables: build_esl_optim_tables' dict, or any dict with cam_w, cam_h, proj_w, proj_h, cam_K, cam_D, proj_K, proj_D, Rt[12], p1_03,
    proj_surface float32 [proj_h][proj_w] (window_size / max_iter / xatol: 3 / 500 / 1e-5)."""
    _destroy = "xm_esl_optim_destroy"

    def __init__(self, tables: dict, device: int = 0):
        self.cam_w, self.cam_h = int(tables["cam_w"]), int(tables["cam_h"])
        self.proj_w, self.proj_h = int(tables["proj_w"]), int(tables["proj_h"])
        proj = np.ascontiguousarray(tables["proj_surface"], dtype=np.float32)
        if proj.shape != (self.proj_h, self.proj_w):
            raise ValueError(f"proj_surface must be ({self.proj_h}, {self.proj_w}), got {proj.shape}")
        vec = lambda key, n: np.ascontiguousarray(tables[key], dtype=np.float64).reshape(-1)[:n]
        parts = {"cam_K": vec("cam_K", 9), "cam_D": vec("cam_D", 5), "proj_K": vec("proj_K", 9), "proj_D": vec("proj_D", 5), "Rt": vec("Rt", 12)}
        for key, n in (("cam_K", 9), ("cam_D", 5), ("proj_K", 9), ("proj_D", 5), ("Rt", 12)):
            if parts[key].size != n:
                raise ValueError(f"{key} must hold {n} values, got {parts[key].size}")
        cfg = N.xm_esl_optim_config(C.sizeof(N.xm_esl_optim_config), self.cam_w, self.cam_h, self.proj_w, self.proj_h,
                                    int(tables.get("window_size", 0)), int(tables.get("max_iter", 0)), 0, float(tables.get("xatol", 0.0)),
                                    float(tables["p1_03"]), (C.c_double * 9)(*parts["cam_K"]), (C.c_double * 5)(*parts["cam_D"]),
                                    (C.c_double * 9)(*parts["proj_K"]), (C.c_double * 5)(*parts["proj_D"]), (C.c_double * 12)(*parts["Rt"]),
                                    _ptr(proj))
        self._create("xm_esl_optim_create", device, cfg)

    def depths_from_time_surfaces(self, surfaces, depth_init, want_nfev: bool = False):
        """A group of camera time surfaces (a list of [cam_h][cam_w] arrays or one 3-D array; float32 or float64, 0 = no event) and
        their depth_init maps (float32, the same shape) in ONE device call -> [(depth_optim f32 [cam_h][cam_w], nfev u16 | None,
        EslOptimStats)] per surface.  An all-zero surface and one with a single non-zero value give zero maps."""
        grp = surface_group(surfaces, self.cam_h, self.cam_w)
        n = grp.shape[0]
        d0 = map_group(depth_init, self.cam_h, self.cam_w, np.float32, "depth_init")
        if d0.shape != grp.shape:
            raise ValueError(f"depth_init must be {grp.shape}, got {d0.shape}")
        depth = np.empty(grp.shape, np.float32)
        nfev = np.empty(grp.shape, np.uint16) if want_nfev else None
        st = (N.xm_esl_optim_stats * n)()
        N.check(self._lib.xm_esl_optim_time_surfaces(self._h, _ptr(grp), _T_DTYPES[grp.dtype], n, N.XM_MEM_HOST, _ptr(d0), _ptr(depth),
                                                     _ptr(nfev), C.cast(st, C.c_void_p)))
        return [(depth[i], nfev[i] if want_nfev else None, EslOptimStats(st[i])) for i in range(n)]

    def time_surfaces_device(self, surfaces_ptr, dtype, n: int, depth_init_ptr, depth_ptr, nfev_ptr=None, stats_ptr=None):
        """the same on device memory of this object's device (raw pointers; synchronous); depth_init_ptr may be the buffer
        EslInit.time_surfaces_device has just filled"""
        N.check(self._lib.xm_esl_optim_time_surfaces(self._h, surfaces_ptr, _T_DTYPES[np.dtype(dtype)], int(n), N.XM_MEM_DEVICE,
                                                     depth_init_ptr, depth_ptr, nfev_ptr, stats_ptr))
