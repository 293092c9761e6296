"""MC3D on the GPU: the other baseline the reference's evaluation runs beside X-maps (python/eval/mc3d_baseline.py;
create_evaluation_table.py's "MC3D" and "MC3D (1 sec)" rows).  Camera time surfaces in, depth maps out: 3 x 3 median, the camera
pixel's rectified position, the projector pixel the time stamp names, a windowed search down that projector column for the
nearest rectified row, P1[0,3] / disparity -- in one device call per group of surfaces (xm_mc3d_time_surfaces; kernel in
csrc/xmaps_mc3d.hpp, the definition in include/xmaps.h).

UNPINNED: cv2.medianBlur(., 3) stands in as the exact median of nine with replicated borders (eval_table.median_blur3), and the
float maps come from calibration.undistort_points, not cv2.undistortPoints; neither has been compared with a cv2 run (DESIGN.md
section 5).  The search itself is pinned against the reference's own compute_disparity (golden G12).  cv2.medianBlur accepts no
float64 image; here a float64 surface is blurred in float64 (its id then comes from a float64 product, as the reference's would).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._group import T_DTYPES as _T_DTYPES, GroupObject, ptr as _ptr, surface_group
from .calibration import CamProjCalibrationParams, init_undistort_rectify_map_inverse, stereo_rectify

POISON = N.XM_MC3D_POISON
SAT = 1 << 30  # finite entries saturate here: include/xmaps.h says why that cannot change a result
MAX_ROW_DIFF = 50  # mc3d_baseline.py:71


def default_nc(proj_h: int) -> int:
    return int(proj_h / 15)  # mc3d_baseline.py:43-45


def mc3d_int_maps(mapx: np.ndarray, mapy: np.ndarray) -> np.ndarray:
    """(x, y) int32 pairs of a float map pair as the reference's int(map[y, x]) makes them: truncated toward zero (entries in
    (-1, 0) become 0, not -1); NaN / +-inf -> POISON (int() raises there and the reference drops the pixel); finite values beyond
    +-2^30 saturate."""
    out = np.empty(mapx.shape + (2,), np.int32)
    for k, m in enumerate((mapx, mapy)):
        m = np.asarray(m, np.float64)
        fin = np.isfinite(m)
        t = np.trunc(np.clip(np.where(fin, m, 0.0), -float(SAT), float(SAT))).astype(np.int32)
        out[..., k] = np.where(fin, t, POISON)
    return out


def build_mc3d_tables(cp: CamProjCalibrationParams, rectify_size=None, maps_on_device: bool = False, device: int = 0) -> dict:
    """The tables of mc3d_baseline.py:99-114 from a CamProjCalibrationParams.from_ESL_yaml object.  esl_utilities.py:133-150
    (loadCalibParams, alpha = -1) calls cv2.stereoRectify(projector, camera, ...) and names its FIRST pair R0 / P0 and its SECOND
    R1 / P1; the camera's map takes R0 / P0 and the projector's R1 / P1 (:109-114) -- the same call and the same assignment as
    build_esl_init_tables makes -- and, unlike ESL-init's map, the projector keeps its own distortion (:109-111).  rectify_size: the image size handed to the rectification; the reference passes the
    PROJECTOR's size there (:99-101) and uses the 3 x frame only for the limits of the search.  The reference builds the camera map
    at projector size but only its [:cam_h, :cam_w] corner is ever read: it is built at camera size.
    maps_on_device: the two float maps on the device (x_maps_amd.rig_maps: the same bits); mc3d_int_maps stays NumPy."""
    size = rectify_size or (cp.projector_width, cp.projector_height)
    R0, R1, P0, P1, _ = stereo_rectify(cp.projector_K, cp.projector_D, cp.camera_K, cp.camera_D, size, cp.cam2proj_R, cp.cam2proj_T)
    inverse = init_undistort_rectify_map_inverse
    if maps_on_device:
        from . import rig_maps
        inverse = lambda *a: rig_maps.init_undistort_rectify_map_inverse(*a, device=device)
    proj_mapx, proj_mapy = inverse(cp.projector_K, cp.projector_D, R1, P1, (cp.projector_width, cp.projector_height))
    img_mapx, img_mapy = inverse(cp.camera_K, cp.camera_D, R0, P0, (cp.camera_width, cp.camera_height))
    return {
        "cam_w": cp.camera_width, "cam_h": cp.camera_height, "proj_w": cp.projector_width, "proj_h": cp.projector_height,
        "cam_map": mc3d_int_maps(img_mapx, img_mapy), "proj_map": mc3d_int_maps(proj_mapx, proj_mapy),
        "cam_map_f32": (img_mapx, img_mapy), "proj_map_f32": (proj_mapx, proj_mapy),
        "p1_03": float(P1[0, 3]), "nc": default_nc(cp.projector_height), "max_row_diff": MAX_ROW_DIFF,
        "rect_x_limit": 3 * cp.projector_height, "rect_y_limit": 3 * cp.projector_width,  # (:100 with :52-57: swapped)
        "R0": R0, "R1": R1, "P0": P0, "P1": P1,
    }


class Mc3dStats:
    __slots__ = ("n_nonzero", "n_positive", "n_in_rect", "n_out_of_range", "n_poisoned", "n_matched", "n_disp_overflow")

    def __init__(self, c):
        for k in self.__slots__:
            setattr(self, k, int(getattr(c, k)))

    def __repr__(self):
        return "Mc3dStats(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.__slots__) + ")"


class Mc3d(GroupObject):
    """with Mc3d(tables) as mc: depths = mc.depths_from_time_surfaces(surfaces)

    tables: build_mc3d_tables' dict, or any dict with cam_w, cam_h, proj_w, proj_h, cam_map int32 [cam_h][cam_w][2], proj_map
    int32 [proj_h][proj_w][2] (mc3d_int_maps), p1_03 (nc, max_row_diff, rect_x_limit / rect_y_limit: the reference's)."""
    _destroy = "xm_mc3d_destroy"

    def __init__(self, tables: dict, device: int = 0):
        self.cam_w, self.cam_h = int(tables["cam_w"]), int(tables["cam_h"])
        self.proj_w, self.proj_h = int(tables["proj_w"]), int(tables["proj_h"])
        cam = np.ascontiguousarray(tables["cam_map"], dtype=np.int32)
        proj = np.ascontiguousarray(tables["proj_map"], dtype=np.int32)
        if cam.shape != (self.cam_h, self.cam_w, 2) or proj.shape != (self.proj_h, self.proj_w, 2):
            raise ValueError(f"table shapes do not match the dimensions: {cam.shape}, {proj.shape}")
        cfg = N.xm_mc3d_config(C.sizeof(N.xm_mc3d_config), self.cam_w, self.cam_h, self.proj_w, self.proj_h,
                               int(tables.get("nc", 0)), int(tables.get("max_row_diff", 0)), int(tables.get("rect_x_limit", 0)),
                               int(tables.get("rect_y_limit", 0)), 0, float(tables["p1_03"]), _ptr(cam), _ptr(proj))
        self._create("xm_mc3d_create", device, cfg)

    def depths_from_time_surfaces(self, surfaces, want_disparity: bool = False, blur: bool = True):
        """A group of camera time surfaces (a list of [cam_h][cam_w] arrays or one 3-D array; float32 or float64, used as stored,
        0 = no event) in ONE device call -> [(depth f32 [cam_h][cam_w], disparity u16 | None, Mc3dStats)] per surface.  An
        all-zero surface gives zero maps and zero counts: the reference skips it."""
        grp = surface_group(surfaces, self.cam_h, self.cam_w)
        n = grp.shape[0]
        depth = np.empty((n, self.cam_h, self.cam_w), np.float32)
        disp = np.empty((n, self.cam_h, self.cam_w), np.uint16) if want_disparity else None
        st = (N.xm_mc3d_stats * n)()
        N.check(self._lib.xm_mc3d_time_surfaces(self._h, _ptr(grp), _T_DTYPES[grp.dtype], n, N.XM_MEM_HOST,
                                                0 if blur else N.XM_MC3D_NO_BLUR, _ptr(depth), _ptr(disp), C.cast(st, C.c_void_p)))
        return [(depth[i], disp[i] if want_disparity else None, Mc3dStats(st[i])) for i in range(n)]

    def time_surfaces_device(self, surfaces_ptr, dtype, n: int, depth_ptr, disp_ptr=None, stats_ptr=None, blur: bool = True):
        """the same on device memory of this object's device (raw pointers; synchronous)"""
        N.check(self._lib.xm_mc3d_time_surfaces(self._h, surfaces_ptr, _T_DTYPES[np.dtype(dtype)], int(n), N.XM_MEM_DEVICE,
                                                0 if blur else N.XM_MC3D_NO_BLUR, depth_ptr, disp_ptr, stats_ptr))
