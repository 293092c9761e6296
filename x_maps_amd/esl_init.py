"""ESL-init on the GPU: the baseline the reference's evaluation runs beside X-maps (python/eval/compute_depth_esl.py:179-226, up
to depth_init; create_evaluation_table.py's "ESL (init)" row).  Camera time surfaces in, depth_init maps out: normalise, rectify
by nearest remap, disparity_init's search over the rectified projector time surface, remap back to the camera, P1[0,3] / disparity
-- in one device call per group of surfaces (xm_esl_init_time_surfaces; kernels in csrc/xmaps_eslinit.hpp).

In scope: this initialisation.  ESL's optimisation behind it (scipy minimize_scalar) is esl_optim.py; its bilateral filter and TV
denoising are out of scope.
The MC3D baseline is mc3d.py.

UNPINNED: the float -> int16 rounding of the two remap tables (mapf_to_i16, np.rint as for every other map of this build) stands
in for cv2.remap(INTER_NEAREST) on float maps; it has not been compared with a cv2 run.  The search itself
is pinned against the reference's own disparity_init (golden G11).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from ._group import T_DTYPES as _T_DTYPES, GroupObject, ptr as _ptr, surface_group
from .calibration import (CamProjCalibrationParams, init_undistort_rectify_map, init_undistort_rectify_map_inverse, mapf_to_i16,
                          remap_nearest, stereo_rectify)

MIN_DISP, MAX_DISP = 5, 900  # compute_depth_esl.py:74


def get_projector_time_surface(proj_w: int, proj_h: int) -> np.ndarray:
    """compute_depth_esl.py:94-101: proj[y][x] = (x * H + y) / (W * H) -- column by column, the quotient in Python float,
    stored float32.  Pixel (0, 0) is 0 = "no data" to the search, as in the reference."""
    x, y = np.meshgrid(np.arange(proj_w, dtype=np.int64), np.arange(proj_h, dtype=np.int64))
    return ((x * proj_h + y) / float(proj_w * proj_h)).astype(np.float32)  # (int64 / float: one float64 division, as Python's)


def _pair_i16(mapx: np.ndarray, mapy: np.ndarray) -> np.ndarray:
    """(x, y) int16 pairs of a float map pair through mapf_to_i16.  A forward map of a rectified frame several times the camera's
    size points far outside the camera near its rim (beyond int16, or NaN where the distortion polynomial folds over); such an entry
    is outside every frame whatever its exact value, so it is saturated first -- the remap's border either way."""
    sat = lambda m: np.clip(np.nan_to_num(m, nan=-32768.0, posinf=32767.0, neginf=-32768.0), -32768.0, 32767.0).astype(np.float32)
    return np.ascontiguousarray(np.stack((mapf_to_i16(sat(mapx)), mapf_to_i16(sat(mapy))), -1))


def build_esl_init_tables(cp: CamProjCalibrationParams, maps_on_device: bool = False, device: int = 0) -> dict:
    """The tables of compute_depth_esl.py:179-201 from a CamProjCalibrationParams.from_ESL_yaml object.  The camera is "camera 0"
    there: it takes R0 / P0, the projector R1 / P1 -- which esl_utilities.py:133-150 (loadCalibParams, alpha = -1, the default
    CALIB_ZERO_DISPARITY) fills with the FIRST and the SECOND pair of cv2.stereoRectify(projector, camera, ...), the same call and
    the same assignment as build_tables makes for X-maps.  The rectified frame is 3 x the projector (cp.rect_image_*), the back
    map is built at the camera's size, and the projector's distortion is ignored in its map (:197).
    maps_on_device: the three maps and the remap on the device (x_maps_amd.rig_maps: the same dict, bit for bit; the projector's
    forward map and its time surface are never stored, only proj_rect comes back)."""
    size = (cp.rect_image_width, cp.rect_image_height)
    R0, R1, P0, P1, _ = stereo_rectify(cp.projector_K, cp.projector_D, cp.camera_K, cp.camera_D, size, cp.cam2proj_R, cp.cam2proj_T)
    if maps_on_device:
        from . import rig_maps
        c2r = rig_maps.forward_map(cp.camera_K, cp.camera_D, R0, P0, size, want_maps=False, want_pair=True, device=device)["pair_i16"]
        r2c = rig_maps.inverse_map(cp.camera_K, cp.camera_D, R0, P0, (cp.camera_width, cp.camera_height), want_maps=False,
                                   want_pair=True, device=device)["pair_i16"]
        proj_rect = rig_maps.forward_map(cp.projector_K, np.zeros(5), R1, P1, size, want_maps=False,
                                         linear_time=(cp.projector_width, cp.projector_height, False), border="constant",
                                         device=device)["remap"]
        return {
            "cam_w": cp.camera_width, "cam_h": cp.camera_height, "rect_w": size[0], "rect_h": size[1],
            "cam_to_rect_map": c2r, "rect_to_cam_map": r2c, "proj_rect": proj_rect,
            "p1_03": float(P1[0, 3]), "min_disp": MIN_DISP, "max_disp": MAX_DISP,
            "R0": R0, "R1": R1, "P0": P0, "P1": P1,
        }
    # rectified view -> image plane (:189-191) and image plane -> rectified plane (:193-198)
    disp_mapx, disp_mapy = init_undistort_rectify_map_inverse(cp.camera_K, cp.camera_D, R0, P0, (cp.camera_width, cp.camera_height))
    img_mapx, img_mapy = init_undistort_rectify_map(cp.camera_K, cp.camera_D, R0, P0, size)
    proj_mapx, proj_mapy = init_undistort_rectify_map(cp.projector_K, np.zeros(5), R1, P1, size)
    proj = get_projector_time_surface(cp.projector_width, cp.projector_height)
    return {
        "cam_w": cp.camera_width, "cam_h": cp.camera_height, "rect_w": size[0], "rect_h": size[1],
        "cam_to_rect_map": _pair_i16(img_mapx, img_mapy),
        "rect_to_cam_map": _pair_i16(disp_mapx, disp_mapy),
        "proj_rect": np.ascontiguousarray(remap_nearest(proj, proj_mapx, proj_mapy, "constant")),  # (:201)
        "p1_03": float(P1[0, 3]), "min_disp": MIN_DISP, "max_disp": MAX_DISP,
        "R0": R0, "R1": R1, "P0": P0, "P1": P1,
    }


class EslInitStats:
    __slots__ = ("n_nonzero", "n_searched", "n_matched", "lo", "hi")

    def __init__(self, c):
        self.n_nonzero, self.n_searched, self.n_matched = int(c.n_nonzero), int(c.n_searched), int(c.n_matched)
        self.lo, self.hi = float(c.lo), float(c.hi)

    def __repr__(self):
        return (f"EslInitStats(n_nonzero={self.n_nonzero}, n_searched={self.n_searched}, n_matched={self.n_matched}, "
                f"lo={self.lo!r}, hi={self.hi!r})")


class EslInit(GroupObject):
    """with EslInit(tables) as esl: depths = esl.depths_from_time_surfaces(surfaces)

    tables: build_esl_init_tables' dict, or any dict with cam_w, cam_h, rect_w, rect_h, cam_to_rect_map int16 [rect_h][rect_w][2],
    rect_to_cam_map int16 [cam_h][cam_w][2], proj_rect float32 [rect_h][rect_w], p1_03 (min_disp / max_disp: 5 / 900)."""
    _destroy = "xm_esl_init_destroy"

    def __init__(self, tables: dict, device: int = 0):
        self.cam_w, self.cam_h = int(tables["cam_w"]), int(tables["cam_h"])
        self.rect_w, self.rect_h = int(tables["rect_w"]), int(tables["rect_h"])
        c2r = np.ascontiguousarray(tables["cam_to_rect_map"], dtype=np.int16)
        r2c = np.ascontiguousarray(tables["rect_to_cam_map"], dtype=np.int16)
        proj = np.ascontiguousarray(tables["proj_rect"], dtype=np.float32)
        if c2r.shape != (self.rect_h, self.rect_w, 2) or r2c.shape != (self.cam_h, self.cam_w, 2) or proj.shape != (self.rect_h, self.rect_w):
            raise ValueError(f"table shapes do not match the dimensions: {c2r.shape}, {r2c.shape}, {proj.shape}")
        self.min_disp, self.max_disp = int(tables.get("min_disp", MIN_DISP)), int(tables.get("max_disp", MAX_DISP))
        cfg = N.xm_esl_init_config(C.sizeof(N.xm_esl_init_config), self.cam_w, self.cam_h, self.rect_w, self.rect_h, self.min_disp,
                                   self.max_disp, 0, float(tables["p1_03"]), _ptr(c2r), _ptr(r2c), _ptr(proj))
        self._create("xm_esl_init_create", device, cfg)

    def depths_from_time_surfaces(self, surfaces, want_disparity: bool = False):
        """A group of camera time surfaces (a list of [cam_h][cam_w] arrays or one 3-D array; float32 or float64, 0 = no event)
        in ONE device call -> [(depth_init f32 [cam_h][cam_w], disp_cam u16 | None, EslInitStats)] per surface.  An all-zero
        surface and one with a single non-zero value give zero maps (n_searched == 0): the reference skips the former."""
        grp = surface_group(surfaces, self.cam_h, self.cam_w)
        n = grp.shape[0]
        depth = np.empty((n, self.cam_h, self.cam_w), np.float32)
        disp = np.empty((n, self.cam_h, self.cam_w), np.uint16) if want_disparity else None
        st = (N.xm_esl_init_stats * n)()
        N.check(self._lib.xm_esl_init_time_surfaces(self._h, _ptr(grp), _T_DTYPES[grp.dtype], n, N.XM_MEM_HOST, _ptr(depth), _ptr(disp),
                                                    C.cast(st, C.c_void_p)))
        return [(depth[i], disp[i] if want_disparity else None, EslInitStats(st[i])) for i in range(n)]

    def time_surfaces_device(self, surfaces_ptr, dtype, n: int, depth_ptr, disp_ptr=None, stats_ptr=None):
        """the same on device memory of this object's device (raw pointers; synchronous)"""
        N.check(self._lib.xm_esl_init_time_surfaces(self._h, surfaces_ptr, _T_DTYPES[np.dtype(dtype)], int(n), N.XM_MEM_DEVICE,
                                                    depth_ptr, disp_ptr, stats_ptr))

    def disparity_init(self, cam_rect) -> np.ndarray:
        """the reference's disparity_init(cam_rect, proj_rect) on a rectified camera image (float64 [rect_h][rect_w]) against this
        object's projector surface -> uint16 [rect_h][rect_w]"""
        cam = np.ascontiguousarray(cam_rect, dtype=np.float64)
        if cam.shape != (self.rect_h, self.rect_w):
            raise ValueError(f"cam_rect must be ({self.rect_h}, {self.rect_w}), got {cam.shape}")
        out = np.empty(cam.shape, np.uint16)
        N.check(self._lib.xm_esl_init_stage_disparity(self._h, _ptr(cam), _ptr(out)))
        return out
