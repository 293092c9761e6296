"""A rig's rectification maps on the GPU: calibration.py's init_undistort_rectify_map, init_undistort_rectify_map_inverse and
remap_nearest with the NumPy functions' arguments and results, bit for bit (kernels in csrc/xmaps_rigmaps.hpp, the entries
xm_rig_forward_map / xm_rig_inverse_map / xm_rig_build_xmaps_tables of include/xmaps.h).  The pin is to this project's NumPy, not
to OpenCV.  stereo_rectify, rodrigues and the 3 x 3 inverse stay on the host: a few hundred flops, pinned to
OpenCV's stored outputs by tests/test_calibration_cpu.py.

forward_map / inverse_map give every output of the two kernels (the saturated int16 pair of esl_init._pair_i16, the int16 maps of
mapf_to_i16, the remap of an image or of the linear projector time map, which is evaluated in place: no time-map table exists);
forward_config / inverse_config make the C structs for callers that bring device pointers of their own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

_BORDERS = {"constant": N.XM_RIG_BORDER_CONSTANT, "replicate": N.XM_RIG_BORDER_REPLICATE}


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _k4(K):
    K = np.asarray(K, np.float64)
    return (C.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _d5(D):
    d = np.zeros(5) if D is None else np.asarray(D, np.float64).ravel()
    out = np.zeros(5)
    out[:min(5, len(d))] = d[:5]  # (calibration._dist5)
    return (C.c_double * 5)(*out)


def _m9(M):
    return (C.c_double * 9)(*np.asarray(M, np.float64)[:3, :3].ravel())


def _p4(P):
    P = np.asarray(P, np.float64)
    return (C.c_double * 4)(P[0, 0], P[1, 1], P[0, 2], P[1, 2])


def _border(border: str) -> int:
    if border not in _BORDERS:
        raise ValueError(f"border must be 'constant' or 'replicate', not {border!r}")
    return _BORDERS[border]


def forward_ir(R, P) -> np.ndarray:
    """inv(P[:3,:3] @ R) as calibration.init_undistort_rectify_map forms it (on the host)"""
    return np.linalg.inv(np.asarray(P, np.float64)[:3, :3] @ np.asarray(R, np.float64))


def forward_config(K, D, R, P, size, *, linear_time=None, src_size=None, src=None, border="constant", border_value=0.0,
                   mapx_in=None, mapy_in=None) -> N.xm_rig_forward_config:
    """xm_rig_forward_config for a (width, height) target frame.  Remap source: linear_time = (proj_w, proj_h, scan_upwards), or
    src = address of a float32 image of src_size = (width, height).  src / mapx_in / mapy_in are plain addresses (host or device,
    by the call's `mem`): the caller keeps what they point to alive."""
    w, h = size
    cfg = N.xm_rig_forward_config()
    cfg.struct_size = C.sizeof(N.xm_rig_forward_config)
    cfg.width, cfg.height = int(w), int(h)
    cfg.border, cfg.border_value = _border(border), float(border_value)
    if linear_time is not None:
        cfg.src_kind = N.XM_RIG_SRC_LINEAR_TIME
        cfg.src_width, cfg.src_height, cfg.scan_upwards = int(linear_time[0]), int(linear_time[1]), int(bool(linear_time[2]))
    elif src is not None:
        cfg.src_kind = N.XM_RIG_SRC_IMAGE
        cfg.src_width, cfg.src_height = int(src_size[0]), int(src_size[1])
        cfg.src = src
    if K is not None:
        cfg.K, cfg.D, cfg.ir = _k4(K), _d5(D), _m9(forward_ir(R, P))
    cfg.mapx_in, cfg.mapy_in = mapx_in, mapy_in
    return cfg


def inverse_config(K, D, R, P, size) -> N.xm_rig_inverse_config:
    w, h = size
    cfg = N.xm_rig_inverse_config()
    cfg.struct_size = C.sizeof(N.xm_rig_inverse_config)
    cfg.width, cfg.height = int(w), int(h)
    cfg.K, cfg.D, cfg.R, cfg.P = _k4(K), _d5(D), _m9(R), _p4(P)
    return cfg


def forward_map(K, D, R, P, size, *, want_maps=True, want_pair=False, linear_time=None, src=None, border="constant",
                border_value=0.0, device: int = 0) -> dict:
    """The forward map's outputs as host arrays: "mapx" / "mapy" float32 [h][w] (want_maps), "pair_i16" int16 [h][w][2]
    (want_pair: esl_init._pair_i16), "remap" float32 [h][w] (linear_time = (proj_w, proj_h, scan_upwards), or src = a 2-D float32
    image) and "kernel_ms"."""
    w, h = int(size[0]), int(size[1])
    img = None
    if src is not None:
        img = np.ascontiguousarray(src, dtype=np.float32)
        if img.ndim != 2:
            raise ValueError("src must be 2-D")
    cfg = forward_config(K, D, R, P, size, linear_time=linear_time, src=None if img is None else img.ctypes.data,
                         src_size=None if img is None else (img.shape[1], img.shape[0]), border=border, border_value=border_value)
    res = {}
    if want_maps:
        res["mapx"], res["mapy"] = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    if want_pair:
        res["pair_i16"] = np.empty((h, w, 2), np.int16)
    if linear_time is not None or img is not None:
        res["remap"] = np.empty((h, w), np.float32)
    out = N.xm_rig_forward_outputs(_ptr(res.get("mapx")), _ptr(res.get("mapy")), _ptr(res.get("pair_i16")), _ptr(res.get("remap")))
    N.check(N.load_library().xm_rig_forward_map(device, C.byref(cfg), C.byref(out), N.XM_MEM_HOST))
    res["kernel_ms"] = float(out.kernel_ms)
    return res


def inverse_map(K, D, R, P, size, *, want_maps=True, want_i16=False, want_pair=False, device: int = 0) -> dict:
    """The inverse map's outputs as host arrays: "mapx" / "mapy" float32 [h][w] (want_maps), "mapx_i16" / "mapy_i16" int16 [h][w]
    (want_i16: mapf_to_i16), "pair_i16" int16 [h][w][2] (want_pair) and "kernel_ms".  ValueError naming the map where
    mapf_to_i16's assertion would fail."""
    w, h = int(size[0]), int(size[1])
    cfg = inverse_config(K, D, R, P, size)
    res = {}
    if want_maps:
        res["mapx"], res["mapy"] = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    if want_i16:
        res["mapx_i16"], res["mapy_i16"] = np.empty((h, w), np.int16), np.empty((h, w), np.int16)
    if want_pair:
        res["pair_i16"] = np.empty((h, w, 2), np.int16)
    out = N.xm_rig_inverse_outputs(_ptr(res.get("mapx")), _ptr(res.get("mapy")), _ptr(res.get("mapx_i16")), _ptr(res.get("mapy_i16")),
                                   _ptr(res.get("pair_i16")))
    N.check(N.load_library().xm_rig_inverse_map(device, C.byref(cfg), C.byref(out), N.XM_MEM_HOST))
    res["kernel_ms"] = float(out.kernel_ms)
    return res


# ---- calibration.py's three functions -----------------------------------------------------------------------------------
def init_undistort_rectify_map(K, D, R, P, size, device: int = 0):
    """calibration.init_undistort_rectify_map on the device: (mapx, mapy) float32 [h][w]"""
    r = forward_map(K, D, R, P, size, device=device)
    return r["mapx"], r["mapy"]


def init_undistort_rectify_map_inverse(K, D, R, P, size, device: int = 0):
    """calibration.init_undistort_rectify_map_inverse on the device: (mapx, mapy) float32 [h][w]"""
    r = inverse_map(K, D, R, P, size, device=device)
    return r["mapx"], r["mapy"]


def remap_nearest(img, mapx, mapy, border: str, border_value=0.0, device: int = 0):
    """calibration.remap_nearest on the device, for a 2-D float32 image and float32 maps.  (Under "replicate" a NaN entry samples
    the first row / column and +-inf the nearest edge; NumPy's own result is undefined there.)"""
    img = np.ascontiguousarray(img)
    mx, my = np.ascontiguousarray(mapx), np.ascontiguousarray(mapy)
    if img.dtype != np.float32 or mx.dtype != np.float32 or my.dtype != np.float32:
        raise ValueError("the device remap takes a float32 image and float32 maps")
    if img.ndim != 2 or mx.ndim != 2 or mx.shape != my.shape:
        raise ValueError("a 2-D image and two 2-D maps of one shape")
    h, w = mx.shape
    cfg = forward_config(None, None, None, None, (w, h), src=img.ctypes.data, src_size=(img.shape[1], img.shape[0]), border=border,
                         border_value=border_value, mapx_in=mx.ctypes.data, mapy_in=my.ctypes.data)
    res = np.empty((h, w), np.float32)
    out = N.xm_rig_forward_outputs(None, None, None, _ptr(res))
    N.check(N.load_library().xm_rig_forward_map(device, C.byref(cfg), C.byref(out), N.XM_MEM_HOST))
    return res


# ---- calibration.build_tables' chain ----------------------------------------------------------------------------------
def build_xmaps_tables(cp, R1, R2, P1, P2, *, scan_upwards: bool, zero_undistort_proj_map: bool, time_map_border: str,
                       x_map_width: int, t_px_scale: int, x_offset: int, time_map_rect=None, device: int = 0) -> dict:
    """xm_rig_build_xmaps_tables for calibration.build_tables (projector = camera 1 of the pair: the camera takes R1 / P1, the
    projector R2 / P2).  Returns time_map_rect, x_map, cam_mapx_f32 / cam_mapy_f32, cam_mapx_i16 / cam_mapy_i16,
    disp_proj_mapxy_i16 and kernel_ms (forward map, X-map, camera inverse map, projector inverse map)."""
    cfg = N.xm_rig_tables_config()
    cfg.struct_size = C.sizeof(N.xm_rig_tables_config)
    cfg.cam_width, cfg.cam_height = int(cp.camera_width), int(cp.camera_height)
    cfg.proj_width, cfg.proj_height = int(cp.projector_width), int(cp.projector_height)
    cfg.rect_width, cfg.rect_height = int(cp.rect_image_width), int(cp.rect_image_height)
    cfg.scan_upwards, cfg.border = int(bool(scan_upwards)), _border(time_map_border)
    cfg.x_map_width, cfg.t_px_scale, cfg.x_offset, cfg.num_scanlines = int(x_map_width), int(t_px_scale), int(x_offset), int(cp.projector_width)
    cfg.cam_K, cfg.cam_D, cfg.cam_R, cfg.cam_P = _k4(cp.camera_K), _d5(cp.camera_D), _m9(R1), _p4(P1)
    cfg.proj_K, cfg.proj_D, cfg.proj_R, cfg.proj_P = _k4(cp.projector_K), _d5(cp.projector_D), _m9(R2), _p4(P2)
    cfg.proj_fwd_D = _d5(None if zero_undistort_proj_map else cp.projector_D)
    cfg.proj_ir = _m9(forward_ir(R2, P2))
    rh, rw, ch, cw, ph, pw = cfg.rect_height, cfg.rect_width, cfg.cam_height, cfg.cam_width, cfg.proj_height, cfg.proj_width
    tm_in = None
    if time_map_rect is not None:
        tm_in = np.ascontiguousarray(time_map_rect, dtype=np.float32)
        if tm_in.shape != (rh, rw):
            raise ValueError(f"the rectified time map must be {rh} x {rw}, not {tm_in.shape}")
        cfg.time_map_rect_in = tm_in.ctypes.data
    res = {"time_map_rect": np.empty((rh, rw), np.float32), "x_map": np.empty((rh, int(x_map_width)), np.int16),
           "cam_mapx_f32": np.empty((ch, cw), np.float32), "cam_mapy_f32": np.empty((ch, cw), np.float32),
           "cam_mapx_i16": np.empty((ch, cw), np.int16), "cam_mapy_i16": np.empty((ch, cw), np.int16),
           "disp_proj_mapxy_i16": np.empty((ph, pw, 2), np.int16)}
    out = N.xm_rig_tables_outputs(_ptr(res["time_map_rect"]), _ptr(res["x_map"]), _ptr(res["cam_mapx_f32"]), _ptr(res["cam_mapy_f32"]),
                                  _ptr(res["cam_mapx_i16"]), _ptr(res["cam_mapy_i16"]), _ptr(res["disp_proj_mapxy_i16"]))
    N.check(N.load_library().xm_rig_build_xmaps_tables(device, C.byref(cfg), C.byref(out)))
    res["kernel_ms"] = tuple(float(v) for v in out.kernel_ms)
    return res
