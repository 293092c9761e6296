"""The small rigs of the rig-map tests and their NumPy expectations (x_maps_amd/calibration.py: the project's own NumPy, which is
not under test there).  tests/test_rig_maps_cases_cpu.py asserts that these rigs reach the edges the GPU tests rely on, so a
missing edge fails on the CPU and cannot pass silently on the GPU.

  S   the ESL calibration (tests/golden/g6_esl_calib.npz) with both K scaled by 1/8: camera 80 x 60, projector 135 x 240, rectified
      frame 3 x projector = 405 x 720 (the evaluation's shape); constant border, scanning downwards
  S2  ("S prime") the same with strong distortion on both sides: forward-map entries up to 1.6e9, thousands of exact .5 ties
  L   the live shape: projector distortion zeroed, rect = round(2.75 x camera) = 220 x 165, scan_upwards, replicate border
  T   hand-made, no stereo_rectify: D = 0, R = I, fx = fy = P00 = P11 = 64, integer cx / cy, P02 = 10.5, P12 = 3.5 -- every entry
      of its inverse map is an exact .5 tie

No width or height is a multiple of 64 or 256 and every map holds more pixels than one block of 256 threads.
"""
import functools
import os
from dataclasses import dataclass, replace

import numpy as np

from x_maps_amd import calibration as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
S2_CAM_D = (-0.4, 0.9, 0.01, -0.02, -3.0)
S2_PROJ_D = (0.1, -0.2, 0.002, 0.001, 0.05)


@dataclass(frozen=True)
class View:
    """one camera of a rectified pair: what the two map functions take"""
    name: str
    K: np.ndarray
    D: np.ndarray
    R: np.ndarray
    P: np.ndarray
    size: tuple         # (width, height) of its own frame: the inverse map's
    rect_size: tuple    # (width, height) of the rectified frame: the forward map's

    @property
    def args(self):
        return self.K, self.D, self.R, self.P


def _scaled_k(K, s):
    K = np.array(K, np.float64)
    K[:2] *= s
    return K


@functools.lru_cache(maxsize=None)
def g6():
    return dict(np.load(os.path.join(GOLDEN, "g6_esl_calib.npz")))


@functools.lru_cache(maxsize=None)
def params(rig: str) -> C.CamProjCalibrationParams:
    g = g6()
    if rig == "full":  # the reference's ESL rig at full size
        return C.CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g["camera_K"], g["camera_D"].ravel(), g["projector_K"],
                                          g["projector_D"].ravel(), g["R"], g["T"])
    s = C.CamProjCalibrationParams(80, 60, 135, 240, 405, 720, _scaled_k(g["camera_K"], 0.125), g["camera_D"].ravel().copy(),
                                   _scaled_k(g["projector_K"], 0.125), g["projector_D"].ravel().copy(), g["R"], g["T"])
    if rig == "S":
        return s
    if rig == "S2":
        return replace(s, camera_D=np.array(S2_CAM_D), projector_D=np.array(S2_PROJ_D))
    if rig == "L":
        return replace(s, projector_D=np.zeros(5), rect_image_width=round(80 * 2.75), rect_image_height=round(60 * 2.75))
    raise KeyError(rig)


# how build_tables / build_eval_tables are called for each rig
TABLE_KW = {"S": dict(scan_upwards=False, zero_undistort_proj_map=True, time_map_border="constant"),
            "S2": dict(scan_upwards=False, zero_undistort_proj_map=True, time_map_border="constant"),
            "L": dict(scan_upwards=True, zero_undistort_proj_map=False, time_map_border="replicate")}


@functools.lru_cache(maxsize=None)
def views(rig: str):
    """(camera, projector) of a rig: projector = camera 1 of the stereo pair, so the camera takes R1 / P1 and the projector R2 / P2
    (calibration.build_tables)"""
    if rig == "T":
        K = np.array([[64.0, 0, 40.0], [0, 64.0, 30.0], [0, 0, 1]])
        P = np.array([[64.0, 0, 10.5, 0], [0, 64.0, 3.5, 0], [0, 0, 1, 0]])
        v = View("T", K, np.zeros(5), np.eye(3), P, (83, 61), (83, 61))
        return v, v
    cp = params(rig)
    rs = (cp.rect_image_width, cp.rect_image_height)
    R1, R2, P1, P2, _ = C.stereo_rectify(cp.projector_K, cp.projector_D, cp.camera_K, cp.camera_D, rs, cp.cam2proj_R, cp.cam2proj_T)
    return (View(rig + "-camera", cp.camera_K, np.asarray(cp.camera_D), R1, P1, (cp.camera_width, cp.camera_height), rs),
            View(rig + "-projector", cp.projector_K, np.asarray(cp.projector_D), R2, P2, (cp.projector_width, cp.projector_height), rs))


def forward_views(rig: str):
    """the forward maps the builders make: the camera's, and the projector's with zeroed distortion"""
    cam, proj = views(rig)
    return cam, replace(proj, name=proj.name + "-D0", D=np.zeros(5))


@functools.lru_cache(maxsize=None)
def forward_expected(rig: str, which: int):
    """calibration.init_undistort_rectify_map of forward_views(rig)[which] (read-only arrays, computed once)"""
    v = forward_views(rig)[which]
    with np.errstate(all="ignore"):
        mx, my = C.init_undistort_rectify_map(*v.args, v.rect_size)
    mx.setflags(write=False), my.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def inverse_expected(rig: str, which: int):
    """calibration.init_undistort_rectify_map_inverse of views(rig)[which]"""
    v = views(rig)[which]
    mx, my = C.init_undistort_rectify_map_inverse(*v.args, v.size)
    mx.setflags(write=False), my.setflags(write=False)
    return mx, my


def out_of_i16_view():
    """S2's projector with P02 shifted by 40 000: its inverse mapx leaves int16, mapf_to_i16 raises"""
    proj = views("S2")[1]
    P = proj.P.copy()
    P[0, 2] += 40000.0
    return replace(proj, name="S2-projector-shifted", P=P)


def undistort_points_elementwise(K, D, R, P, size):
    """calibration.init_undistort_rectify_map_inverse restated element by element, the way a kernel computes it: the rotation as the
    three sums R[i,0] * x + R[i,1] * y + R[i,2], left to right, instead of the matrix product; everything else as undistort_points
    writes it"""
    w, h = size
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    px, py = u.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = (float(c) for c in C._dist5(D))
    x0 = (px - cx) / fx
    y0 = (py - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1 + r2 * (k1 + r2 * (k2 + r2 * k3)))
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    R = np.asarray(R, np.float64)
    xr = R[0, 0] * x + R[0, 1] * y + R[0, 2]
    yr = R[1, 0] * x + R[1, 1] * y + R[1, 2]
    wr = R[2, 0] * x + R[2, 1] * y + R[2, 2]
    x, y = xr / wr, yr / wr
    return (P[0, 0] * x + P[0, 2]).astype(np.float32), (P[1, 1] * y + P[1, 2]).astype(np.float32)


def ties(m: np.ndarray) -> np.ndarray:
    """entries that sit exactly on .5: where rint's half-to-even is decided"""
    m = np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(m) & (np.abs(m - np.trunc(m)) == 0.5)


def bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    """float32 arrays: equal as int32 bit patterns where finite, np.array_equal(..., equal_nan=True) elsewhere"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    fin = np.isfinite(a)
    if not np.array_equal(fin, np.isfinite(b)):
        return False
    return bool(np.array_equal(a[fin].view(np.int32), b[fin].view(np.int32)) and np.array_equal(a[~fin], b[~fin], equal_nan=True))
