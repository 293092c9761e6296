"""Small ESL-init rigs for the CPU and GPU tests: random int16 maps (entries outside both frames, a rectified pixel that two camera
pixels reference, full / clipped / empty windows), remap-like projector rows, and groups of time surfaces with the two degenerate
ones (all zero; a single value)."""
import numpy as np

G11 = "g11_esl_init.npz"


def projector_rows(rng, h, w, density=0.8, run=3):
    """rows as a nearest remap of a rising surface makes them: runs of equal values with holes"""
    base = np.sort(rng.random((h, (w + run - 1) // run)).astype(np.float32), axis=1)
    rows = np.repeat(base, run, axis=1)[:, :w].copy()
    rows[rng.random((h, w)) >= density] = 0
    return np.ascontiguousarray(rows)


def make_rig(seed=3, cam_w=37, cam_h=13, rect_w=1100, rect_h=20, max_disp=900):
    rng = np.random.default_rng(seed)
    cam_to_rect = np.stack((rng.integers(-2, cam_w + 2, (rect_h, rect_w)), rng.integers(-2, cam_h + 2, (rect_h, rect_w))), -1)
    rect_to_cam = np.stack((rng.integers(-5, rect_w + 5, (cam_h, cam_w)), rng.integers(-2, rect_h + 2, (cam_h, cam_w))), -1)
    full = max(rect_w - max_disp, 1)  # columns below this have an unclipped window
    rect_to_cam[0, :8, 0] = rng.integers(0, full, 8)       # full windows
    rect_to_cam[1, :4, 0] = [rect_w - 1, rect_w - 5, rect_w - 6, rect_w - 7]  # empty, empty, one column, two columns
    rect_to_cam[:2, :8, 1] = rng.integers(0, rect_h, (2, 8))
    rect_to_cam[2, 0] = rect_to_cam[0, 0]                  # one rectified pixel, two camera pixels
    rect_to_cam[cam_h - 1, cam_w - 1] = rect_to_cam[0, 1]
    for y, x in ((0, 0), (0, 1), (1, 2), (1, 3)):          # ... whose camera source lies inside the camera
        rx, ry = rect_to_cam[y, x]
        cam_to_rect[ry, rx] = (rng.integers(0, cam_w), rng.integers(0, cam_h))
    return {"cam_w": cam_w, "cam_h": cam_h, "rect_w": rect_w, "rect_h": rect_h,
            "cam_to_rect": np.ascontiguousarray(cam_to_rect.astype(np.int16)),
            "rect_to_cam": np.ascontiguousarray(rect_to_cam.astype(np.int16)),
            "proj_rect": projector_rows(rng, rect_h, rect_w)}


def make_surfaces(rig, n, dtype, seed=5):
    """n surfaces; from three on, [1] is all zero and [2] holds a single value"""
    rng = np.random.default_rng(seed)
    s = rng.random((n, rig["cam_h"], rig["cam_w"])) * 3e4 + 1e3
    s[rng.random(s.shape) < 0.3] = 0
    s = s.astype(dtype)
    if n >= 3:
        s[1] = 0
        s[2] = np.where(s[2] != 0, dtype(1234.5), 0)
    return np.ascontiguousarray(s)
