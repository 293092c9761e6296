"""Plain NumPy restatement of the ESL-init baseline (python/eval/compute_depth_esl.py:72-101, 204-226 of the reference) -- the
yardstick of xm_esl_init_* (tests/test_gpu_esl_init.py), itself compared array for array with the reference's own outputs (golden
G11, tests/test_esl_init_ref_cpu.py).  oracle/ is frozen; this follows the precedent of tests/eval_ref.py.

The five steps of one camera time surface:
  1. normalise()            lo / hi over the non-zero pixels, (f64(v) - lo) / (hi - lo), negatives to 0 (float64 first: G7's convention)
  2. remap_nearest_i16()    cam_rect[r][c] = v'[my][mx] through the int16 pair map, 0 outside the source (constant border)
  3. disparity_init()       per pixel > 0: window [c + min_disp, c + max_disp) clipped at the row's end, its non-zero entries are the
                            candidates, more than one -> offset of the FIRST minimum of (f64(p) - e)^2, else 0
  4. remap_nearest_i16()    disp_cam[y][x] = disparity[ry][rx], 0 outside
  5. depth_from_disparity() f32(p1_03 / f64(disp)), 0 where the disparity is 0
depth_init_staged() composes them on whole images; depth_init_fused() is the definition the device's fused kernel follows: it
searches only the rectified pixels step 4 references and never builds a rectified image.  The two agree exactly."""
import numpy as np


def get_projector_time_surface(proj_w, proj_h):
    """:94-101: proj[y][x] = (x * H + y) / (W * H), the quotient in Python float, stored float32"""
    out = np.zeros((proj_h, proj_w), np.float32)
    for x in range(proj_w):
        for y in range(proj_h):
            out[y, x] = (x * proj_h + y) / (proj_w * proj_h)
    return out


def normalise(surface):
    """-> (v' float64 or None when nothing can be searched, stats dict n_nonzero / lo / hi)"""
    img = np.asarray(surface).astype(np.float64)
    nz = img != 0
    n = int(nz.sum())
    if n == 0:
        return None, {"n_nonzero": 0, "lo": 0.0, "hi": 0.0}
    lo, hi = float(img[nz].min()), float(img[nz].max())
    st = {"n_nonzero": n, "lo": lo, "hi": hi}
    if not hi > lo:
        return None, st
    v = (img - lo) / (hi - lo)
    v[v < 0] = 0
    return v, st


def remap_nearest_i16(img, map_xy):
    """out[i][j] = img[my][mx], (mx, my) = map_xy[i][j]; 0 where the entry lies outside img"""
    h, w = img.shape
    mx, my = map_xy[..., 0].astype(np.int64), map_xy[..., 1].astype(np.int64)
    ok = (mx >= 0) & (mx < w) & (my >= 0) & (my < h)
    out = np.zeros(map_xy.shape[:2], img.dtype)
    out[ok] = img[my[ok], mx[ok]]
    return out


def search(e, proj_row, c, min_disp=5, max_disp=900):
    """the disparity of one rectified pixel with camera value e > 0 in column c"""
    win = proj_row[c + min_disp:c + max_disp]  # (slicing clips at the row's end; may be empty)
    idx = np.flatnonzero(win)
    if idx.size <= 1:
        return 0
    d = win[idx].astype(np.float64) - np.float64(e)
    with np.errstate(over="ignore", under="ignore"):
        cost = d * d
    return min_disp + int(idx[np.argmin(cost)])  # np.argmin: the first minimum


def disparity_init(cam_rect, proj_rect, min_disp=5, max_disp=900):
    """step 3 on a whole rectified frame -> uint16"""
    cam = np.asarray(cam_rect, np.float64)
    proj = np.asarray(proj_rect, np.float32)
    assert cam.shape == proj.shape
    out = np.zeros(cam.shape, np.uint16)
    for r, c in zip(*np.nonzero(cam > 0)):
        out[r, c] = search(cam[r, c], proj[r], int(c), min_disp, max_disp)
    return out


def depth_from_disparity(disp_cam, p1_03):
    d = np.asarray(disp_cam).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = (np.float64(p1_03) / d.astype(np.float64)).astype(np.float32)
    depth[d == 0] = 0
    return depth


def _stats(st, n_searched, n_matched):
    return dict(st, n_searched=int(n_searched), n_matched=int(n_matched))


def depth_init_staged(surface, cam_to_rect, rect_to_cam, proj_rect, p1_03, min_disp=5, max_disp=900):
    """-> (depth f32, disp_cam u16, stats, disparity_rect u16): steps 1-5 on whole images"""
    ch, cw = np.asarray(surface).shape
    v, st = normalise(surface)
    if v is None:
        return np.zeros((ch, cw), np.float32), np.zeros((ch, cw), np.uint16), _stats(st, 0, 0), np.zeros(proj_rect.shape, np.uint16)
    cam_rect = remap_nearest_i16(v, cam_to_rect)
    disp = disparity_init(cam_rect, proj_rect, min_disp, max_disp)
    disp_cam = remap_nearest_i16(disp, rect_to_cam)
    live = remap_nearest_i16((cam_rect > 0).astype(np.uint8), rect_to_cam)
    return depth_from_disparity(disp_cam, p1_03), disp_cam, _stats(st, live.sum(), (disp_cam != 0).sum()), disp


def depth_init_fused(surface, cam_to_rect, rect_to_cam, proj_rect, p1_03, min_disp=5, max_disp=900):
    """-> (depth f32, disp_cam u16, stats): per camera pixel, only the rectified pixels the back map references"""
    ch, cw = np.asarray(surface).shape
    rh, rw = proj_rect.shape
    disp_cam = np.zeros((ch, cw), np.uint16)
    v, st = normalise(surface)
    n_searched = 0
    if v is not None:
        for y in range(ch):
            for x in range(cw):
                rx, ry = int(rect_to_cam[y, x, 0]), int(rect_to_cam[y, x, 1])
                if not (0 <= rx < rw and 0 <= ry < rh):
                    continue
                mx, my = int(cam_to_rect[ry, rx, 0]), int(cam_to_rect[ry, rx, 1])
                if not (0 <= mx < cw and 0 <= my < ch):
                    continue
                e = v[my, mx]
                if e > 0:
                    n_searched += 1
                    disp_cam[y, x] = search(e, proj_rect[ry], rx, min_disp, max_disp)
    return depth_from_disparity(disp_cam, p1_03), disp_cam, _stats(st, n_searched, (disp_cam != 0).sum())
