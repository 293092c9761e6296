"""Vectorised NumPy restatement of the MC3D baseline (python/eval/mc3d_baseline.py:15-18, 40-78, 129-140 of the reference) -- the
yardstick of xm_mc3d_* (tests/test_gpu_mc3d.py), itself compared array for array with the reference's own outputs (golden G12,
tests/test_mc3d_ref_cpu.py).  oracle/ is frozen; this follows the precedent of tests/esl_init_ref.py.

The steps of one camera time surface, used as stored (no normalisation):
  1. median_blur3()        median of the 3 x 3 neighbourhood, borders replicated, in the surface's own type (cv2.medianBlur(., 3)
                           for float32; cv2 takes no float64 image: the float64 form is this build's definition)
  2. search()              per pixel v > 0: camera entry inside the (swapped) rect limits, id = int(W * H * v) in the surface's
                           type, id < W * H, the window [max(proj_y - nc, 0), min(proj_y + nc, H)) down projector column proj_x,
                           the FIRST minimum of |yc - yp|, accepted if <= max_row_diff, disp = xp - xc kept if > 0; poison in
                           the camera entry or anywhere in the window drops the pixel
  3. depth_from_disparity  f32(p1_03 / f64(disp)), 0 where the disparity is 0
Maps are the int32 pairs of x_maps_amd.mc3d.mc3d_int_maps (int_maps() here restates it the slow, obvious way)."""
import numpy as np

POISON = -2 ** 31
SAT = 1 << 30
STAT_KEYS = ("n_nonzero", "n_positive", "n_in_rect", "n_out_of_range", "n_poisoned", "n_matched", "n_disp_overflow")


def int_maps(mapx, mapy):
    """int(map[y, x]) entry by entry: truncation toward zero, POISON where int() raises, saturation at +-2^30"""
    out = np.empty(np.shape(mapx) + (2,), np.int32)
    for k, m in enumerate((mapx, mapy)):
        for idx in np.ndindex(*np.shape(m)):
            try:
                out[idx + (k,)] = max(-SAT, min(SAT, int(m[idx])))
            except (ValueError, OverflowError):
                out[idx + (k,)] = POISON
    return out


def median_blur3(img):
    img = np.asarray(img)
    assert img.dtype in (np.float32, np.float64)
    p = np.pad(img, 1, mode="edge")
    h, w = img.shape
    stack = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 0)
    return np.sort(stack, axis=0)[4]


def search(v, cam_map, proj_map, nc=None, max_row_diff=50, rect_x_limit=None, rect_y_limit=None):
    """step 2 on a whole (already blurred) surface -> (disparity int64 [h][w] -- values beyond 65535 still in it --, counts)"""
    v = np.asarray(v)
    H, W = proj_map.shape[:2]
    nc = int(H / 15) if nc is None else nc
    x_lim = 3 * H if rect_x_limit is None else rect_x_limit
    y_lim = 3 * W if rect_y_limit is None else rect_y_limit
    disp = np.zeros(v.shape, np.int64)
    st = dict.fromkeys(STAT_KEYS, 0)
    pos = v > 0
    st["n_positive"] = int(pos.sum())
    xc, yc = cam_map[..., 0].astype(np.int64), cam_map[..., 1].astype(np.int64)  # (POISON is negative: it fails 0 < xc by itself)
    in_rect = pos & (xc > 0) & (xc < x_lim) & (yc > 0) & (yc < y_lim)
    st["n_in_rect"] = int(in_rect.sum())
    wh = v.dtype.type(W * H)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = wh * v  # (float32 * float32 or float64 * float64: the reference's W * H * cam_image[i, j])
    in_range = in_rect & (prod < wh)
    st["n_out_of_range"] = int((in_rect & ~in_range).sum())
    ii, jj = np.nonzero(in_range)
    if nc == 0 or ii.size == 0:
        return disp, st
    idx = prod[ii, jj].astype(np.int64)  # (truncation; all of them in [0, W * H))
    col, row = idx // H, idx % H
    ys = (row - nc)[:, None] + np.arange(2 * nc)[None, :]
    valid = (ys >= 0) & (ys < H)
    ent = proj_map[np.clip(ys, 0, H - 1), col[:, None]].astype(np.int64)  # [n][2 nc][2]
    bad = valid & ((ent[..., 0] == POISON) | (ent[..., 1] == POISON))
    poisoned = bad.any(1)
    st["n_poisoned"] = int(poisoned.sum())
    cost = np.where(valid, np.abs(yc[ii, jj][:, None] - ent[..., 1]), np.iinfo(np.int64).max)
    k = np.argmin(cost, axis=1)  # (the first minimum)
    n = np.arange(ii.size)
    d = ent[n, k, 0] - xc[ii, jj]
    ok = ~poisoned & (cost[n, k] <= max_row_diff) & (d > 0)
    disp[ii[ok], jj[ok]] = d[ok]
    return disp, st


def depth_from_disparity(disp, p1_03):
    d = np.asarray(disp).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = (np.float64(p1_03) / d.astype(np.float64)).astype(np.float32)
    depth[d == 0] = 0
    return depth


def mc3d(surface, cam_map, proj_map, p1_03, blur=True, **kw):
    """-> (depth f32, disparity u16, counts): the whole entry on one surface, as xm_mc3d_time_surfaces defines it (a disparity
    beyond 65535 is stored as 0 and counted)"""
    s = np.asarray(surface)
    v = median_blur3(s) if blur else s
    disp, st = search(v, cam_map, proj_map, **kw)
    st["n_nonzero"] = int((s != 0).sum())
    over = disp > 65535
    st["n_disp_overflow"] = int(over.sum())
    disp[over] = 0
    st["n_matched"] = int((disp > 0).sum())
    disp = disp.astype(np.uint16)
    return depth_from_disparity(disp, p1_03), disp, st
