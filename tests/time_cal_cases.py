"""The NumPy oracle of the projector time-map calibration (include/xmaps.h, "projector time-map calibration"; kernels in
x_maps_amd/csrc/xmaps_timecal.hpp) and the cases of its tests.  The reference ships no code for this step: the arithmetic here is
this build's definition, written elementwise in float64, every expression in the order the header gives.

  Oracle            accumulate (sequential acc = acc + ... per surface), mean / valid
  corners           core pixels, the four corners, the verdict (CornerError names the reason)
  homography        the 8 x 8 solve with h8 = 1
  warp, fill        per projector pixel; along each projector row
  render            camera pixels inside a quadrilateral observe a projector time function through the inverse homography

tests/test_time_cal_cases_cpu.py pins the oracle and asserts that each case reaches the loop bound it is named for;
tests/test_gpu_time_cal.py holds the device code to it bit for bit.
"""
import functools
import math

import numpy as np

BLOCK = 256            # threads per block of every kernel (xmaps_geometry.hpp)
RED_CHUNK = 8 * BLOCK  # pixels per block of k_surf_extrema / k_tcal_accumulate

CAM = (70, 50)         # 3 500 px: two reduction chunks
CAM_SMALL = (40, 28)   # 1 120 px: under one chunk
PROJ = (33, 47)        # under one wave per row
PROJ_SIZES = ((33, 47), (300, 5), (600, 3))  # fill trips per row at BLOCK = 256: 1, 2, 3
QUAD_AFFINE = ((8, 6), (58, 9), (60, 41), (10, 38))   # a parallelogram: TL, TR, BR, BL
QUAD_PERSP = ((9, 7), (57, 11), (62, 43), (6, 36))
QUAD_WIDE = ((5, 4), (61, 8), (66, 46), (2, 39))  # explicit corners beyond the seen area: missing runs at both ends of a row, empty rows
WIDE_MIN_COUNT = 7  # ... on the n9 case with this min_count, which also opens holes inside: missing runs between present pixels


class CornerError(ValueError):
    pass


# ---- accumulate, mean ------------------------------------------------------------------------------------------------------
def surface_extrema(s):
    d = np.asarray(s).astype(np.float64)
    nz = d != 0.0
    nnz = int(nz.sum())
    if nnz == 0:
        return math.inf, -math.inf, 0
    return float(d[nz].min()), float(d[nz].max()), nnz


class Oracle:
    def __init__(self, cam_size):
        self.w, self.h = cam_size
        self.reset()

    def reset(self):
        self.sum = np.zeros((self.h, self.w), np.float64)
        self.cnt = np.zeros((self.h, self.w), np.uint32)
        self.n_added = self.n_skipped = 0

    def add(self, surfaces):
        for s in surfaces:
            self.n_added += 1
            lo, hi, nnz = surface_extrema(s)
            if not (nnz != 0 and hi > lo):
                self.n_skipped += 1
                continue
            d = np.asarray(s).astype(np.float64)
            nz = d != 0.0
            vn = (d - lo) / (hi - lo)
            vn = np.where(vn < 0.0, 0.0, vn)
            self.sum = self.sum + np.where(nz, vn, 0.0)  # (x + 0.0 == x for every x >= 0 in the accumulator)
            self.cnt = self.cnt + nz.astype(np.uint32)

    @property
    def n_used(self):
        return self.n_added - self.n_skipped

    def mean(self, min_count):
        assert min_count >= 1
        valid = self.cnt >= min_count
        mean = np.zeros_like(self.sum)
        mean[valid] = self.sum[valid] / self.cnt[valid].astype(np.float64)
        return mean, valid


def min_count_for(min_share, n_used):
    """max(1, ceil(min_share * n_used)) (TimeMapCalibrator.mean)"""
    return max(1, int(math.ceil(min_share * n_used)))


# ---- corners ---------------------------------------------------------------------------------------------------------------
def core_mask(valid):
    v = np.asarray(valid, bool)
    h, w = v.shape
    core = np.zeros_like(v)
    if h >= 3 and w >= 3:
        c = np.ones((h - 2, w - 2), bool)
        for dy in range(3):
            for dx in range(3):
                c &= v[dy:dy + h - 2, dx:dx + w - 2]
        core[1:-1, 1:-1] = c
    return core


def corner_verdict(corners):
    """distinct and strictly convex in the order TL -> TR -> BR -> BL (integer cross products of consecutive edges)"""
    c = [(int(x), int(y)) for x, y in corners]
    for a in range(4):
        for b in range(a + 1, 4):
            if c[a] == c[b]:
                raise CornerError(f"two corners coincide at {c[a]}")
    cross = []
    for k in range(4):
        p, q, r = c[k], c[(k + 1) % 4], c[(k + 2) % 4]
        cross.append((q[0] - p[0]) * (r[1] - q[1]) - (q[1] - p[1]) * (r[0] - q[0]))
    if not (all(v > 0 for v in cross) or all(v < 0 for v in cross)):
        raise CornerError("the corner quadrilateral is not strictly convex")


def find_corners(valid, check=True):
    """(n_valid, n_core, corners [4][2] int or None).  CornerError when check and the verdict fails."""
    v = np.asarray(valid, bool)
    core = core_mask(v)
    n_valid, n_core = int(v.sum()), int(core.sum())
    if n_core == 0:
        if check:
            raise CornerError("no core pixel")
        return n_valid, 0, None
    ys, xs = np.nonzero(core)  # raster order: np.argmin / argmax return the first = the smallest raster index
    xs, ys = xs.astype(np.int64), ys.astype(np.int64)
    picks = (np.argmin(xs + ys), np.argmax(xs - ys), np.argmax(xs + ys), np.argmin(xs - ys))
    corners = [(int(xs[i]), int(ys[i])) for i in picks]
    if check:
        corner_verdict(corners)
    return n_valid, n_core, corners


# ---- homography ------------------------------------------------------------------------------------------------------------
SYMMETRIES = ((0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (1, 0, 3, 2), (0, 3, 2, 1), (3, 2, 1, 0), (2, 1, 0, 3))


def homography(src, dst):
    """h[9] (h8 = 1) with dst ~ h (src, 1) for four point pairs: the usual 8 x 8 system through np.linalg.solve"""
    A = np.zeros((8, 8), np.float64)
    b = np.zeros(8, np.float64)
    for i, ((u, v), (x, y)) in enumerate(zip(src, dst)):
        u, v, x, y = float(u), float(v), float(x), float(y)
        A[2 * i] = (u, v, 1.0, 0.0, 0.0, 0.0, -u * x, -v * x)
        A[2 * i + 1] = (0.0, 0.0, 0.0, u, v, 1.0, -u * y, -v * y)
        b[2 * i], b[2 * i + 1] = x, y
    return np.concatenate((np.linalg.solve(A, b), (1.0,)))


def proj_to_cam(proj_size, corners, corner_order=0):
    W, H = proj_size
    src = ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))
    return homography(src, [corners[k] for k in SYMMETRIES[corner_order]])


# ---- warp ------------------------------------------------------------------------------------------------------------------
def warp(mean, valid, h, proj_size):
    """(value f64 [H][W], present bool [H][W])"""
    W, H = proj_size
    mean, valid = np.asarray(mean, np.float64), np.asarray(valid, bool)
    ch, cw = mean.shape
    h = np.asarray(h, np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        X = h[0] * u + h[1] * v + h[2]
        Y = h[3] * u + h[4] * v + h[5]
        D = h[6] * u + h[7] * v + h[8]
        x, y = X / D, Y / D
        inside = (x > -1.0) & (x < float(cw)) & (y > -1.0) & (y < float(ch))  # (NaN fails)
        xs, ys = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
        xf, yf = np.floor(xs), np.floor(ys)
        fx, fy = xs - xf, ys - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        den = np.zeros((H, W), np.float64)
        num = np.zeros((H, W), np.float64)
        taps = ((x0, y0, (1.0 - fx) * (1.0 - fy)), (x0 + 1, y0, fx * (1.0 - fy)), (x0, y0 + 1, (1.0 - fx) * fy), (x0 + 1, y0 + 1, fx * fy))
        for tx, ty, wgt in taps:
            ok = inside & (tx >= 0) & (tx < cw) & (ty >= 0) & (ty < ch)
            cx, cy = np.where(ok, tx, 0), np.where(ok, ty, 0)
            ok = ok & valid[cy, cx]
            wt = np.where(ok, wgt, 0.0)
            m = np.where(ok, mean[cy, cx], 0.0)
            den = den + wt
            num = num + wt * m
        present = den > 0.0
        value = np.where(present, num / np.where(present, den, 1.0), 0.0)
    return value, present


def taps_valid(valid, h, proj_size):
    """per projector pixel, how many of the four taps are inside and valid (the tests' classification of interior / partial)"""
    W, H = proj_size
    valid = np.asarray(valid, bool)
    ch, cw = valid.shape
    h = np.asarray(h, np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    with np.errstate(all="ignore"):
        D = h[6] * u + h[7] * v + h[8]
        x, y = (h[0] * u + h[1] * v + h[2]) / D, (h[3] * u + h[4] * v + h[5]) / D
    n = np.zeros((H, W), np.int64)
    inside = (x > -1.0) & (x < float(cw)) & (y > -1.0) & (y < float(ch))
    x0 = np.floor(np.where(inside, x, 0.0)).astype(np.int64)
    y0 = np.floor(np.where(inside, y, 0.0)).astype(np.int64)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        tx, ty = x0 + dx, y0 + dy
        ok = inside & (tx >= 0) & (tx < cw) & (ty >= 0) & (ty < ch)
        n += ok & valid[np.where(ok, ty, 0), np.where(ok, tx, 0)]
    return n, x, y


# ---- fill ------------------------------------------------------------------------------------------------------------------
def fill(value, present):
    """(float32 map, n_missing, n_unfilled): along each row, as the header writes it"""
    value, present = np.asarray(value, np.float64), np.asarray(present, bool)
    H, W = value.shape
    out = np.zeros((H, W), np.float64)
    n_unfilled = 0
    for r in range(H):
        cols = np.nonzero(present[r])[0]
        if len(cols) == 0:
            n_unfilled += 1
            continue
        for u in range(W):
            if present[r, u]:
                out[r, u] = value[r, u]
                continue
            left, right = cols[cols < u], cols[cols > u]
            if len(left) and len(right):
                ul, ur = int(left[-1]), int(right[0])
                ml, mr = value[r, ul], value[r, ur]
                out[r, u] = ml + (mr - ml) * (np.float64(u - ul) / np.float64(ur - ul))
            elif len(left):
                out[r, u] = value[r, int(left[-1])]
            else:
                out[r, u] = value[r, int(right[0])]
    return out.astype(np.float32), int((~present).sum()), n_unfilled


def solve(oracle, min_count, proj_size, corners=None, corner_order=0):
    """the whole chain on an Oracle's accumulators: a dict of every stage's result"""
    mean, valid = oracle.mean(min_count)
    n_valid, n_core, found = find_corners(valid, check=corners is None)
    use = found if corners is None else corners
    h = proj_to_cam(proj_size, use, corner_order)
    value, present = warp(mean, valid, h, proj_size)
    time_map, n_missing, n_unfilled = fill(value, present)
    return dict(mean=mean, valid=valid, n_valid=n_valid, n_core=n_core, corners=found, h=h, value=value, present=present,
                time_map=time_map, n_missing=n_missing, n_unfilled=n_unfilled)


@functools.lru_cache(maxsize=None)
def solved(name, min_count, proj_size, corners=None, corner_order=0):
    """solve() on a named accumulate case, computed once and shared (read-only by convention)"""
    return solve(accumulated(name), min_count, proj_size, corners, corner_order)


# ---- the renderer ----------------------------------------------------------------------------------------------------------
def linear_time(proj_size):
    W, H = proj_size
    return lambda u, v: (u * H + v) / (W * H)


def curved_time(proj_size):
    """a non-linear scan: what a calibration is for"""
    W, H = proj_size
    return lambda u, v: ((u * H + v) / (W * H)) ** 1.3


def render(cam_size, proj_size, quad, time_fn, n, *, dtype=np.float64, bases=None, span=1000.0, drop=0.0, seed=0):
    """n camera time surfaces [n][cam_h][cam_w]: a camera pixel (x, y) inside `quad` sees projector position (u, v) = inv(h)(x, y)
    and is stamped base_k + 1 + t(u, v) * span; `drop` = share of the seen pixels that lose their event (per surface, seeded)"""
    cw, ch = cam_size
    W, H = proj_size
    hinv = np.linalg.inv(proj_to_cam(proj_size, quad).reshape(3, 3))
    x, y = np.meshgrid(np.arange(cw, dtype=np.float64), np.arange(ch, dtype=np.float64))
    d = hinv[2, 0] * x + hinv[2, 1] * y + hinv[2, 2]
    u, v = (hinv[0, 0] * x + hinv[0, 1] * y + hinv[0, 2]) / d, (hinv[1, 0] * x + hinv[1, 1] * y + hinv[1, 2]) / d
    eps = 1e-9
    seen = (u >= -eps) & (u <= W - 1 + eps) & (v >= -eps) & (v <= H - 1 + eps)
    t = time_fn(np.clip(u, 0, W - 1), np.clip(v, 0, H - 1))
    rng = np.random.default_rng(seed)
    out = np.zeros((n, ch, cw), np.float64)
    for k in range(n):
        base = 0.0 if bases is None else float(bases[k])
        keep = seen if drop == 0.0 else seen & (rng.random((ch, cw)) >= drop)
        out[k] = np.where(keep, base + 1.0 + t * span, 0.0)
    return out.astype(dtype)


def diagonal_time(proj_size):
    """a sweep along the projector's diagonal: neighbouring camera pixels differ by a small step of t in both directions, so a
    rendered frame has no pause inside (the trigger finder cuts at gaps of 40 us)"""
    W, H = proj_size
    return lambda u, v: (u / (W - 1) + v / (H - 1)) / 2.0


def events_from_surface(surface, t0):
    """one frame of EventCD records, time-sorted: every non-zero pixel fires once at t0 + rint(stamp)"""
    from x_maps_amd.synthetic import EVENT_CD_DTYPE
    ys, xs = np.nonzero(surface)
    t = t0 + np.rint(np.asarray(surface, np.float64)[ys, xs]).astype(np.int64)
    order = np.argsort(t, kind="stable")
    evs = np.zeros(len(order), EVENT_CD_DTYPE)
    evs["x"], evs["y"], evs["t"], evs["p"] = xs[order], ys[order], t[order], 1
    return evs


# ---- the cases -------------------------------------------------------------------------------------------------------------
GROUPINGS = {"one": (9,), "4+5": (4, 5), "nine": (1,) * 9}


@functools.lru_cache(maxsize=None)
def surfaces(name):
    """the accumulate cases: name -> surfaces [n][h][w] (read-only)"""
    if name in ("n1", "n3", "n9"):
        n = int(name[1:])
        s = render(CAM, PROJ, QUAD_PERSP, curved_time(PROJ), n, bases=[1000.0 * k for k in range(n)], drop=0.3 if n > 1 else 0.0, seed=n)
    elif name == "n9_f32":
        s = render(CAM, PROJ, QUAD_PERSP, curved_time(PROJ), 9, dtype=np.float32, bases=[1000.0 * k for k in range(9)], drop=0.3, seed=9)
    elif name == "small":
        s = render(CAM_SMALL, PROJ, ((4, 3), (34, 5), (36, 24), (3, 22)), curved_time(PROJ), 3, drop=0.2, seed=5)
    elif name == "skipped":  # an all-zero surface and a single-valued one in the middle of a group
        s = render(CAM, PROJ, QUAD_PERSP, curved_time(PROJ), 5, drop=0.2, seed=7).copy()
        s[1] = 0.0
        s[3] = np.where(s[3] != 0.0, 17.0, 0.0)
    elif name == "affine":   # noise-free, the linear time map through a parallelogram
        s = render(CAM, PROJ, QUAD_AFFINE, linear_time(PROJ), 2)
    elif name == "persp":    # the same through a perspective quadrilateral
        s = render(CAM, PROJ, QUAD_PERSP, linear_time(PROJ), 2)
    else:
        raise KeyError(name)
    s.setflags(write=False)
    return s


def accumulated(name, sizes=None):
    s = surfaces(name)
    o = Oracle((s.shape[2], s.shape[1]))
    k = 0
    for n in sizes or (len(s),):
        o.add(s[k:k + n])
        k += n
    assert k == len(s)
    return o


def _mask(size, fn):
    w, h = size
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    return fn(x, y)


@functools.lru_cache(maxsize=None)
def corner_masks():
    """name -> (valid mask, expected corners or the CornerError's word)"""
    m = {
        # an axis-aligned rectangle: TL and BR are unique, x - y ties along nothing but every edge ties elsewhere (TR / BL are
        # decided by the score alone, the raster rule by the rows of equal x + y inside)
        "rectangle": (_mask(CAM, lambda x, y: (x >= 10) & (x <= 50) & (y >= 8) & (y <= 40)), ((11, 9), (49, 9), (49, 39), (11, 39))),
        # a diamond-like quadrilateral whose top-left edge runs along x + y = const: two (and more) core pixels share the minimum
        "diamond": (_mask(CAM, lambda x, y: (x + y >= 30) & (x + y <= 80) & (x - y >= -10) & (x - y <= 28) & (y >= 4) & (y <= 45)), None),
        "two_wide": (_mask(CAM, lambda x, y: (x >= 20) & (x <= 21) & (y >= 5) & (y <= 40)), "no core pixel"),
        "blob3": (_mask(CAM, lambda x, y: (abs(x - 30) <= 1) & (abs(y - 20) <= 1)), "coincide"),
    }
    for v in m.values():
        v[0].setflags(write=False)
    return m


NON_CONVEX = ((10, 10), (30, 25), (50, 12), (30, 40))  # TL -> TR -> BR -> BL with TR pushed inside: a dart


@functools.lru_cache(maxsize=None)
def fill_rows():
    """a hand-built present mask and values, one row per fill case, 300 columns (two chunks at BLOCK = 256)"""
    W = 300
    names = ("start", "end", "boundary", "alternating", "full", "empty")
    present = np.ones((len(names), W), bool)
    present[0, :7] = False          # a missing run at the row's start
    present[1, W - 9:] = False      # ... at its end
    present[2, 250:263] = False     # a run across the chunk boundary at 256
    present[3, 1::2] = False        # alternating, the row's last pixel missing
    present[5, :] = False           # fully missing
    rng = np.random.default_rng(3)
    value = np.where(present, rng.random((len(names), W)), 0.0)
    value.setflags(write=False)
    present.setflags(write=False)
    return names, value, present


def warp_probe():
    """mean / valid on CAM_SMALL (one invalid pixel inside) for the warp positions below"""
    cw, ch = CAM_SMALL
    rng = np.random.default_rng(11)
    valid = np.ones((ch, cw), bool)
    valid[5, 7] = False
    mean = np.where(valid, rng.random((ch, cw)), 0.0)
    return mean, valid


WARP_PROBE_SIZE = (5, 4)
# name -> h for a 5 x 4 projector on CAM_SMALL (40 x 28)
WARP_PROBES = {
    "centre": (1.0, 0.0, 5.0, 0.0, 1.0, 4.0, 0.0, 0.0, 1.0),       # every pixel on a pixel centre: fx = fy = 0, three taps of weight 0
    "last": (1.0, 0.0, 35.0, 0.0, 1.0, 24.0, 0.0, 0.0, 1.0),       # u = 4 -> x = 39, v = 3 -> y = 27: the +1 taps are outside
    "outside": (1.0, 0.0, 37.5, 0.0, 1.0, 25.5, 0.0, 0.0, 1.0),    # x = 39.5 has two taps outside, x >= 40.5 is outside altogether
    "before": (1.0, 0.0, -1.5, 0.0, 1.0, -0.5, 0.0, 0.0, 1.0),     # x = -1.5: outside; x = -0.5: only the +1 taps are inside
    "d_zero": (1.0, 0.0, 5.0, 0.0, 1.0, 4.0, 1.0, 0.0, -2.0),      # D = u - 2: 0 at u = 2 (inf, and NaN where X = 0 too), negative before
    "nan": (1.0, 0.0, -2.0, 0.0, 1.0, 4.0, 1.0, 0.0, -2.0),        # X = D = 0 at u = 2: 0 / 0
    "half": (0.5, 0.25, 6.0, 0.25, 0.5, 4.5, 0.0, 0.0, 1.0),       # fractions, the invalid pixel (7, 5) among the taps
}
ARBITRARY_H = (1.31, -0.12, 9.3, 0.21, 0.61, 6.8, 1.1e-3, -7e-4, 1.0)  # not a solve of anything: on the n9 mean, projector 33 x 47
