"""What the frame -> point cloud tests share: the definition as a composition of oracle.xmaps_oracle functions, the rig, and the
frames every GPU test runs.

The definition (include/xmaps.h, xm_frames_to_point_clouds): with use_polarity only events with p == 1 exist; (t_min, t_max) are
taken over all existing events; an existing event off the sensor is left out and counted in n_index_errors; every other existing
event goes through rectify_cam_coords_i16 and compute_disparity; the cloud is construct_point_cloud(xr_f32[mask], yr_f32[mask],
disparity) -- one row per inlier event in stream order.  An empty frame: no rows, zero statistics.

compute_disparity takes its extrema from the stamps it is given.  The frame's extrema also cover the events that were left out, so
the oracle hands them through as two further entries whose rectified row is -1: the row mask (xmd:23) drops them before anything
is gathered, and their two mask entries are cut off again.  tests/test_frame_cloud_cases_cpu.py holds the composition against a
per-event Python loop."""
import numpy as np

import xmaps_oracle as O
from x_maps_amd import synthetic as S

CAM_W, CAM_H = 70, 37  # as tests/frame_surface_cases.py: 2 590 cells, no multiple of 64
CHUNK = 1024           # events per block and trip of the per-event passes (csrc/xmaps_framecloud.hpp: FC_CHUNK)
WAVE = 64              # events per inlier count
STAT_FIELDS = ("n_events", "n_inliers", "n_index_errors", "t_min", "t_max")


def add_cloud_tables(tb, seed=17):
    """tables + float rectify maps (the int16 maps plus a seeded sub-pixel offset) and a plausible Q (a rectified pair with equal
    principal points, as stereoRectify's CALIB_ZERO_DISPARITY gives: focal length 80 px, baseline 0.11 m -- so w == 0 at
    disparity 0: the reference's inf / nan row)"""
    tb = dict(tb)
    rng = np.random.default_rng(seed)
    shape = np.asarray(tb["cam_mapx_i16"]).shape
    tb["cam_mapx_f32"] = (tb["cam_mapx_i16"] + rng.uniform(-0.5, 0.5, shape)).astype(np.float32)
    tb["cam_mapy_f32"] = (tb["cam_mapy_i16"] + rng.uniform(-0.5, 0.5, shape)).astype(np.float32)
    f, cx, cy, base = 80.0, 95.3, 50.7, 0.11
    tb["Q"] = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1 / base, 0]], np.float64)
    return tb


def rig_tables(cam_w=CAM_W, cam_h=CAM_H, seed=17):
    """the synthetic rig with a cam_w x cam_h camera (projector 64 x 48) and add_cloud_tables' maps and Q"""
    return add_cloud_tables(S.make_tables(S.RigConfig(f"C-{cam_w}x{cam_h}", cam_w, cam_h, 64, 48, 0)), seed)


def disparity_with_extrema(tb, x, y, t, t_min, t_max):
    """(disp[M] int16 compacted, mask[N]) of on-sensor events under the given frame extrema (see the module text)"""
    xr, yr = O.rectify_cam_coords_i16(tb["cam_mapx_i16"], tb["cam_mapy_i16"], x, y)
    xr2 = np.concatenate([xr, np.zeros(2, np.int16)])
    yr2 = np.concatenate([yr, np.full(2, -1, np.int16)])
    t2 = np.concatenate([np.asarray(t, np.int64), np.array([t_min, t_max], np.int64)])
    disp, mask = O.compute_disparity(xr2, yr2, t2, tb["proj_x_map"], tb["t_px_scale"], tb["x_offset"])
    assert not mask[-2:].any()
    return disp, mask[:-2]


def oracle(tb, evs, use_polarity=False):
    """one frame of EventCD records -> dict(cloud f32 [n_inliers][3], stats, and what the cloud was made of: on (existing events
    on the sensor, among the existing), mask (inliers among those), disp (int16, compacted), xr_f / yr_f (compacted))"""
    cam_w, cam_h = tb["cam_w"], tb["cam_h"]
    if use_polarity:
        evs = evs[evs["p"] == 1]
    stats = dict.fromkeys(STAT_FIELDS, 0)
    if len(evs) == 0:
        z = np.zeros(0, np.float32)
        return dict(cloud=np.zeros((0, 3), np.float32), stats=stats, on=np.zeros(0, bool), mask=np.zeros(0, bool), disp=np.zeros(0, np.int16),
                    xr_f=z, yr_f=z)
    t = evs["t"].astype(np.int64)
    t_min, t_max = int(t.min()), int(t.max())
    on = (evs["x"] < cam_w) & (evs["y"] < cam_h)
    x, y = evs["x"][on].astype(np.int64), evs["y"][on].astype(np.int64)
    disp, mask = disparity_with_extrema(tb, x, y, t[on], t_min, t_max)
    xr_f, yr_f = O.rectify_cam_coords_f32(tb["cam_mapx_f32"], tb["cam_mapy_f32"], x[mask], y[mask])
    cloud = O.construct_point_cloud(tb["Q"], xr_f, yr_f, disp.astype(np.float32))
    stats.update(n_events=len(evs), n_inliers=int(mask.sum()), n_index_errors=int((~on).sum()), t_min=t_min, t_max=t_max)
    return dict(cloud=cloud, stats=stats, on=on, mask=mask, disp=disp, xr_f=xr_f, yr_f=yr_f)


def oracle_loop(tb, evs, use_polarity=False):
    """the same by a plain loop over the events in stream order (the oracle's own check): (rows as a list of (xr_f, yr_f, disp),
    stats).  The rows' 3-D points are the business of construct_point_cloud, which the goldens pin."""
    cam_w, cam_h, S_, xo = tb["cam_w"], tb["cam_h"], tb["t_px_scale"], tb["x_offset"]
    X, mx, my = tb["proj_x_map"], tb["cam_mapx_i16"], tb["cam_mapy_i16"]
    ex = [e for e in evs if not use_polarity or int(e["p"]) == 1]
    stats = dict.fromkeys(STAT_FIELDS, 0)
    if not ex:
        return [], stats
    t_min, t_max = min(int(e["t"]) for e in ex), max(int(e["t"]) for e in ex)
    rows, left = [], 0
    for e in ex:
        x, y, t = int(e["x"]), int(e["y"]), int(e["t"])
        if x >= cam_w or y >= cam_h:
            left += 1
            continue
        xr, yr = int(mx[y, x]), int(my[y, x])
        if not 0 <= yr < X.shape[0] - 1:
            continue
        col = 0 if t_max == t_min else int(round(float(t - t_min) / float(t_max - t_min) * S_))  # (round: ties to even)
        d = (int(X[yr, col]) - xr - xo + 32768) % 65536 - 32768  # int16 wrap-around
        if d < 0:
            continue
        rows.append((float(tb["cam_mapx_f32"][y, x]), float(tb["cam_mapy_f32"][y, x]), d))
    stats.update(n_events=len(ex), n_inliers=len(rows), n_index_errors=left, t_min=t_min, t_max=t_max)
    return rows, stats


# ---- the frames ----------------------------------------------------------------------------------------------------------------
def _events(x, y, t, p=1):
    ev = np.zeros(len(t), S.EVENT_CD_DTYPE)
    ev["x"], ev["y"], ev["t"], ev["p"] = x, y, t, p
    return ev


def _random(rng, n, cam_w, cam_h, t0, span, sort=True):
    t = rng.integers(0, span + 1, n) + t0
    t[0], t[-1] = t0, t0 + span  # (the extrema do not depend on the draw)
    if sort:
        t.sort()
    return _events(rng.integers(0, cam_w, n), rng.integers(0, cam_h, n), t)


def _select(tb, rng, n, t0, span, want_inlier):
    """n events of a frame with extrema (t0, t0 + span), every one of them an inlier / none of them, in time order.
    An event that holds t_min lies in X-map column 0, which is undefined (0) on every rig the table builders make, so it is never
    an inlier: "every event an inlier" means every event but the frame's first, which holds t_min alone."""
    cam_w, cam_h = tb["cam_w"], tb["cam_h"]
    m = 40 * n
    x, y = rng.integers(0, cam_w, m), rng.integers(0, cam_h, m)
    t = rng.integers(0, span + 1, m) + t0
    _, mask = disparity_with_extrema(tb, x, y, t, t0, t0 + span)
    pick = np.flatnonzero(mask == want_inlier)
    assert len(pick) >= n
    # the two events that hold the extrema are of the wanted kind as well
    assert not disparity_with_extrema(tb, x, y, np.full(m, t0), t0, t0 + span)[1].any()
    lo = pick[0]
    hi = next(i for i in range(m) if disparity_with_extrema(tb, x[[i]], y[[i]], [t0 + span], t0, t0 + span)[1][0] == want_inlier)
    pick = pick[t[pick] > t0][:n]
    pick = pick[np.argsort(t[pick], kind="stable")]
    ev = _events(x[pick], y[pick], t[pick])
    ev[0] = _events([x[lo]], [y[lo]], [t0])[0]
    ev[-1] = _events([x[hi]], [y[hi]], [t0 + span])[0]
    return ev


def frames(tb=None, seed=23):
    """name -> frame, in the order of the group.  What each is for is asserted by tests/test_frame_cloud_cases_cpu.py."""
    tb = tb or rig_tables()
    cam_w, cam_h = tb["cam_w"], tb["cam_h"]
    rng = np.random.default_rng(seed)
    span = 13_000
    f = {}
    f["empty"] = _events([], [], [])
    f["single"] = _events([cam_w // 2], [cam_h // 2], [123_456_789])
    for n in (WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1):
        f[f"n{n}"] = ev = _random(rng, n, cam_w, cam_h, 1_000_000 * n, span)
        if n in (WAVE + 1, CHUNK + 1):  # the one event behind the boundary (it holds t_max) is an inlier: a row of its own wave / block
            ys, xs = np.mgrid[0:cam_h, 0:cam_w]
            _, mask = disparity_with_extrema(tb, xs.ravel(), ys.ravel(), np.full(cam_w * cam_h, ev["t"][-1]), ev["t"][0], ev["t"][-1])
            p = int(np.flatnonzero(mask)[len(ev) % 97])
            ev["x"][-1], ev["y"][-1] = p % cam_w, p // cam_w
    f["long"] = _random(rng, 3 * CHUNK + 500, cam_w, cam_h, 2_000_000, span)  # four chunks: two trips of two blocks under XM_FC_MAX_BLOCKS=2
    f["no_inlier"] = _select(tb, rng, 300, 3_000_000, span, False)
    f["all_inlier"] = _select(tb, rng, 300, 4_000_000, span, True)
    # events off the sensor, first and last in the frame among them; the first holds t_min, the last t_max
    out = _random(rng, 1200, cam_w, cam_h, 6_000_000, span)
    out["x"][0] = cam_w
    out["y"][400] = cam_h
    out["x"][800] = 65_535
    out["y"][801] = 65_535
    out["x"][1199], out["y"][1199] = 65_535, 65_535
    f["outside"] = out
    pol = _random(rng, 1300, cam_w, cam_h, 8_000_000, span)
    pol["p"] = rng.random(1300) >= 0.3
    pol["p"][0], pol["t"][0] = 0, 7_990_000  # a negative event holds the smallest t: the columns depend on use_polarity
    f["polarity"] = pol
    shuffled = _random(rng, 1500, cam_w, cam_h, 9_000_000, span, sort=False)
    shuffled["t"][0], shuffled["t"][777] = 9_006_000, 8_999_990  # the earliest event is not the first
    f["shuffled"] = shuffled
    f["equal_t"] = _events(rng.integers(0, cam_w, 900), rng.integers(0, cam_h, 900), np.full(900, 4_444_444))
    # exact .5 ties: span 128, t - t_min = 64 -> 64 / 128 * 63 = 31.5 exactly -> column 32 (to even)
    tie = _random(rng, 600, cam_w, cam_h, 10_000_000, 128)
    tie["t"][200:400] = 10_000_064
    f["tie"] = tie
    # rows with disparity 0: span 16 * 63, so that t0 + 16 c lies in column c; every (pixel, column) whose disparity is 0 once
    S_ = tb["t_px_scale"]
    d0 = _random(rng, 900, cam_w, cam_h, 11_000_000, 16 * S_)
    ys, xs = np.mgrid[0:cam_h, 0:cam_w]
    hits = []
    for c in range(S_ + 1):
        disp, mask = disparity_with_extrema(tb, xs.ravel(), ys.ravel(), np.full(cam_w * cam_h, 11_000_000 + 16 * c), 11_000_000, 11_000_000 + 16 * S_)
        full = np.full(cam_w * cam_h, -1)
        full[mask] = disp
        hits += [(int(p % cam_w), int(p // cam_w), 11_000_000 + 16 * c) for p in np.flatnonzero(full == 0)]
    hits = hits[:: max(1, len(hits) // 50)][:50]
    for k, (x, y, t) in enumerate(hits):
        d0[10 + 17 * k] = _events([x], [y], [t])[0]
    f["disp0"] = d0
    f["one_pixel"] = _events(np.full(700, cam_w // 2), np.full(700, cam_h // 2), np.sort(rng.integers(0, 9000, 700)) + 50_000)
    f["empty_between"] = _events([], [], [])
    f["after_empty"] = _random(rng, 2100, cam_w, cam_h, 12_000_000, span)
    return f


DENSE = ("n1023", "n1024", "n1025", "long", "outside", "polarity", "shuffled", "tie", "disp0", "after_empty")


def concat(frames, lead=0):
    """(the frames as one array of 16-byte records behind `lead` records that belong to nobody, their offsets): np.concatenate
    would hand back a packed 14-byte layout"""
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    offs += np.uint64(lead)
    evs = np.zeros(int(offs[-1]), S.EVENT_CD_DTYPE)
    evs["x"][:lead], evs["y"][:lead], evs["t"][:lead] = 1, 1, 77
    for f, a in zip(frames, offs[:-1]):
        evs[int(a):int(a) + len(f)] = f
    assert evs.itemsize == 16
    return evs, offs


def group(tb=None, seed=23):
    fr = frames(tb, seed)
    return list(fr), list(fr.values())


def group33(tb=None, seed=23):
    """33 frames, empties in between: two launch sequences (32 + 1)"""
    names, fr = group(tb, seed)
    order = [i % len(fr) for i in range(33)]
    assert sum(len(fr[i]) == 0 for i in order) >= 3 and len(fr[order[32]]) > 0
    return order
