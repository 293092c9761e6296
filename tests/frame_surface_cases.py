"""What the frame -> time surface tests share: the definition as a NumPy oracle, and the frames of the group every GPU test runs.

The definition (include/xmaps.h, xm_frames_to_time_surfaces): with use_polarity only events with p == 1 exist; an existing event
takes part iff x < cam_w and y < cam_h (the others are counted in n_index_errors); base = the smallest t over the existing events,
those left out included; per pixel the event with the largest ("last") or smallest ("first") INDEX in the frame is selected;
S[y][x] = t_selected - base + 1 in int64, converted once by astype; 0 = no event; t_span = the largest t - base over the existing
events.  An empty frame: zeros everywhere.

The oracle picks the winners explicitly, by np.maximum.at / np.minimum.at on event indices; it does not rely on the order in which
a fancy assignment with duplicate indices writes.  tests/test_frame_surface_cases_cpu.py holds it against a per-event Python loop."""
import numpy as np

from x_maps_amd import synthetic as S

CAM_W, CAM_H = 70, 37  # 2 590 cells: no multiple of 64 or 1024, three blocks of 1024 cells
SELECTS = ("last", "first")
STAT_FIELDS = ("n_events", "n_pixels", "n_index_errors", "t_base", "t_span")


def rig_tables(cam_w=CAM_W, cam_h=CAM_H):
    """the synthetic rig with a cam_w x cam_h camera (projector 64 x 48)"""
    return S.make_tables(S.RigConfig(f"C-{cam_w}x{cam_h}", cam_w, cam_h, 64, 48, 0))


def oracle(evs, cam_w, cam_h, select="last", dtype=np.float32, use_polarity=False):
    """(surface [cam_h][cam_w] of dtype, statistics as a dict of Python ints) of one frame of EventCD records"""
    assert select in SELECTS
    if use_polarity:
        evs = evs[evs["p"] == 1]
    stats = dict.fromkeys(STAT_FIELDS, 0)
    s64 = np.zeros(cam_h * cam_w, np.int64)
    if len(evs) == 0:
        return s64.reshape(cam_h, cam_w).astype(dtype), stats
    t = evs["t"].astype(np.int64)
    base = int(t.min())
    part = (evs["x"] < cam_w) & (evs["y"] < cam_h)
    idx = np.flatnonzero(part).astype(np.int64)
    cell = evs["y"][idx].astype(np.int64) * cam_w + evs["x"][idx].astype(np.int64)
    if select == "last":
        win = np.full(cam_h * cam_w, -1, np.int64)
        np.maximum.at(win, cell, idx)
        hit = win >= 0
    else:
        win = np.full(cam_h * cam_w, len(evs), np.int64)
        np.minimum.at(win, cell, idx)
        hit = win < len(evs)
    s64[hit] = t[win[hit]] - base + 1
    stats.update(n_events=len(evs), n_pixels=int(hit.sum()), n_index_errors=int((~part).sum()), t_base=base, t_span=int(t.max()) - base)
    return s64.reshape(cam_h, cam_w).astype(dtype), stats


def oracle_loop(evs, cam_w, cam_h, select="last", dtype=np.float32, use_polarity=False):
    """the same by a plain loop over the events in stream order (the oracle's own check)"""
    s64 = np.zeros((cam_h, cam_w), np.int64)
    seen = np.zeros((cam_h, cam_w), bool)
    n = n_left = 0
    base = t_max = None
    for e in evs:
        if use_polarity and int(e["p"]) != 1:
            continue
        t = int(e["t"])
        base = t if base is None else min(base, t)
        t_max = t if t_max is None else max(t_max, t)
        n += 1
    for e in evs:
        if use_polarity and int(e["p"]) != 1:
            continue
        x, y = int(e["x"]), int(e["y"])
        if x >= cam_w or y >= cam_h:
            n_left += 1
            continue
        if select == "first" and seen[y, x]:
            continue
        s64[y, x] = int(e["t"]) - base + 1
        seen[y, x] = True
    stats = dict.fromkeys(STAT_FIELDS, 0)
    if n:
        stats.update(n_events=n, n_pixels=int(seen.sum()), n_index_errors=n_left, t_base=base, t_span=t_max - base)
    return s64.astype(dtype), stats


# ---- the frames ----------------------------------------------------------------------------------------------------------------
def _events(x, y, t, p=1):
    ev = np.zeros(len(t), S.EVENT_CD_DTYPE)
    ev["x"], ev["y"], ev["t"], ev["p"] = x, y, t, p
    return ev


def _random(rng, n, cam_w, cam_h, t0, span, sort=True):
    t = rng.integers(0, span, n) + t0
    if sort:
        t.sort()
    return _events(rng.integers(0, cam_w, n), rng.integers(0, cam_h, n), t)


def frames(cam_w=CAM_W, cam_h=CAM_H, seed=5):
    """name -> frame, in the order of the group.  What each is for is asserted by tests/test_frame_surface_cases_cpu.py."""
    rng = np.random.default_rng(seed)
    cells = cam_w * cam_h
    f = {}
    f["empty"] = _events([], [], [])
    f["single"] = _events([cam_w - 1], [cam_h - 1], [123_456_789])
    f["long"] = _random(rng, 5000, cam_w, cam_h, 2_000_000, 13_000)  # five chunks of the event pass, about two events per cell
    f["one_pixel"] = _events(np.full(700, 3), np.full(700, 2), np.sort(rng.integers(0, 9000, 700)) + 50_000)
    # about 60 % duplicates: 2.5 x as many events as the cells they are drawn from
    dup_cells = rng.choice(cells, cells // 4, replace=False)
    c = rng.choice(dup_cells, int(2.5 * len(dup_cells)))
    f["duplicates"] = _events(c % cam_w, c // cam_w, np.sort(rng.integers(0, 13_000, len(c))) + 7_000_000)
    shuffled = _random(rng, 1500, cam_w, cam_h, 3_000_000, 13_000, sort=False)
    shuffled["t"][0], shuffled["t"][777] = 3_006_000, 2_999_990  # the earliest event is not the first
    f["shuffled"] = shuffled
    f["equal_t"] = _events(rng.integers(0, cam_w, 900), rng.integers(0, cam_h, 900), np.full(900, 4_444_444))
    # events outside the sensor: x == cam_w, y == cam_h, 65 535; the one at index 1 holds the frame's smallest t
    out = _random(rng, 1200, cam_w, cam_h, 6_000_000, 13_000)
    out["x"][1], out["t"][1] = cam_w, 5_999_000
    out["y"][400] = cam_h
    out["x"][800] = 65_535
    out["y"][801] = 65_535
    out["x"][1199], out["y"][1199] = 65_535, 65_535
    f["outside"] = out
    pol = _random(rng, 1300, cam_w, cam_h, 8_000_000, 13_000)
    pol["p"] = rng.random(1300) >= 0.3
    pol["p"][0], pol["t"][0] = 0, 7_990_000  # a negative event holds the smallest t: base depends on use_polarity
    f["polarity"] = pol
    # a span beyond 2^24 us: float32 rounds down, up, and an exact tie both ways (to even)
    big = _random(rng, 1100, cam_w, cam_h, 9_000_000, 13_000)
    base = 9_000_000
    big["t"][0], big["x"][0], big["y"][0] = base, 20, 5
    for k, d in enumerate(((1 << 24) + 1, (1 << 24) + 3, (1 << 24) + 2, (1 << 24) + 6, (1 << 25) + 2, (1 << 25) + 6, (1 << 26) + 12345,
                           (1 << 26) + 12351)):
        i = 1099 - k  # the frame's last events: each the last writer of a pixel of its own
        big["t"][i] = base + d - 1  # (S = t - base + 1 = d)
        big["x"][i], big["y"][i] = k, 0
    keep = np.ones(1100, bool)
    keep[:1092] = ~((big["y"][:1092] == 0) & (big["x"][:1092] < 8))  # (nobody else fires at those pixels: "first" sees them too)
    f["wide_span"] = big[keep]
    f["empty_between"] = _events([], [], [])
    f["after_empty"] = _random(rng, 2100, cam_w, cam_h, 11_000_000, 13_000)
    return f


def concat(frames):
    """(the frames as one array of 16-byte records, their offsets): np.concatenate would hand back a packed 14-byte layout"""
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    evs = np.zeros(int(offs[-1]), S.EVENT_CD_DTYPE)
    for f, a in zip(frames, offs[:-1]):
        evs[int(a):int(a) + len(f)] = f
    assert evs.itemsize == 16
    return evs, offs


def group(cam_w=CAM_W, cam_h=CAM_H, seed=5):
    fr = frames(cam_w, cam_h, seed)
    return list(fr), list(fr.values())
