"""Event frames at the borders of K1's time-stamp domain -- cases only, no tests (tests/test_stamp_edge_cases_cpu.py proves on
the oracle alone that they are what they claim; tests/test_gpu_stamp_edges.py runs them through every K1 family).

The hot path is compared with the NumPy oracle mostly on one kind of stamp: int64, a frame of a few thousand microseconds, a base
below 2^40.  The code has branches for everything else:

  * TimeNorm<long long> (csrc/xmaps_common.hpp) takes column_fast only while tmax - tmin <= 0xffffffff and t - tmin fits 32 bits;
    column_exact otherwise -- and past 2^53 the (double)(t - tmin) it starts from rounds;
  * the column tiles and the owner tiles carry a = t - tmin in 32 bits: the boundary pass writes "K1 objects" for a span
    >= 0xffffffff (xmaps_k1cols.hpp, cols_bounds_body), both tile kernels test the high word of a per event, and
    xm_debug_cols_thresholds refuses such a span;
  * the tiled K1, K0 and the one-thread-per-event K1 exist for float and double stamps, with and without a polarity column, in both
    views, and the verified-sorted shortcut with the compact key frame carries no type condition (host/xm_plan.hpp).

Rigs: S.C_TINY (64 x 48 camera, X-map 132 rows x 64 time columns, t_px_scale 63), the smallest on which the direct kernel, the
tiled K1 on 64-bit keys, the compact key frame of either view and the column tiles are all taken; S.make_tables_shared_cells()
with S.C_SHARED for the owner tiles.  Event counts: N_SPARSE (one thread per event), N_DENSE (tiled_path needs
(w_ts - 1.5) n / xmap_w >= 1024: 3.5 * 24 000 / 64 = 1312), N_RAGGED (the tiled kernel's last block partial), N_SHARED, and
N_SHARED_CAPTURED for the captured group on the owner tiles (see there).

Generators, all from the stamps t of S.make_events(...), rel = t - t[0], span0 = rel[-1]:

  stretch(span, t0)   t0 + rel * span // span0 in Python integers (sorted; first stamp t0, last t0 + span).  SPANS: on both sides
                      of 0xffffffff (2^32 - 2 is the largest the tiles accept), 2^40, on both sides of 2^53, 2^62, 2^63 - 1,
                      with zero, small, and negative bases.
  probes(span, t0)    the stretched stream plus, for every column c = 1 .. S, three events at a0 - 1, a0, a0 + 1 (clipped to
                      [0, span]) around a0 = floor((c - 1/2) span / S) in exact integer arithmetic -- the column boundary: an
                      off-by-one in a threshold or a conversion moves one of them to another column.  Where a step of one
                      microsecond is below what float64 resolves (spans from PROBE_WIDE_FROM on: a / span * S moves by S / span
                      per microsecond, its rounding error is about c 2^-52), two more at a0 -+ probe_width(span), which do
                      straddle the boundary.  Past 2^53 also stamps at offsets 2^53 + 1 and 2^53 + 3: odd, float64 cannot hold
                      them.  Merged into the stream and re-sorted (stable).
  one_wild(k)         the plain short frame with event k moved 2^34 us ahead (one wild TIME_HIGH word): k in the middle leaves
                      the stream unsorted, k = n - 1 leaves it sorted with a span past 2^32.  The oracle keeps a handful of
                      inliers (every other event falls into column 0, which no X-map defines).
  equal(n)            all stamps equal: `degenerate` (0 / 0 -> column 0 for every event).
  float cases         float64 / float32: normalised (0, 1] values in raster order (the reference's evaluation caller; unsorted),
                      2^53 + 2 rel as float64, 2^24 + 2 rel as float32 (sorted, exact, ties), 2^20 + rel as float32 (sorted,
                      exact), and a negative base for each type.

Out of scope: spans whose tmax - tmin overflows int64 -- the reference's NumPy wraps there, there is nothing to agree with --, and
NaN / inf stamps."""
from __future__ import annotations

import functools

import numpy as np

import xmaps_oracle as O
from x_maps_amd import synthetic as S

N_SPARSE, N_DENSE, N_RAGGED, N_SHARED = 2_000, 24_000, 24_001, 40_000
# A captured group takes the tiles only where the group is dense enough for the tiled K1 as well (frame_path, xm_plan.hpp: `!p.direct`,
# i.e. batch_path -> tiled_path: 3.5 n / xmap_w >= 1024): its redo runs there.  On C-shared (270 time columns) that is n >= 78 994.
N_SHARED_CAPTURED = 80_000

# (span, t0) of stretch / probes
SPANS = [(2 ** 32 - 2, 0), (2 ** 32 - 1, 7), (2 ** 32, 7), (2 ** 32 + 1, -5), (2 ** 40, 123), (2 ** 53 + 2, 1),
         (2 ** 62, -2 ** 61), (2 ** 63 - 1, -2 ** 62)]
TILE_SPAN_MAX = 2 ** 32 - 2  # the largest span the column / owner tiles accept (a = t - tmin and span + 1 in 32 bits)
WILD_US = 2 ** 34
# a / span * S changes by S / span per microsecond; computed in float64 it is off by up to ~S 2^-52.  One microsecond decides the
# column while S / span >> S 2^-52; from 2^46 us on the probes get a second, wider pair
PROBE_WIDE_FROM = 2 ** 46


def probe_width(span: int) -> int:
    return span >> 44  # 2^-44 of the span: sixteen times the rounding error's bound, a 2^-38-th of a column at S = 63


def rig(name: str):
    """(RigConfig, tables) of 'tiny' / 'shared'"""
    return _rig(name)


@functools.lru_cache(maxsize=None)
def _rig(name):
    if name == "tiny":
        return S.C_TINY, S.make_tables(S.C_TINY)
    if name == "shared":
        return S.C_SHARED, S.make_tables_shared_cells(S.C_SHARED)
    raise KeyError(name)


def base_events(cfg, n: int, frame: int = 0) -> np.ndarray:
    """the plain short frame: sorted int64 stamps over a 13 ms scan; first and last event pinned to the scan's ends so that
    span0 does not depend on the draw"""
    evs = S.make_events(cfg, frame=700 + frame, n=n)
    evs["t"][-1] = evs["t"][0] + 12_999
    return evs


def _rel(evs):
    t = evs["t"].astype(np.int64)
    return [int(v) for v in (t - t[0])]


def stretch(evs: np.ndarray, span: int, t0: int) -> np.ndarray:
    rel = _rel(evs)
    span0 = rel[-1]
    out = evs.copy()
    out["t"] = np.array([t0 + r * span // span0 for r in rel], dtype=np.int64)
    return out


def probe_offsets(span: int, scale: int) -> list:
    """[(c, [a ...])] for c = 1 .. scale: the offsets a = t - tmin of column c's probes"""
    out = []
    w = probe_width(span) if span >= PROBE_WIDE_FROM else 0
    for c in range(1, scale + 1):
        a0 = (2 * c - 1) * span // (2 * scale)
        offs = [a0 - 1, a0, a0 + 1] + ([a0 - w, a0 + w] if w else [])
        out.append((c, [min(max(a, 0), span) for a in offs]))
    return out


def probes(evs: np.ndarray, span: int, t0: int, cfg, scale: int) -> np.ndarray:
    """the stretched stream with the probe events merged in; a probe sits at the camera column the scan has reached at its time
    (so that it is an inlier like its neighbours) and at a row of its own"""
    base = stretch(evs, span, t0)
    offs = [a for _, aa in probe_offsets(span, scale) for a in aa]
    offs += [a for a in (2 ** 53 + 1, 2 ** 53 + 3) if a < span]
    extra = np.zeros(len(offs), S.EVENT_CD_DTYPE)
    extra["t"] = np.array([t0 + a for a in offs], dtype=np.int64)
    extra["x"] = [min(a * cfg.cam_w // span, cfg.cam_w - 1) for a in offs]
    extra["y"] = [(5 * i + 3) % cfg.cam_h for i in range(len(offs))]
    extra["p"] = 1
    out = np.zeros(len(base) + len(extra), S.EVENT_CD_DTYPE)
    out[:len(base)], out[len(base):] = base, extra
    return out[np.argsort(out["t"], kind="stable")]


def one_wild(evs: np.ndarray, k: int) -> np.ndarray:
    out = evs.copy()
    out["t"][k] += WILD_US
    return out


def equal(evs: np.ndarray) -> np.ndarray:
    out = evs.copy()
    out["t"] = out["t"][0]
    return out


def span_name(span: int, t0: int) -> str:
    for e in (32, 40, 53, 62, 63):
        d = span - 2 ** e
        if abs(d) <= 3:
            return f"2^{e}{d:+d}@{t0}" if d else f"2^{e}@{t0}"
    return f"{span}@{t0}"


@functools.lru_cache(maxsize=None)
def int64_cases(rig_name: str, n: int, frame: int = 0):
    """the full list of sorted int64 frames: [(name, span, EventCD array)] -- every span stretched, then every span with probes"""
    cfg, tb = rig(rig_name)
    evs = base_events(cfg, n, frame)
    out = [(f"stretch {span_name(s, t0)}", s, stretch(evs, s, t0)) for s, t0 in SPANS]
    out += [(f"probes {span_name(s, t0)}", s, probes(evs, s, t0, cfg, tb["t_px_scale"])) for s, t0 in SPANS]
    return out


@functools.lru_cache(maxsize=None)
def group_frames(rig_name: str, n: int):
    """three frames for one group: a short one, one at the tiles' largest span, one past it (different draws)"""
    cfg, _ = rig(rig_name)
    return [base_events(cfg, n, 1), stretch(base_events(cfg, n, 2), TILE_SPAN_MAX, 11), stretch(base_events(cfg, n, 3), 2 ** 32 + 1, -5)]


@functools.lru_cache(maxsize=None)
def wild_frames(rig_name: str, n: int):
    """{'middle': unsorted, 'last': sorted with a span past 2^32}"""
    cfg, _ = rig(rig_name)
    evs = base_events(cfg, n, 4)
    return {"middle": one_wild(evs, n // 2), "last": one_wild(evs, n - 1)}


# ---- float stamps ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_cases(rig_name: str, n: int, kind: str):
    """kind 'float64' / 'float32' -> [(name, sorted?, x u16, y u16, t float64 holding values the kind represents exactly)].
    The frames are handed over as t.astype(kind)."""
    cfg, _ = rig(rig_name)
    evs = base_events(cfg, n, 5)
    x, y, t, _ = S.to_soa(evs)
    rel = (t - t[0]).astype(np.float64)
    raster = np.lexsort((x, y))  # row by row, as np.argwhere walks a time surface
    norm = (rel + 1.0) / (rel[-1] + 1.0)  # (0, 1], the largest exactly 1
    if kind == "float32":
        norm = norm.astype(np.float32).astype(np.float64)  # (the evaluation caller's f32 surface: rounded once, here)
        big, neg = 2.0 ** 24 + 2.0 * rel, -(2.0 ** 24) + 2.0 * rel
    else:
        big, neg = 2.0 ** 53 + 2.0 * rel, -(2.0 ** 53) + 2.0 * rel
    out = [("normalised raster", False, x[raster], y[raster], norm[raster]),
           ("big base", True, x, y, big),
           ("negative base", True, x, y, neg)]
    if kind == "float32":
        out.append(("2^20 + rel", True, x, y, 2.0 ** 20 + rel))
    return out


# ---- the oracle, once per frame -------------------------------------------------------------------------------------------------
_refs = {}


def ref(rig_name: str, key, x, y, t, camera: bool = False):
    """O.process_ev_frame of the frame, computed once per (rig, key, view) and shared (callers must not write into it)"""
    k = (rig_name, key, bool(camera))
    if k not in _refs:
        _, tb = rig(rig_name)
        _refs[k] = O.process_ev_frame(tb, np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64), t, camera_perspective=camera)
    return _refs[k]


def ref_events(rig_name: str, key, evs, camera: bool = False):
    x, y, t, _ = S.to_soa(evs)
    return ref(rig_name, key, x, y, t, camera)
