"""NumPy restatement of the reference's four frame event filters (python/frame_event_filter.py:19-128) by explicit survivor
index -- the yardstick of the device ingest's frame-filter stage (tests/test_gpu_ingest_frame_filters.py), itself pinned against
the reference's own outputs (golden G5: tests/test_frame_filter_ref_cpu.py).

Per cell -- (y, x), or (y, xp) for FirstEventPerYT -- the event with the LAST index in the frame survives (what the reference
computes as it runs: x_maps_amd/frame_event_filter.py), with `intended` the FIRST.  The cells are written with NumPy's own fancy
indexing on maps of the reference's extents (max + 1), so a negative column wraps exactly as the reference's does and one that
is still out of range raises IndexError; time stamps go through int32 like the reference's maps; survivors come out in raster
order of the cells."""
import numpy as np

FIRST_PER_YT, FIRST_PER_XY, LAST_PER_XY, MEAN_PER_XY = 1, 2, 3, 4
BY_CLASS = {"FirstEventPerYTFilter": FIRST_PER_YT, "FirstEventPerXYFilter": FIRST_PER_XY, "LastEventPerXYFilter": LAST_PER_XY,
            "MeanFirstLastEventPerXYFilter": MEAN_PER_XY}


def survivor_maps(events, xp_i16, filter_id):
    """(last, first): per cell the largest / smallest index into the p == 1 events, -1 where no event fell"""
    ev = events[events["p"] == 1]
    y = ev["y"].astype(np.int64)
    col = np.asarray(xp_i16).astype(np.int64) if filter_id == FIRST_PER_YT else ev["x"].astype(np.int64)
    assert len(col) == len(ev)
    idx = np.arange(len(ev), dtype=np.int64)
    shape = (int(y.max()) + 1, int(col.max()) + 1)
    last = np.full(shape, -1, np.int64)
    last[y, col] = idx  # repeated cells: the last assignment stays
    first = np.full(shape, -1, np.int64)
    first[y[::-1].copy(), col[::-1].copy()] = idx[::-1].copy()  # (contiguous copies: assigned back to front, the first index stays)
    return last, first


def filter_events(events, xp_i16, filter_id, intended=False):
    """the events `filter_id` hands on for the frame `events` (xp_i16: the rectified x of its p == 1 events)"""
    ev = events[events["p"] == 1]
    last, first = survivor_maps(events, xp_i16, filter_id)
    occ = last >= 0
    li = last[occ]  # raster order
    fi = first[occ] if intended else li
    rows, cols = np.nonzero(occ)
    t32 = ev["t"].astype(np.int32)  # the reference's int32 maps: wraps
    if filter_id == LAST_PER_XY:
        t = t32[li]
    elif filter_id == MEAN_PER_XY:
        with np.errstate(over="ignore"):
            t = (t32[li] + t32[fi]) >> 1  # int32 sum (wraps), floor
    else:
        t = t32[fi]
    out = np.zeros(len(li), dtype=events.dtype)
    out["x"] = ev["x"][fi] if filter_id == FIRST_PER_YT else cols
    out["y"] = rows
    out["t"] = t.astype(np.int64)
    out["p"] = 1
    return out
