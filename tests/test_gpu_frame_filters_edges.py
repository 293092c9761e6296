"""-m gpu: the frame event filters (xm_frame_event_filter: k_filter_scatter, k_filter_scan_blocks, k_filter_scan_sums,
k_filter_emit of csrc/xmaps_filters.hpp) against tests/frame_filter_ref.py past the bound of the scan of the block totals --
k_filter_scan_sums is one block that walks the totals in chunks of SCAN_BLOCK and carries a running sum, so its second trip takes
more than SCAN_BLOCK * SCAN_BLOCK = 1 048 576 cells --, with negative columns, the out-of-range error, polarities the kernel has
to drop itself, and the small maps around one scan block.

    frame     map (rows x width)   cells       scan blocks   for
    SQUARE    1025 x 1025          1 050 625   1027          the XY filters; time stamps up to 2^33 (int32 wraps in the mean)
    NARROW      41 x 32768         1 343 488   1312          FirstEventPerYT, xp over all of int16: every negative column wraps
    WRAP      1025 x 1400          1 435 000   1402          FirstEventPerYT, xp in [-200, 1399]; one xp below -width: IndexError
(the unmarked test at the end checks this table against SCAN_BLOCK on the CPU.)

One rule (_same): x, y, t and p of the output are array_equal to the reference's, for every filter in both `intended` forms.
Expected values never come from the package."""
import functools
import os
import re

import numpy as np
import pytest

import frame_filter_ref as R
from x_maps_amd import synthetic as S

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCAN_BLOCK = 1024  # csrc/xmaps_filters.hpp (checked at the end)
SQUARE, NARROW, WRAP = (1025, 1025), (41, 32768), (1025, 1400)
SQUARE_CELLS = (0, 1023, 1024, 1_048_575, 1_048_576, 1_050_624)  # first, both sides of a block edge and of the chunk edge, last
XY_CLASSES = ("FirstEventPerXYFilter", "LastEventPerXYFilter", "MeanFirstLastEventPerXYFilter")
YT_CLASS = "FirstEventPerYTFilter"
N_EVENTS = 300_000


@pytest.fixture(scope="module")
def engine():
    from x_maps_amd.engine import XMapsEngine
    with XMapsEngine(S.make_tables(S.C_TINY)) as eng:
        yield eng


def _events(rng, n, rows, cols, p_zero=0.1, t_max=1 << 33):
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["y"], ev["x"] = rng.integers(0, rows, n), rng.integers(0, cols, n)
    ev["t"] = np.sort(rng.integers(0, t_max, n))
    ev["p"] = rng.random(n) >= p_zero
    return ev


def _same(out, want, what):
    assert out.dtype == S.EVENT_CD_DTYPE and len(out) == len(want), (what, len(out), len(want))
    for fld in ("x", "y", "t", "p"):
        assert np.array_equal(out[fld], want[fld]), (what, fld, int((out[fld] != want[fld]).sum()), int(np.flatnonzero(out[fld] != want[fld])[0]))


def _through_the_class(engine, cls, ev, xp, intended):
    from x_maps_amd import frame_event_filter as F
    return getattr(F, cls)(engine, intended_semantics=intended).filter_events(ev, xp)


@functools.lru_cache(maxsize=None)
def _square():
    """-> ev: 1025 x 1025, an event forced into each of SQUARE_CELLS"""
    ev = _events(np.random.default_rng(101), N_EVENTS, *SQUARE)
    pos = np.flatnonzero(ev["p"] == 1)
    at = pos[np.linspace(0, len(pos) - 1, len(SQUARE_CELLS)).astype(int)]
    ev["y"][at], ev["x"][at] = np.divmod(SQUARE_CELLS, SQUARE[1])
    ev.flags.writeable = False
    return ev


@functools.lru_cache(maxsize=None)
def _narrow():
    """-> ev, xp (of the p == 1 events): 41 rows, xp over the full int16 range"""
    rng = np.random.default_rng(102)
    ev = _events(rng, N_EVENTS, NARROW[0], 1280)
    n_pos = int((ev["p"] == 1).sum())
    xp = rng.integers(-32768, 32768, n_pos).astype(np.int16)
    xp[[7, n_pos // 2, n_pos - 3]] = 32767, -32768, -1
    ev.flags.writeable = xp.flags.writeable = False
    return ev, xp


@functools.lru_cache(maxsize=None)
def _wrap():
    """-> ev, xp: 1025 rows, xp in [-200, 1399]"""
    rng = np.random.default_rng(103)
    ev = _events(rng, N_EVENTS, WRAP[0], 1280)
    n_pos = int((ev["p"] == 1).sum())
    xp = rng.integers(-200, 1400, n_pos).astype(np.int16)
    xp[[5, 11]] = 1399, -200
    # one cell written both ways: directly, then through the wrap
    pos = np.flatnonzero(ev["p"] == 1)
    ev["y"][pos[[100, 200]]] = 77
    xp[[100, 200]] = 1300, 1300 - WRAP[1]
    ev.flags.writeable = xp.flags.writeable = False
    return ev, xp


# ---- 1. the second trip of the sums scan, XY filters --------------------------------------------------------------------------
@gpu
def test_xy_filters_past_the_sums_scans_first_chunk(engine):
    ev = _square()
    pos = ev[ev["p"] == 1]
    assert 0.05 < (ev["p"] == 0).mean() < 0.15 and ev["t"].max() > 1 << 32
    last, first = R.survivor_maps(ev, None, R.LAST_PER_XY)
    assert last.shape == SQUARE and (last.ravel()[list(SQUARE_CELLS)] >= 0).all()
    occ = last >= 0
    assert (first[occ] != last[occ]).sum() > 1000  # cells where `intended` makes a difference
    t32 = pos["t"].astype(np.int32).astype(np.int64)
    for pair in (t32[last[occ]] + t32[first[occ]], 2 * t32[last[occ]]):  # intended / as the reference runs: exact arithmetic
        assert ((pair > np.iinfo(np.int32).max) | (pair < np.iinfo(np.int32).min)).any()  # the int32 sum of the mean wraps for real
    for cls in XY_CLASSES:
        for intended in (False, True):
            want = R.filter_events(ev, None, R.BY_CLASS[cls], intended)
            assert len(want) == occ.sum() and (want["t"] < 0).any()
            _same(_through_the_class(engine, cls, ev, None, intended), want, (cls, intended))


# ---- 2. the second trip, FirstEventPerYT on narrow rows -------------------------------------------------------------------------
@gpu
def test_first_per_yt_over_the_full_int16_range(engine):
    ev, xp = _narrow()
    pos = ev[ev["p"] == 1]
    assert pos["y"].max() == NARROW[0] - 1 and xp.max() == 32767 and xp.min() == -32768 and (xp < 0).mean() > 0.4
    last, first = R.survivor_maps(ev, xp, R.FIRST_PER_YT)
    assert last.shape == NARROW and (first[last >= 0] != last[last >= 0]).sum() > 1000
    for intended in (False, True):
        want = R.filter_events(ev, xp, R.FIRST_PER_YT, intended)
        cells = np.nonzero(last >= 0)[1]
        assert (want["x"] != cells).mean() > 0.9  # x is the surviving event's own, not the cell's column
        _same(_through_the_class(engine, YT_CLASS, ev, xp, intended), want, intended)


# ---- 3. negative columns at a width that is no multiple of anything; the out-of-range error and the call after it ---------------
@gpu
def test_negative_columns_wrap_and_one_below_the_width_is_an_index_error(engine):
    ev, xp = _wrap()
    pos = ev[ev["p"] == 1]
    last, first = R.survivor_maps(ev, xp, R.FIRST_PER_YT)
    assert last.shape == WRAP and xp.min() == -200
    assert first[77, 1300] <= 100 < 200 <= last[77, 1300] and (xp[100], xp[200]) == (1300, -100)  # one cell directly, then wrapped
    direct, wrapped = np.zeros(WRAP, bool), np.zeros(WRAP, bool)
    direct[pos["y"][xp >= 1200], xp[xp >= 1200]] = True
    wrapped[pos["y"][xp < 0], xp[xp < 0].astype(np.int64) + WRAP[1]] = True
    assert (direct & wrapped).sum() > 100 and (direct & ~wrapped).sum() > 100 and (wrapped & ~direct).sum() > 100
    want = {i: R.filter_events(ev, xp, R.FIRST_PER_YT, i) for i in (False, True)}
    for intended in (False, True):
        _same(_through_the_class(engine, YT_CLASS, ev, xp, intended), want[intended], ("legal", intended))
    bad = xp.copy()
    bad[len(bad) // 3] = -WRAP[1] - 1  # one column below -width: not a legal negative index any more
    with pytest.raises(IndexError):
        R.survivor_maps(ev, bad, R.FIRST_PER_YT)
    for intended in (False, True):
        with pytest.raises(IndexError):
            _through_the_class(engine, YT_CLASS, ev, bad, intended)
        # the counter of out-of-range indices is rearmed: the legal frame is exact again on the same engine
        _same(_through_the_class(engine, YT_CLASS, ev, xp, intended), want[intended], ("after the error", intended))


# ---- 4. polarity handled by the kernel --------------------------------------------------------------------------------------------
@gpu
def test_the_kernel_drops_the_events_whose_polarity_is_not_1(engine):
    """the classes strip p != 1 on the host; the C ABI takes the frame as it is, with xp_i16[n] (include/xmaps.h)"""
    rng = np.random.default_rng(104)
    rows, cols = 200, 333
    ev = _events(rng, 40_000, rows, cols, p_zero=0.0, t_max=1 << 33)
    ev["p"] = rng.choice(np.array([1, 1, 1, 0, -1, 2, 257], np.int16), len(ev))  # 257: the low byte alone is 1
    xp = rng.integers(-100, 500, len(ev)).astype(np.int16)  # one per event of the frame, whatever its polarity
    keep = ev["p"] == 1
    assert 0.3 < keep.mean() < 0.6 and set(np.unique(ev["p"])) == {-1, 0, 1, 2, 257}
    ev["y"][np.flatnonzero(keep)[:2]], ev["x"][np.flatnonzero(keep)[:2]] = rows - 1, cols - 1
    xp[np.flatnonzero(keep)[:2]] = 499, -100
    # events the map has no cell for, none of them with p == 1: they must neither raise nor be seen
    out = np.flatnonzero(~keep)[[3, 30, 300, 3000]]
    ev["x"][out[0]], xp[out[0]] = 40_000, 32_000  # column outside the map, XY and YT
    ev["y"][out[1]] = 50_000  # row outside the map
    xp[out[2]] = -501  # below -width
    ev["x"][out[3]], ev["y"][out[3]], xp[out[3]] = cols, rows, 500  # the first column and row outside
    shape_xy = (int(ev["y"][keep].max()) + 1, int(ev["x"][keep].max()) + 1)
    shape_yt = (shape_xy[0], int(xp[keep].max()) + 1)
    assert shape_xy == (rows, cols) and shape_yt == (rows, 500)
    for fid in (R.FIRST_PER_XY, R.LAST_PER_XY, R.MEAN_PER_XY, R.FIRST_PER_YT):
        yt = fid == R.FIRST_PER_YT
        for intended in (False, True):
            want = R.filter_events(ev, xp[keep] if yt else None, fid, intended)
            got = engine.frame_event_filter(fid, ev, xp if yt else None, shape_yt if yt else shape_xy, intended)
            _same(got, want, (fid, intended))
    # ... while the same column under a p == 1 event is the IndexError it is in the reference
    ev["p"][out[0]] = 1
    with pytest.raises(IndexError):
        engine.frame_event_filter(R.FIRST_PER_YT, ev, xp, shape_yt)
    with pytest.raises(IndexError):
        engine.frame_event_filter(R.LAST_PER_XY, ev, None, shape_xy)


# ---- 5. small edges ---------------------------------------------------------------------------------------------------------------
def _small_frames():
    """name -> (ev, rows, width): x is the cell's column for the XY filters; FirstEventPerYT gets the mirrored column as xp"""
    rng = np.random.default_rng(105)
    one = _events(rng, 1, 1, 1, p_zero=0.0)
    one["y"], one["x"] = 5, 7
    cell = _events(rng, 500, 1, 1)
    cell["y"], cell["x"] = 3, 9
    frames = {"one_event": (one, 6, 8), "one_cell": (cell, 4, 10)}
    for name, (rows, width, n) in {"cells_1024": (32, 32, 700), "cells_1025": (25, 41, 700), "all_occupied": (33, 64, 12_000)}.items():
        ev = _events(rng, n, rows, width)
        pos = np.flatnonzero(ev["p"] == 1)
        if name == "all_occupied":  # every cell once by hand, the rest at random
            ev["y"][pos[:rows * width]], ev["x"][pos[:rows * width]] = np.divmod(rng.permutation(rows * width), width)
        else:
            ev["y"][pos[:2]], ev["x"][pos[:2]] = (0, rows - 1), (0, width - 1)
        frames[name] = (ev, rows, width)
    return frames


@gpu
@pytest.mark.parametrize("name", ["one_event", "one_cell", "cells_1024", "cells_1025", "all_occupied"])
def test_small_maps(engine, name):
    ev, rows, width = _small_frames()[name]
    pos = ev[ev["p"] == 1]
    xp = (width - 1 - pos["x"].astype(np.int64)).astype(np.int16)  # mirrored: max(xp) + 1 is the width again when column 0 is hit
    last, _ = R.survivor_maps(ev, None, R.LAST_PER_XY)
    assert last.shape == (rows, width)
    assert {"one_event": len(pos) == 1, "one_cell": (last >= 0).sum() == 1 and len(pos) > 400, "cells_1024": last.size == SCAN_BLOCK,
            "cells_1025": last.size == SCAN_BLOCK + 1, "all_occupied": (last >= 0).all() and len(pos) > 2 * last.size}[name]
    if name in ("cells_1024", "cells_1025"):
        assert last[0, 0] >= 0 and last[-1, -1] >= 0  # the first and the last cell
    for cls in XY_CLASSES + (YT_CLASS,):
        for intended in (False, True):
            cols = xp if cls == YT_CLASS else None
            want = R.filter_events(ev, cols, R.BY_CLASS[cls], intended)
            if cls == YT_CLASS and name not in ("one_event", "one_cell"):
                assert R.survivor_maps(ev, xp, R.FIRST_PER_YT)[0].shape == (rows, width)
            _same(_through_the_class(engine, cls, ev, cols, intended), want, (cls, intended))


# ---- 6. geometry (CPU) ------------------------------------------------------------------------------------------------------------
def test_frames_reach_the_second_trip_of_the_sums_scan():
    src = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_filters.hpp")).read()
    scan_block = int(re.search(r"constexpr\s+int\s+SCAN_BLOCK\s*=\s*(\d+)\s*;", src).group(1))
    assert scan_block == SCAN_BLOCK
    assert re.search(r"for\s*\(u32 b0 = 0; b0 < n_blocks; b0 \+= SCAN_BLOCK\)", src)  # the loop these frames are for
    blocks = {name: -(-h * w // scan_block) for name, (h, w) in {"square": SQUARE, "narrow": NARROW, "wrap": WRAP}.items()}
    assert blocks == {"square": 1027, "narrow": 1312, "wrap": 1402} and all(b > scan_block for b in blocks.values())
    sb = scan_block
    assert SQUARE_CELLS == (0, sb - 1, sb, sb * sb - 1, sb * sb, SQUARE[0] * SQUARE[1] - 1)
    assert NARROW[1] == 32768 and max(h * w for h, w in (SQUARE, NARROW, WRAP)) * 16 <= 25_000_000  # what the entry's caller allocates
