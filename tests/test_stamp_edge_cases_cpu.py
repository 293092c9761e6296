"""CPU: the frames of tests/stamp_edge_cases.py are what they claim -- on the oracle alone, no GPU.  (What the kernels make of them:
tests/test_gpu_stamp_edges.py.)"""
import os
import re

import numpy as np

import stamp_edge_cases as K
import xmaps_oracle as O
from x_maps_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*parts):
    with open(os.path.join(ROOT, "x_maps_amd", "csrc", *parts)) as f:
        return f.read()


def test_stretched_and_probe_frames_keep_the_scan():
    """Every stretched / probe frame is sorted, starts at t0, spans exactly `span`, and keeps at least half of its events as
    inliers (the columns of a stretched stream are the short frame's up to rounding: the same count at every span)."""
    counts = set()
    for name, span, evs in K.int64_cases("tiny", K.N_DENSE):
        t = evs["t"].astype(np.int64)
        assert (np.diff(t) >= 0).all() and int(t[-1]) - int(t[0]) == span, name
        assert int(t[0]) == dict(K.SPANS)[span], name
        n_in = int(K.ref_events("tiny", name, evs)["mask"].sum())
        assert 2 * n_in >= len(evs), (name, n_in)
        if name.startswith("stretch"):
            counts.add(n_in)
            assert len(evs) == K.N_DENSE
        else:
            assert len(evs) > K.N_DENSE + 3 * 63 - 1
    assert len(counts) == 1, counts
    print("inliers of the stretched C-tiny frame at every span:", counts.pop(), "of", K.N_DENSE)
    for name, span, evs in K.int64_cases("shared", K.N_SHARED):  # the same list on the owner tiles' rig
        t = evs["t"].astype(np.int64)
        assert (np.diff(t) >= 0).all() and int(t[-1]) - int(t[0]) == span, name
        assert 2 * int(K.ref_events("shared", (name, K.N_SHARED), evs)["mask"].sum()) >= len(evs), name
    for rig_name, n in (("tiny", K.N_DENSE), ("shared", K.N_SHARED), ("shared", K.N_SHARED_CAPTURED)):
        spans = []
        for i, evs in enumerate(K.group_frames(rig_name, n)):
            t = evs["t"].astype(np.int64)
            assert (np.diff(t) >= 0).all()
            spans.append(int(t[-1]) - int(t[0]))
            assert 2 * int(K.ref_events(rig_name, ("group", n, i), evs)["mask"].sum()) >= n
        assert spans[0] < 2 ** 16 and spans[1] == K.TILE_SPAN_MAX and spans[2] == 2 ** 32 + 1


def test_spans_sit_on_both_sides_of_the_branches():
    spans = [s for s, _ in K.SPANS]
    assert max(s for s in spans if s < 0xffffffff) == 0xffffffff - 1 == K.TILE_SPAN_MAX  # the tiles' test is span >= 0xffffffff
    assert 0xffffffff in spans and 0xffffffff + 1 in spans and 0xffffffff + 2 in spans    # fast_frame's is span <= 0xffffffff
    assert any(2 ** 32 < s < 2 ** 53 for s in spans) and min(s for s in spans if s > 2 ** 53) == 2 ** 53 + 2
    assert max(spans) == 2 ** 63 - 1
    for s, t0 in K.SPANS:  # tmax - tmin, tmin and tmax are int64: nothing here wraps in the reference
        assert -2 ** 63 <= t0 and t0 + s <= 2 ** 63 - 1 and s <= 2 ** 63 - 1
    assert any(t0 < 0 for _, t0 in K.SPANS) and any(t0 == 0 for _, t0 in K.SPANS)
    # (double)(t - tmin) rounds past 2^53: the odd offsets are in the probe frames, and float64 does not hold them
    for s, t0 in K.SPANS:
        if s > 2 ** 53 + 3:
            evs = dict((sp, e) for nm, sp, e in K.int64_cases("tiny", K.N_DENSE) if nm.startswith("probes"))[s]
            a = evs["t"].astype(np.int64) - np.int64(t0)
            for odd in (2 ** 53 + 1, 2 ** 53 + 3):
                assert (a == odd).any() and int(np.float64(odd)) != odd


def test_probe_stamps_straddle_every_column_change():
    """For each column c the oracle's columns at the probes are not all equal and take the value c: at a0 - 1 .. a0 + 1 while one
    microsecond is above float64's resolution of a / span * S, at the wider pair from PROBE_WIDE_FROM on (there the three narrow
    probes may share a column: checked, so that the bound sits where the module says it does)."""
    _, tb = K.rig("tiny")
    scale = tb["t_px_scale"]
    narrow_fails = {}
    for span, t0 in K.SPANS:
        evs = dict((sp, e) for nm, sp, e in K.int64_cases("tiny", K.N_DENSE) if nm.startswith("probes"))[span]
        stamps = set(int(v) for v in evs["t"])
        fails = 0
        for c, offs in K.probe_offsets(span, scale):
            assert all(t0 + a in stamps for a in offs), (span, c)
            col = O.time_to_xmap_column(np.array([t0] + [t0 + a for a in offs] + [t0 + span], dtype=np.int64), scale)[1:-1]
            narrow = col[:3]
            if span < K.PROBE_WIDE_FROM:
                assert len(offs) == 3 and len(set(narrow.tolist())) > 1 and c in narrow, (span, c, narrow)
            else:
                assert len(offs) == 5 and len(set(col.tolist())) > 1 and c in col, (span, c, col)
                fails += not (len(set(narrow.tolist())) > 1 and c in narrow)
        narrow_fails[span] = fails
    assert all(v == 0 for s, v in narrow_fails.items() if s < K.PROBE_WIDE_FROM)
    assert narrow_fails[2 ** 62] > 0 and narrow_fails[2 ** 63 - 1] > 0  # one microsecond decides nothing there


def test_wild_and_equal_frames():
    for rig_name, n in (("tiny", K.N_DENSE), ("shared", K.N_SHARED)):
        w = K.wild_frames(rig_name, n)
        tm, tl = w["middle"]["t"].astype(np.int64), w["last"]["t"].astype(np.int64)
        assert (np.diff(tm) < 0).any() and int(tm.max()) - int(tm[-1]) > 2 ** 33           # unsorted: the maximum sits in the middle
        assert (np.diff(tl) >= 0).all() and int(tl[-1]) - int(tl[0]) == 12_999 + K.WILD_US  # sorted, span past 2^32
        for k, evs in w.items():
            n_in = int(K.ref_events(rig_name, ("wild", n, k), evs)["mask"].sum())
            print(rig_name, "one_wild", k, "inliers:", n_in)
            assert n_in <= 8  # every other event falls into column 0
    cfg, tb = K.rig("tiny")
    evs = K.equal(K.base_events(cfg, K.N_DENSE, 6))
    r = K.ref_events("tiny", "equal", evs)
    assert len(set(evs["t"].tolist())) == 1 and not r["mask"].any() and not r["depth"].any()


def test_float_stamps_are_exact_in_their_type():
    for kind in ("float64", "float32"):
        cases = K.float_cases("tiny", K.N_DENSE, kind)
        names = [c[0] for c in cases]
        assert "normalised raster" in names and "big base" in names and "negative base" in names
        assert ("2^20 + rel" in names) == (kind == "float32")
        for name, is_sorted, x, y, t in cases:
            assert t.dtype == np.float64 and len(t) == K.N_DENSE
            assert np.array_equal(t.astype(kind).astype(np.float64), t), (kind, name)
            assert bool((np.diff(t) >= 0).all()) == is_sorted, (kind, name)
            if name == "normalised raster":
                assert t.min() > 0 and t.max() == 1.0
                assert (np.diff(y.astype(np.int64) * 65536 + x) >= 0).all()  # raster order
            if name == "negative base":
                assert t.max() < 0
            if name == "big base":
                assert t.min() == (2.0 ** 24 if kind == "float32" else 2.0 ** 53)
                assert (np.diff(t) == 0).any()  # ties
            assert 2 * int(K.ref("tiny", (kind, name), x, y, t.astype(kind))["mask"].sum()) >= len(t), (kind, name)


def test_shapes_sit_astride_the_kernels_constants():
    """the constants the event counts and spans were chosen against are the kernels' and the plan's"""
    geo, plan = _src("xmaps_geometry.hpp"), _src("host", "xm_plan.hpp")
    common, cols, own = _src("xmaps_common.hpp"), _src("xmaps_k1cols.hpp"), _src("xmaps_k1own.hpp")
    api = _src("host", "xm_api_engine.hpp")
    # the 32-bit borders
    assert re.search(r"fast_frame = \(u64\)\(hi - lo\) <= 0xffffffffull && !degenerate;", common)
    assert re.search(r"ok = \(\(u32\)\(a >> 32\) == 0u\) & ", common)
    assert re.search(r"if \(span64 >= 0xffffffffull\) \{", cols)
    assert re.search(r"in_tile = \(u32\)\(a64 >> 32\) == 0u && av\[k\] - A_lo < A_span;", cols)
    assert re.search(r"in_tile = \(u32\)\(a64 >> 32\) == 0u && r < v_A_span;", own)
    assert re.search(r"\(unsigned long long\)\(t_last - t_first\) >= 0xffffffffull && t_last >= t_first", api)
    # dense / sparse: the tiled K1 needs blocks of >= 1024 events inside its window of w_ts = 5 time columns
    assert re.search(r"return p\.dims\.xmap_w > 0 \? \(p\.k1\.w_ts - 1\.5\) \* \(double\)n / \(double\)p\.dims\.xmap_w : 0\.0;", plan)
    assert re.search(r"k1_block_events\(p, n\) >= 1024\.0;", plan) and re.search(r"int w_ts = 5, w_x = k1_wx;", plan)
    cfg, tb = K.rig("tiny")
    xmap_w = tb["proj_x_map"].shape[1]
    assert (xmap_w, tb["proj_x_map"].shape[0], tb["t_px_scale"]) == (64, 132, 63)
    assert 3.5 * K.N_SPARSE / xmap_w < 1024 <= 3.5 * K.N_DENSE / xmap_w
    # the tiled K1's smallest block is 1024 events, eight per thread: both dense counts leave a partial last block, the ragged one
    # a partial last 8-event group as well
    assert re.search(r"#define XM_TILE_THREADS 512", geo) and re.search(r"constexpr int TILE_EPT = 4096 / XM_TILE_THREADS;", geo)
    assert re.search(r"while \(threads > 1024 / TILE_EPT && ", plan)
    assert K.N_DENSE % 1024 and K.N_RAGGED % 1024 and K.N_RAGGED % 8 and K.N_RAGGED == K.N_DENSE + 1
    # compact key frame, camera view: the order field holds the event index
    assert re.search(r"CAM32_MAX_EVENTS = \(1u << 20\) - 1u;", geo) and K.N_RAGGED + 400 < (1 << 20) - 1
    # column tiles: about `target` events per tile, at least 1024; owner tiles: at least 128 events per tile
    assert re.search(r"int xr_min = 0, w_max = 0, target = 3700;", plan) and re.search(r"if \(per_col \* W < 1024\.0\) return 0;", plan)
    assert re.search(r"return n >= tiles \* 128 && n < \(1ull << 28\) \? os\.w : 0;", plan)
    assert re.search(r"constexpr int OWN_BW = 4;", geo)
    assert K.N_DENSE / xmap_w * 1 * 3 >= 1024  # (three columns suffice; the plan takes min(3700 / 375, w_max))
    scfg, stb = K.rig("shared")
    assert K.N_SHARED >= -(-stb["proj_x_map"].shape[1] // 4) * 128
    assert K.N_SHARED == S.C_SHARED.n_events
    # a captured group takes the tiles only if it is not `direct`, i.e. dense enough for the tiled K1
    assert re.search(r"else if \(group && can_redo && n >= 2 && now\.capturing && !p\.direct && rp\.cols\.ok && !k2_untiled\)", plan)
    shared_w = stb["proj_x_map"].shape[1]
    assert 3.5 * K.N_SHARED / shared_w < 1024 <= 3.5 * K.N_SHARED_CAPTURED / shared_w
    assert 3.5 * (K.N_SHARED_CAPTURED - 1_100) / shared_w < 1024  # (the smallest round count that passes)
