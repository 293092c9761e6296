"""-m gpu: the frame event filters (key E of the reference, python/frame_event_filter.py) as a stage of the device ingest
(xm_ingest_set_frame_filter): between the cut and the frame kernels, on the device.

Expected values never come from the package: oracle/ingest_oracle.TriggerFinderOracle cuts the frames, tests/frame_filter_ref.py
(pinned to the reference's own outputs, golden G5) filters them, oracle/xmaps_oracle.process_ev_frame renders them.  Every frame
comparison is np.array_equal.

The stream: ingest_helpers._tiny_stream(12, seed=6) on the 64 x 48 camera of S.C_TINY in quarter-period packets -- five cut
frames of 1948-2491 events, of which LastEventPerXY keeps about 69 %."""
import functools

import numpy as np
import pytest

import frame_filter_ref as R
import ingest_oracle as IO
import xmaps_oracle as O
from ingest_helpers import Window, _packets, _processor_params, _tiny_stream
from x_maps_amd import XMapsEngine, evt3
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
INGEST = dict(capacity_events=1 << 13, max_packet_events=1 << 11, result_ring=16)
NONE = (0, False)
FILTERS = (R.FIRST_PER_YT, R.FIRST_PER_XY, R.LAST_PER_XY, R.MEAN_PER_XY)
KEY_E_ORDER = (R.FIRST_PER_YT, R.FIRST_PER_XY, R.LAST_PER_XY, R.MEAN_PER_XY, 0)  # FrameEventFilterProcessor's cycle from NoFilter


@functools.lru_cache(maxsize=None)
def _tables():
    return S.make_tables(CFG)


def _cut(packets):
    """the CPU chain over `packets`: the cut frames and, per frame, the index of the packet that cut it"""
    tf, by = IO.TriggerFinderOracle(60), []
    for i, p in enumerate(packets):
        n = len(tf.frames)
        tf.process_events(IO.polarity_filter(p))
        by += [i] * (len(tf.frames) - n)
    return tf.frames, by


@functools.lru_cache(maxsize=None)
def _stream_case(t_shift=0):
    stream = _tiny_stream(12, seed=6)
    stream["t"] += t_shift
    packets = _packets(stream, int(1e6 / 60 / 4))
    frames, by = _cut(packets)
    assert all(len(p) for p in packets)
    assert len(frames) == 5 and all(1948 <= len(f) <= 2491 for f in frames), [len(f) for f in frames]
    return packets, frames, by


def _xr(tb, evs):
    return np.asarray(tb["cam_mapx_i16"])[evs["y"], evs["x"]]


def _render(tb, evs):
    x, y, t, _ = S.to_soa(evs)
    return O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t)


def _kept(tb, evs, flt):
    fid, intended = flt
    return R.filter_events(evs, _xr(tb, evs), fid, intended) if fid else evs


_RENDERED = {}


def _want(tb_key, tb, frame_key, evs, flt):
    """(survivors, oracle frame) of cut frame `evs` under `flt`: computed once per (tables, frame, filter), shared, never changed"""
    k = (tb_key, frame_key, flt)
    if k not in _RENDERED:
        kept = _kept(tb, evs, flt)
        _RENDERED[k] = (kept, _render(tb, kept))
    return _RENDERED[k]


def _check(tb_key, tb, case_key, got, frames, flts, index_errors=None):
    assert len(got) == len(frames), (len(got), len(frames))
    for i, (fr, evs, flt) in enumerate(zip(got, frames, flts)):
        kept, ref = _want(tb_key, tb, (case_key, i), evs, flt)
        assert not fr.lost and fr.overflow == 0, (i, fr.lost, fr.overflow)
        assert (fr.n_events, fr.t_first, fr.t_last) == (len(evs), int(evs["t"][0]), int(evs["t"][-1])), (i, flt)  # the CUT frame's
        assert fr.n_kept == len(kept), (i, flt, fr.n_kept, len(kept))
        assert fr.n_inliers == int(ref["mask"].sum()), (i, flt)
        assert fr.n_index_errors == (index_errors[i] if index_errors else 0), (i, flt, fr.n_index_errors)
        assert np.array_equal(fr.depth, ref["depth"]) and np.array_equal(fr.bgr, ref["bgr"]), (i, flt)


def _run(tb, packets, flt_of_packet):
    """the packets through a DeviceIngest; flt_of_packet(i) -> the filter selected while packet i is pushed (told to the ingest
    when it changes: between pushes, no flush, no reset)"""
    with XMapsEngine(tb) as eng, DeviceIngest(eng, 60, **INGEST) as ing:
        got, cur = [], NONE
        for i, p in enumerate(packets):
            if flt_of_packet(i) != cur:
                cur = flt_of_packet(i)
                ing.set_frame_filter(*cur)
            ing.push(p)
            got += ing.poll()
        ing.flush()
        got += ing.poll()
    return got


def test_the_stream_can_tell_the_filters_apart():
    """Preconditions of every case below, on the first three frames: the filter drops events, and the oracle's frame differs
    between raster and time order of the survivors and between filtered and unfiltered events."""
    tb = _tables()
    _, frames, _ = _stream_case()
    for evs in frames[:3]:
        kept = R.filter_events(evs, None, R.LAST_PER_XY)
        assert 0.6 < len(kept) / len(evs) < 0.75
        raster, by_time, unfiltered = _render(tb, kept)["bgr"], _render(tb, np.sort(kept, order="t", kind="stable"))["bgr"], _render(tb, evs)["bgr"]
        assert not np.array_equal(raster, by_time) and not np.array_equal(raster, unfiltered)


@pytest.mark.parametrize("intended", [False, True])
@pytest.mark.parametrize("fid", FILTERS)
def test_each_filter_both_semantics(fid, intended):
    """The filter set before the first push: every frame == the oracle's on the restatement's survivors; n_events / t_first /
    t_last stay the cut frame's, n_kept / n_inliers are the filtered frame's, no index error, nothing lost."""
    tb = _tables()
    packets, frames, _ = _stream_case()
    got = _run(tb, packets, lambda i: (fid, intended))
    _check("tiny", tb, "plain", got, frames, [(fid, intended)] * len(frames))
    if fid == R.FIRST_PER_XY:  # (the two semantics are different frames on this stream)
        assert len(_want("tiny", tb, ("plain", 0), frames[0], (fid, True))[0]) == len(_want("tiny", tb, ("plain", 0), frames[0], (fid, False))[0])
        assert not np.array_equal(_want("tiny", tb, ("plain", 0), frames[0], (fid, True))[1]["bgr"],
                                  _want("tiny", tb, ("plain", 0), frames[0], (fid, False))[1]["bgr"])


def test_yt_cells_are_not_xy_cells():
    """A rectify table quantised to q columns merges (y, xr) cells that stay apart as (y, x): the smallest power of two q for which
    FirstEventPerYT keeps fewer events than the XY filters on frame 0 (4: the table's slope is 2)."""
    tb0 = _tables()
    packets, frames, _ = _stream_case()
    m = np.asarray(tb0["cam_mapx_i16"])
    n_xy = len(R.filter_events(frames[0], None, R.LAST_PER_XY))
    for q in (1, 2, 4, 8, 16):
        tb = dict(tb0)
        tb["cam_mapx_i16"] = ((m // q) * q).astype(np.int16)
        if len(R.filter_events(frames[0], _xr(tb, frames[0]), R.FIRST_PER_YT)) < n_xy:
            break
    assert q == 4
    assert len(R.filter_events(frames[0], _xr(tb, frames[0]), R.FIRST_PER_YT)) < n_xy
    got = _run(tb, packets, lambda i: (R.FIRST_PER_YT, False))
    _check("q4", tb, "plain", got, frames, [(R.FIRST_PER_YT, False)] * len(frames))
    assert got[0].n_kept < n_xy


@pytest.mark.parametrize("intended", [False, True])
def test_negative_yt_columns_wrap_at_the_frames_own_width(intended):
    """cam_mapx_i16 - 12: xr in [-2, 126]; frames 0 and 2 hold events in negative columns, which wrap at the frame's own width
    (127 and 107: the per-frame maximum must be known on the device), frame 1 holds none.  The reference raises nothing here."""
    tb = dict(_tables())
    tb["cam_mapx_i16"] = (np.asarray(tb["cam_mapx_i16"]) - 12).astype(np.int16)
    packets, frames, _ = _stream_case()
    xr = [_xr(tb, f) for f in frames[:3]]
    assert (min(int(v.min()) for v in xr), max(int(v.max()) for v in xr)) == (-2, 126)
    assert [int((v < 0).sum()) for v in xr] == [33, 0, 25] and [int(v.max()) + 1 for v in xr] == [127, 127, 107]
    got = _run(tb, packets, lambda i: (R.FIRST_PER_YT, intended))
    _check("neg12", tb, "plain", got, frames, [(R.FIRST_PER_YT, intended)] * len(frames))


@pytest.mark.parametrize("fid", [R.LAST_PER_XY, R.MEAN_PER_XY])
def test_time_stamps_wrap_through_int32(fid):
    """t += 2^31 + 12345: the survivors' stamps go through the reference's int32 maps and come out negative."""
    tb = _tables()
    packets, frames, _ = _stream_case((1 << 31) + 12345)
    assert all((R.filter_events(f, None, R.LAST_PER_XY)["t"] < 0).all() for f in frames)
    got = _run(tb, packets, lambda i: (fid, False))
    _check("tiny", tb, "big_t", got, frames, [(fid, False)] * len(frames))


def test_switching_the_filter_inside_one_stream():
    """none -> LastEventPerXY -> FirstEventPerYT -> none, switched between pushes with no flush and no reset: every frame is the
    oracle's under the filter selected when the packet that cut it was pushed, and the frames under "none" are those of an ingest
    that never had a filter."""
    tb = _tables()
    packets, frames, by = _stream_case()
    seq = [NONE, (R.LAST_PER_XY, False), (R.FIRST_PER_YT, False), NONE, NONE]
    # the filter changes right behind the packet that cut a frame: frame k is cut under seq[k]; the packets behind the last cut
    # (the stream's tail, which cuts nothing) stay under the last entry
    flt_of_packet = lambda i: seq[min(sum(1 for b in by if b < i), len(seq) - 1)]  # noqa: E731
    assert by[-1] < len(packets) - 1  # (there is such a tail)
    assert [flt_of_packet(b) for b in by] == seq
    got = _run(tb, packets, flt_of_packet)
    _check("tiny", tb, "plain", got, frames, seq)
    plain = _run(tb, packets, lambda i: NONE)
    for k in (0, 3, 4):
        assert np.array_equal(got[k].bgr, plain[k].bgr) and np.array_equal(got[k].depth, plain[k].depth)
        assert got[k].n_kept == got[k].n_events == plain[k].n_kept


@pytest.mark.parametrize("fid", [R.LAST_PER_XY, R.FIRST_PER_YT])
def test_events_outside_the_sensor_are_dropped_and_counted(fid):
    """Three events of frame 0 carry x = cam_w (the reference raises IndexError there): left out, n_index_errors == 3, the frame
    is the oracle's on the rest."""
    tb = _tables()
    packets, frames, _ = _stream_case()
    t_bad = frames[0]["t"][[500, 1000, 1500]]
    assert len(set(t_bad.tolist())) == 3
    packets = [p.copy() for p in packets]
    for p in packets:
        p["x"][np.isin(p["t"], t_bad) & (p["p"] == 1)] = CFG.cam_w
    frames2, _ = _cut(packets)
    assert [len(f) for f in frames2] == [len(f) for f in frames] and int((frames2[0]["x"] == CFG.cam_w).sum()) == 3
    rest = [f[f["x"] < CFG.cam_w] for f in frames2]
    got = _run(tb, packets, lambda i: (fid, False))
    assert len(got) == len(frames2)
    for i, (fr, evs, ok) in enumerate(zip(got, frames2, rest)):
        kept = _kept(tb, ok, (fid, False))
        ref = _render(tb, kept)
        assert (fr.n_events, fr.t_first, fr.t_last) == (len(evs), int(evs["t"][0]), int(evs["t"][-1]))
        assert fr.n_index_errors == (3 if i == 0 else 0) and fr.n_kept == len(kept) and fr.n_inliers == int(ref["mask"].sum())
        assert np.array_equal(fr.depth, ref["depth"]) and np.array_equal(fr.bgr, ref["bgr"]), i


def test_key_e_keeps_the_stream_on_the_ingest():
    """The reference's call pattern with RuntimeParams.device_frame_filters: key E pressed between packets (right behind every
    packet that cuts a frame) -- the stream never leaves the ingest, nothing is reset, and the frames shown are the oracle's
    under the filter selected when they were cut: NoFilter, then the four filters in the order E cycles them."""
    tb = _tables()
    packets, frames, by = _stream_case()
    shown = []
    with DepthReprojectionProcessor(_processor_params(tb, device_frame_filters=True, activity_filter=False), window=Window(shown)) as proc:
        pipe = proc._pipe
        assert pipe.ingest is not None
        for i, p in enumerate(packets):
            proc.process_events(p)
            assert not pipe._host_chain_active
            if i in by:
                proc.keyboard_cb("e", None, "release")
    assert not pipe._host_chain_active
    flts = [NONE] + [(f, False) for f in KEY_E_ORDER[:4]]
    assert len(shown) == len(frames) == len(flts)
    for i, (img, evs, flt) in enumerate(zip(shown, frames, flts)):
        assert np.array_equal(img, _want("tiny", tb, ("plain", i), evs, flt)[1]["bgr"]), (i, flt)
    assert proc.stats_printer.metrics["frame evs filtered out [%]"].max > 0


def test_evt3_words_take_the_same_stage():
    """The same stream as EVT 3.0 words through process_evt3_words with LastEventPerXY selected: the frames of
    test_each_filter_both_semantics."""
    tb = _tables()
    packets, frames, _ = _stream_case()
    shown = []
    with DepthReprojectionProcessor(_processor_params(tb, device_frame_filters=True, activity_filter=False), window=Window(shown)) as proc:
        for _ in range(3):  # NoFilter -> FirstEventPerYT -> FirstEventPerXY -> LastEventPerXY
            proc.keyboard_cb("e", None, "release")
        assert str(proc._pipe.ev_filter_proc.selected_filter()) == "LastEventPerXYFilter"
        for p in packets:
            proc.process_evt3_words(evt3.encode_evt3(p))
        assert proc._pipe._raw_dev and not proc._pipe._host_chain_active
    assert len(shown) == len(frames)
    for i, (img, evs) in enumerate(zip(shown, frames)):
        assert np.array_equal(img, _want("tiny", tb, ("plain", i), evs, (R.LAST_PER_XY, False))[1]["bgr"]), i
