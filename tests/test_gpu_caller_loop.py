"""-m gpu: the caller's loop as the reference writes it (python/depth_reprojection.py:60-80) --

    with DepthReprojectionProcessor(params) as proc:
        for evs in packets:
            proc.process_events(evs)

-- and nothing else.  NO TEST IN THIS MODULE CALLS flush, on the processor, the pipe or the ingest: that method does not exist in
the reference, so a caller written for the reference never calls it, and every frame cut from the packets it fed must reach its
window all the same -- the last ones by reset() / close() / __exit__ at the latest.  Same frames, same order, none lost; how soon a
frame arrives is not pinned here.

The yardstick is never the device ingest: expected frames come from the host chain of the same package (device_ingest=False:
NumPy polarity mask, activity filter, the NumPy trigger finder, one fused call per frame -- synchronous, pinned to the reference's
golden G5) or from oracle/ingest_oracle.py + xmaps_oracle.process_ev_frame.  Every comparison is np.array_equal.

The streams end with a packet that itself cuts a frame (the host chain's run says which packet that is, and every case asserts
it), so a frame is certainly in flight when the loop ends."""
import numpy as np
import pytest

from conftest import xm_option

import ingest_oracle as IO
from ingest_helpers import Window, _check_frames, _packets, _processor_params, _tiny_stream
from x_maps_amd import XMapsEngine, evt2, evt3
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor
from x_maps_amd.frame_event_filter import NoFilter
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

PERIOD_US = 1e6 / 60


class SnapshotWindow(Window):
    """keeps every frame it is shown (never a copy) and, beside it, a copy taken at delivery time"""

    def __init__(self, shown, snaps):
        super().__init__(shown)
        self.snaps = snaps

    def show_async(self, img):
        super().show_async(img)
        self.snaps.append(np.array(img))


def _feed(proc, item, how):
    getattr(proc, how)(item)


def _host_run(tb, items, how="process_events", **kw):
    """The yardstick: the host chain (device_ingest=False) over `items`, one call each.  Returns the frames shown and, per item,
    how many frames had been shown once its call returned (the host chain delivers inside the call that cuts the frame)."""
    shown, after = [], []
    with DepthReprojectionProcessor(_processor_params(tb, device_ingest=False, **kw), window=Window(shown)) as proc:
        assert proc._pipe.ingest is None
        for it in items:
            _feed(proc, it, how)
            after.append(len(shown))
    assert len(shown) == after[-1]  # (nothing arrives late on the host chain)
    return shown, after


def _end_on_a_cut(tb, items, how="process_events", min_frames=7, **kw):
    """`items` up to and including the last one that cuts a frame on the host chain, and the frames the host chain shows for
    them.  Asserts what the cases rely on: the last item cuts a frame, and there are at least `min_frames` frames."""
    shown, after = _host_run(tb, items, how, **kw)
    cutting = [i for i in range(len(items)) if after[i] > (after[i - 1] if i else 0)]
    assert cutting, "the host chain cut no frame"
    items = items[:cutting[-1] + 1]
    want, after = _host_run(tb, items, how, **kw)  # (the run the case is compared with: exactly these calls)
    assert after[-1] > (after[-2] if len(after) > 1 else 0), "the last packet must itself cut a frame"
    assert len(want) >= min_frames, len(want)
    return items, want, after


def _same_frames(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), i


# ---- (a) + (e): the frames in flight when the loop ends ---------------------------------------------------------------------------
@pytest.mark.parametrize("camera", [False, True])
@pytest.mark.parametrize("activity", [False, True])
@pytest.mark.parametrize("packets_per_period", [4, 1, 0.5])
def test_the_loop_without_anything_else_shows_every_frame(packets_per_period, activity, camera):
    """The reference's loop, device ingest (defaults otherwise) against host chain: the same frames in the same order, the one
    the last packet cuts included; and every frame -- those delivered while the processor closed too -- is the window's own:
    readable, writeable and unchanged after the processor, its ingest and its engine are gone."""
    tb = S.make_tables(S.C_TINY)
    pk = _packets(_tiny_stream(30, seed=6), int(PERIOD_US / packets_per_period))
    kw = dict(activity_filter=activity, camera_perspective=camera)
    pk, want, _ = _end_on_a_cut(tb, pk, **kw)
    shown, snaps = [], []
    with DepthReprojectionProcessor(_processor_params(tb, **kw), window=SnapshotWindow(shown, snaps)) as proc:
        assert proc._pipe.ingest is not None
        for p in pk:
            proc.process_events(p)
        in_loop = len(shown)
    print(f"frames: {len(want)} wanted, {in_loop} shown inside the loop, {len(shown)} after the block")
    assert proc.stats_printer.counters["frames shown"] == len(shown)
    _same_frames(shown, want)
    _same_frames(shown, snaps)
    for g, w in zip(shown, want):
        assert g.flags.writeable
        g[0, 0, 0] ^= 0xff  # (the window's own memory: a write goes through and touches nothing else)
        g[0, 0, 0] ^= 0xff
        assert np.array_equal(g, w)


@pytest.mark.parametrize("packets_per_period", [4, 1])
def test_views_into_the_result_ring_are_delivered_before_the_ring_is_freed(packets_per_period):
    """ingest_frame_views=True: the window gets views into the ingest's result ring (16 entries: more than the frames in flight at
    the end), valid for a while only -- so the pixels are compared inside the callback.  The views handed out while the processor
    closes must be delivered before the ring goes."""
    tb = S.make_tables(S.C_TINY)
    pk = _packets(_tiny_stream(30, seed=6), int(PERIOD_US / packets_per_period))
    pk, want, _ = _end_on_a_cut(tb, pk)
    verdicts = []

    class CheckingWindow:
        def should_close(self):
            return False

        def show_async(self, img):
            i = len(verdicts)
            verdicts.append(i < len(want) and np.array_equal(img, want[i]))

    with DepthReprojectionProcessor(_processor_params(tb, ingest_frame_views=True, ingest_result_ring=16), window=CheckingWindow()) as proc:
        for p in pk:
            proc.process_events(p)
    assert len(verdicts) == len(want) and all(verdicts), verdicts


# ---- (b) raw words ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [3, 2])
def test_raw_words_in_period_sized_chunks_show_every_frame(fmt):
    """process_evt3_words / process_evt2_words on a recording this build's encoders write, one projector period per chunk: decoded
    on the device in front of the ingest == decoded on the host in front of the host chain, the last frame included."""
    tb = S.make_tables(S.C_TINY)
    enc = evt3.encode_evt3 if fmt == 3 else evt2.encode_evt2
    how = "process_evt3_words" if fmt == 3 else "process_evt2_words"
    chunks = [enc(p) for p in _packets(_tiny_stream(30, seed=6), int(PERIOD_US)) if len(p)]
    chunks, want, _ = _end_on_a_cut(tb, chunks, how)
    shown = []
    with DepthReprojectionProcessor(_processor_params(tb), window=Window(shown)) as proc:
        for w in chunks:
            _feed(proc, w, how)
        assert proc._pipe._raw_dev  # (decoded on the device)
    _same_frames(shown, want)


# ---- (c) reset() in mid-stream ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activity", [False, True])
@pytest.mark.parametrize("packets_per_period", [4, 1])
def test_reset_delivers_what_was_cut_and_nothing_of_the_old_stream_afterwards(packets_per_period, activity):
    """A recording that loops (depth_reprojection.py:72-78): packets[:k], reset(), all packets again.  Packet k - 1 cuts a frame:
    it and every frame before it have been shown when reset() returns (in the reference they were shown inside the calls that
    cut them); what the trigger finder had buffered is discarded, so the frames after the reset are those of a fresh start."""
    tb = S.make_tables(S.C_TINY)
    pk = _packets(_tiny_stream(30, seed=6), int(PERIOD_US / packets_per_period))
    kw = dict(activity_filter=activity)
    pk, _, after = _end_on_a_cut(tb, pk, **kw)
    cutting = [i for i in range(1, len(pk)) if after[i] > after[i - 1]]
    k = cutting[len(cutting) // 2] + 1
    assert after[k - 1] > after[k - 2] and after[k - 1] >= 3

    def run(device_ingest):
        shown, at_reset = [], []
        with DepthReprojectionProcessor(_processor_params(tb, device_ingest=device_ingest, **kw), window=Window(shown)) as proc:
            for p in pk[:k]:
                proc.process_events(p)
            proc.reset()
            at_reset.append(len(shown))
            for p in pk:
                proc.process_events(p)
        return shown, at_reset[0]

    want, want_at_reset = run(False)
    assert want_at_reset == after[k - 1] and len(want) == after[k - 1] + after[-1]
    got, got_at_reset = run(True)
    print(f"shown when reset() returned: {got_at_reset} (host chain {want_at_reset}); in all {len(got)} (host chain {len(want)})")
    assert got_at_reset == want_at_reset
    _same_frames(got, want)


# ---- (d) no_frame_dropping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activity", [False, True])
@pytest.mark.parametrize("ring", [2, 3, 4, 5])
def test_no_frame_dropping_with_a_frame_on_almost_every_push(ring, activity):
    """one packet per projector period: nearly every push cuts a frame, the result ring has 2 .. 5 entries; no_frame_dropping
    (the default) must hold -- every frame of the host chain's run, bit-identical and in order, none counted as lost"""
    tb = S.make_tables(S.C_TINY)
    pk = _packets(_tiny_stream(30, seed=6), int(PERIOD_US))
    want, _ = _host_run(tb, pk, activity_filter=activity)
    if activity:
        assert len(want) >= 20, len(want)
    else:
        assert len(want) == 29, len(want)
    shown = []
    with DepthReprojectionProcessor(_processor_params(tb, ingest_result_ring=ring, activity_filter=activity), window=Window(shown)) as proc:
        assert proc._pipe.ingest._lossless
        for p in pk:
            proc.process_events(p)
    print(f"ring {ring}: {len(shown)} of {len(want)} frames shown, lost {proc.stats_printer.counters.get('frame lost', 0)}")
    assert proc.stats_printer.counters.get("frame lost", 0) == 0
    _same_frames(shown, want)


def _pieces_oracle(stream, piece):
    """the trigger finder's run when every `piece` raw events are a packet of their own (what DeviceIngest.push documents for a
    packet larger than max_packet_events)"""
    tf = IO.TriggerFinderOracle(60)
    n = 0
    for a in range(0, len(stream), piece):
        tf.process_events(IO.polarity_filter(stream[a:a + piece]))
        n += 1
    return tf.frames, n


@pytest.mark.parametrize("launch_thread", [True, False])
@pytest.mark.parametrize("n_frames,seed,n_pieces,n_cut", [(14, 4, 20, 11), (30, 6, 41, 26)])
def test_lossless_holds_for_one_push_of_a_whole_stream(n_frames, seed, n_pieces, n_cut, launch_thread):
    """ONE push of a whole stream: 20 (41) pieces of 2048 events that cut 11 (26) frames with no poll in between, a result ring of
    4.  lossless=True promises that no frame is lost, however the caller packs its events."""
    tb = S.make_tables(S.C_TINY)
    stream = _tiny_stream(n_frames, seed)
    frames, pieces = _pieces_oracle(stream, 1 << 11)
    assert (pieces, len(frames)) == (n_pieces, n_cut)
    with XMapsEngine(tb) as eng, DeviceIngest(eng, 60, lossless=True, result_ring=4, capacity_events=1 << 16, max_packet_events=1 << 11,
                                              launch_thread=launch_thread) as ing:
        ing.push(stream)
        ds = ing.device_stats()  # (everything pushed has run)
        got = ing.poll()
    print(f"{len(got)} frames polled, {sum(f.lost for f in got)} of them lost; the device cut {ds['frames_cut']}, the oracle {len(frames)}")
    assert ds["frames_cut"] == len(frames) and ds["events_dropped"] == 0
    assert not any(f.lost for f in got)
    _check_frames(tb, got, frames)


@pytest.mark.parametrize("launch_thread", [True, False])
def test_without_lossless_the_same_push_says_what_it_lost_and_tears_nothing(launch_thread):
    """lossless=False: the ring of 4 may be lapped, and then says so -- every frame polled is either `lost` without images or
    bit-identical to the oracle's frame with the same (t_first, t_last); a `lost` record may stand for several lapped frames;
    the frame cut last is still in the ring, intact."""
    tb = S.make_tables(S.C_TINY)
    stream = _tiny_stream(30, seed=6)
    frames, _ = _pieces_oracle(stream, 1 << 11)
    by_span = {(int(e["t"][0]), int(e["t"][-1])): e for e in frames}
    assert len(by_span) == len(frames) == 26
    with XMapsEngine(tb) as eng, DeviceIngest(eng, 60, lossless=False, result_ring=4, capacity_events=1 << 16, max_packet_events=1 << 11,
                                              launch_thread=launch_thread) as ing:
        ing.push(stream)
        ds = ing.device_stats()
        got = ing.poll()
    n_lost = sum(f.lost for f in got)
    print(f"{len(got)} records polled, {n_lost} lost, {len(got) - n_lost} delivered; the device cut {ds['frames_cut']}")
    assert ds["frames_cut"] == len(frames)
    assert got and all(a.seq < b.seq for a, b in zip(got[:-1], got[1:]))
    assert len(got) <= len(frames)
    for fr in got:
        if fr.lost:
            assert fr.depth is None and fr.bgr is None
        else:
            assert (fr.t_first, fr.t_last) in by_span, fr.seq
            _check_frames(tb, [fr], [by_span[(fr.t_first, fr.t_last)]])
    last = got[-1]
    assert not last.lost and last.seq == len(frames) - 1 and (last.t_first, last.t_last) == (int(frames[-1]["t"][0]), int(frames[-1]["t"][-1]))


# ---- (f) a failed ingest at exit --------------------------------------------------------------------------------------------------
def _up_to_the_first_cut(tb):
    pk = _packets(_tiny_stream(14, seed=4), int(PERIOD_US / 4))
    _, after = _host_run(tb, pk)
    first = next(i for i, n in enumerate(after) if n)
    return pk, first


def _closed(proc):
    pipe = proc._pipe
    return not pipe.ingest._g.value and not pipe.calib_maps.engine._h.value


@pytest.mark.parametrize("stop", ["at_the_first_cut", "whole_stream"])
def test_a_launch_side_error_reaches_the_caller_once_and_everything_is_released(stop):
    """XM_K2_DIRECT=1 (read by xm_create) makes the projector-view ingest refuse the first frame it cuts -- on the host, before the
    frame's K2 is launched.  The caller's loop gets that ValueError exactly once: from a process_events call when packets follow,
    from __exit__ when the loop ends with the packet that cut the frame (nothing else would ever report it).  The processor is
    closed afterwards; closing it again does nothing."""
    tb = S.make_tables(S.C_TINY)
    pk, first = _up_to_the_first_cut(tb)
    if stop == "at_the_first_cut":
        pk = pk[:first + 1]
    xm_option("XM_K2_DIRECT", "1")
    shown, errors, calls = [], [], [0]
    proc = DepthReprojectionProcessor(_processor_params(tb), window=Window(shown))
    try:
        with proc:
            for p in pk:
                calls[0] += 1
                proc.process_events(p)
    except ValueError as e:
        errors.append(e)
    assert len(errors) == 1 and "ingest needs the tiled frame kernel" in str(errors[0]), errors
    assert not isinstance(errors[0].__context__, ValueError)  # (not raised a second time while the first one was on its way)
    if stop == "at_the_first_cut":
        assert calls[0] == len(pk)  # (every packet was accepted: the error came out of __exit__)
    assert not shown and _closed(proc)
    proc._pipe.close()
    assert _closed(proc)


def test_a_caller_that_handles_the_error_in_its_loop_does_not_get_it_again_at_exit():
    tb = S.make_tables(S.C_TINY)
    pk, _ = _up_to_the_first_cut(tb)
    xm_option("XM_K2_DIRECT", "1")
    errors = []
    proc = DepthReprojectionProcessor(_processor_params(tb), window=Window([]))
    with proc:
        try:
            for p in pk:
                proc.process_events(p)
        except ValueError as e:
            errors.append(e)
    assert len(errors) == 1 and "ingest needs the tiled frame kernel" in str(errors[0]), errors
    assert _closed(proc)


def test_an_exception_of_the_callers_own_is_not_replaced_by_the_ingests_at_exit():
    """KeyError("mine") leaves the `with` block while the ingest holds an error nobody has seen (the block ends right behind the
    packet that cut the refused frame): the KeyError goes on, everything is released."""
    tb = S.make_tables(S.C_TINY)
    pk, first = _up_to_the_first_cut(tb)
    xm_option("XM_K2_DIRECT", "1")
    proc = DepthReprojectionProcessor(_processor_params(tb), window=Window([]))
    with pytest.raises(KeyError, match="mine"):
        with proc:
            for p in pk[:first + 1]:
                proc.process_events(p)
            raise KeyError("mine")
    assert _closed(proc)
    proc._pipe.close()


# ---- (g) the frame event filter switch --------------------------------------------------------------------------------------------
def test_the_frame_event_filter_switch_and_the_tail_behind_it():
    """Key E after a packet that cut a frame, the host chain (with the filter) for a while, back to the ingest, end of the loop
    on a packet that cuts a frame.  Either side starts clean at a switch, so each segment's frames are those of a host-chain
    processor fed that segment alone: the first segment's are all there once the switch has happened, the third's by the end.
    (72 projector periods: a trigger finder that starts in mid-stream may need many periods to lock -- with the activity filter
    on, the CPU chain cuts 13 / 13 / 10 frames in the three segments of this stream, and 6 / 2 / 1 in those of a 30-period one.)"""
    tb = S.make_tables(S.C_TINY)
    pk = _packets(_tiny_stream(72, seed=6), int(PERIOD_US / 4))
    _, after = _host_run(tb, pk)
    cutting = [i for i in range(1, len(pk)) if after[i] > after[i - 1]]
    a = cutting[len(cutting) // 3] + 1       # (packet a - 1 cuts a frame: it is in flight when E is pressed)
    b = cutting[2 * len(cutting) // 3] + 1
    seg1, want1, _ = _end_on_a_cut(tb, pk[:a], min_frames=3)
    assert len(seg1) == a
    seg3, want3, _ = _end_on_a_cut(tb, pk[b:], min_frames=3)

    def filtered_host_run():
        shown = []
        with DepthReprojectionProcessor(_processor_params(tb, device_ingest=False), window=Window(shown)) as proc:
            proc.keyboard_cb("e", None, "release")
            for p in pk[a:b]:
                proc.process_events(p)
        return shown

    want2 = filtered_host_run()
    assert len(want2) >= 3
    shown = []
    with DepthReprojectionProcessor(_processor_params(tb), window=Window(shown)) as proc:
        pipe = proc._pipe
        for p in seg1:
            proc.process_events(p)
        assert not pipe._host_chain_active
        proc.keyboard_cb("e", None, "release")
        assert not isinstance(pipe.ev_filter_proc.selected_filter(), NoFilter)
        proc.process_events(pk[a])  # (the switch happens with the first packet behind the key)
        assert pipe._host_chain_active
        print(f"shown once the switch has happened: {len(shown)} (host chain on the first segment: {len(want1)})")
        _same_frames(shown, want1)  # (a quarter of a period into an empty trigger finder cuts nothing)
        for p in pk[a + 1:b]:
            proc.process_events(p)
        _same_frames(shown[len(want1):], want2)
        while not isinstance(pipe.ev_filter_proc.selected_filter(), NoFilter):
            proc.keyboard_cb("e", None, "release")
        for p in seg3:
            proc.process_events(p)
        assert not pipe._host_chain_active
    print(f"shown in all: {len(shown)} (wanted {len(want1)} + {len(want2)} + {len(want3)})")
    _same_frames(shown[len(want1) + len(want2):], want3)
