"""-m gpu: camera time surfaces as a stage of the device ingest (xm_ingest_set_surface_output / xm_ingest_copy_surface) and the
pipe's surface_callback.

Expected values never come from the package: oracle/ingest_oracle.TriggerFinderOracle (and its activity filter) cuts the frames of
the very packets the device gets, tests/frame_surface_cases.oracle turns each into its surface.  Every comparison is bit for bit.

The stream: ingest_helpers._tiny_stream(12, seed=6) on S.C_TINY's 64 x 48 camera in quarter-period packets -- five cut frames of
1948-2491 events (tests/test_gpu_ingest_frame_filters.py uses the same)."""
import functools

import numpy as np
import pytest

import frame_filter_ref as R
import frame_surface_cases as K
import ingest_oracle as IO
import xmaps_oracle as O
from ingest_helpers import Window, _check_frames, _cpu_chain, _packets, _processor_params, _tiny_stream
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
INGEST = dict(capacity_events=1 << 13, max_packet_events=1 << 11, result_ring=16)


@functools.lru_cache(maxsize=None)
def _tables():
    return S.make_tables(CFG)


@functools.lru_cache(maxsize=None)
def _case(act=False):
    """(packets, the CPU chain's frames, index of the packet that cut each)"""
    packets = _packets(_tiny_stream(12, seed=6), int(1e6 / 60 / 4))
    tf = IO.TriggerFinderOracle(60)
    flt = IO.ActivityFilterOracle(CFG.cam_w, CFG.cam_h, int(1e6 / 60)) if act else None
    by = []
    for i, p in enumerate(packets):
        n = len(tf.frames)
        kept = IO.polarity_filter(p)
        tf.process_events(flt.process(kept) if flt else kept)
        by += [i] * (len(tf.frames) - n)
    if not act:
        assert len(_cpu_chain(packets)[0].frames) == len(tf.frames) == 5
    assert len(tf.frames) >= 3 and all(len(f) > 1000 for f in tf.frames)
    return packets, tf.frames, by


@functools.lru_cache(maxsize=None)
def _want(i, select="last", dtype=np.float32, act=False):
    s, st = K.oracle(_case(act)[1][i], CFG.cam_w, CFG.cam_h, select, dtype)
    s.setflags(write=False)
    return s, st


def _same(a, want):
    u = np.uint32 if want.dtype == np.float32 else np.uint64
    return a is not None and a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a.view(u), want.view(u))


def _stats(st):
    return {f: getattr(st, f) for f in K.STAT_FIELDS}


def _run(packets, setting_of_packet, flt=None, act=False, ring=0, ingest=INGEST):
    """the packets through a DeviceIngest; setting_of_packet(i) -> None (stage off) or (select, dtype) while packet i is pushed.
    Returns (frames, {seq: (surface, stats) or None}) -- the surface fetched right behind the poll that handed the frame out"""
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=act, **ingest) as ing:
        if flt:
            ing.set_frame_filter(*flt)
        got, surfs, cur = [], {}, None
        for i, p in enumerate(packets + [None]):
            if p is not None:
                if setting_of_packet(i) != cur:
                    cur = setting_of_packet(i)
                    if cur:
                        ing.set_surface_output(cur[0], cur[1], ring=ring)
                    else:
                        ing.set_surface_output(None)
                ing.push(p)
            else:
                ing.flush()
            for fr in ing.poll():
                got.append(fr)
                surfs[fr.seq] = ing.surface(fr.seq, with_stats=True)
    return got, surfs


@pytest.mark.parametrize("select,dtype", [("last", np.float32), ("first", np.float64)])
def test_every_frames_surface_equals_the_oracle_and_the_frames_do_not_change(select, dtype):
    packets, frames, _ = _case()
    got, surfs = _run(packets, lambda i: (select, dtype))
    plain, none = _run(packets, lambda i: None)
    _check_frames(_tables(), got, frames)
    assert len(got) == len(plain) == len(frames) and all(v is None for v in none.values())
    for a, b in zip(got, plain):  # identical to a run with the stage off
        assert np.array_equal(a.depth, b.depth) and np.array_equal(a.bgr, b.bgr) and (a.n_events, a.n_inliers) == (b.n_events, b.n_inliers)
    for i, fr in enumerate(got):
        want, st = _want(i, select, dtype)
        assert surfs[fr.seq] is not None, i
        assert _same(surfs[fr.seq][0], want) and _stats(surfs[fr.seq][1]) == st, i
        assert st["n_events"] == fr.n_events and st["t_base"] == fr.t_first and st["t_span"] == fr.t_last - fr.t_first


def test_a_frame_event_filter_at_the_same_time():
    """the surface is still the CUT frame's, the frames are still the filter's"""
    tb = _tables()
    packets, frames, _ = _case()
    got, surfs = _run(packets, lambda i: ("last", np.float32), flt=(R.LAST_PER_XY, False))
    assert len(got) == len(frames)
    for i, (fr, evs) in enumerate(zip(got, frames)):
        kept = R.filter_events(evs, None, R.LAST_PER_XY)
        assert len(kept) < len(evs) and fr.n_kept == len(kept) and fr.n_events == len(evs)
        x, y, t, _ = S.to_soa(kept)
        ref = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t)
        assert np.array_equal(fr.depth, ref["depth"]) and np.array_equal(fr.bgr, ref["bgr"]), i
        assert _same(surfs[fr.seq][0], _want(i)[0]) and _stats(surfs[fr.seq][1]) == _want(i)[1], i


def test_switched_on_in_mid_stream_and_off_again():
    """ordered like a push: frames cut by packets pushed before the call have no surface, later ones do"""
    packets, frames, by = _case()
    on_from, off_from = by[1] + 1, by[3] + 1  # behind the packet that cut frame 1 / frame 3: frames 2 and 3 get a surface
    got, surfs = _run(packets, lambda i: ("last", np.float32) if on_from <= i < off_from else None)
    assert len(got) == len(frames) == 5
    assert [surfs[fr.seq] is not None for fr in got] == [False, False, True, True, False]
    for i in (2, 3):
        assert _same(surfs[got[i].seq][0], _want(i)[0])


def test_a_ring_of_two_is_lapped():
    packets, frames, _ = _case()
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, **INGEST) as ing:
        ing.set_surface_output("last", np.float32, ring=2)
        with pytest.raises(ValueError):
            ing.set_surface_output("last", np.float32, ring=3)  # the ring's length is fixed by the first call
        ing.set_surface_output("first", np.float64, ring=2)  # ... select and dtype are not: frames from here on
        for p in packets:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        assert len(got) == len(frames) == 5
        held = [ing.surface(fr.seq) for fr in got]
        assert [h is not None for h in held] == [False, False, False, True, True]
        for i in (3, 4):
            assert _same(held[i], _want(i, "first", np.float64)[0]), i
        assert ing.surface(17) is None and ing.surface(5) is None


def test_reset_and_the_stream_again():
    packets, frames, _ = _case()
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, **INGEST) as ing:
        ing.set_surface_output("last", np.float32)
        seqs = []
        for rnd in range(2):
            for p in packets:
                ing.push(p)
            ing.flush()
            got = ing.poll()
            assert len(got) == len(frames)
            seqs.append([fr.seq for fr in got])
            for i, fr in enumerate(got):
                assert _same(ing.surface(fr.seq), _want(i)[0]), (rnd, i)
            ing.reset()  # keeps the setting, drops the ring's contents
            assert all(ing.surface(fr.seq) is None for fr in got)
        assert seqs == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]  # (the frame counter goes on)


def test_with_the_activity_filter():
    packets, frames, _ = _case(act=True)
    assert [len(f) for f in frames] != [len(f) for f in _case()[1]][:len(frames)]  # (the filter drops events of these frames)
    got, surfs = _run(packets, lambda i: ("last", np.float32), act=True)
    assert len(got) == len(frames)
    for i, fr in enumerate(got):
        want, st = _want(i, act=True)
        assert fr.n_events == len(frames[i])
        assert _same(surfs[fr.seq][0], want) and _stats(surfs[fr.seq][1]) == st, i


def test_surface_callback_on_both_chains():
    """DepthReprojectionProcessor with surface_callback: device ingest and host chain deliver equal arrays, each immediately before
    its frame"""
    tb = _tables()
    packets, frames, _ = _case()
    runs = {}
    for dev in (True, False):
        log = []

        class W(Window):
            def show_async(self, img):
                log.append(("frame", img))

        params = _processor_params(tb, device_ingest=dev, activity_filter=False, surface_callback=lambda s: log.append(("surface", s)))
        with DepthReprojectionProcessor(params, window=W(None)) as proc:
            for p in packets:
                proc.process_events(p)
        runs[dev] = log
    for dev, log in runs.items():
        assert [k for k, _ in log] == ["surface", "frame"] * len(frames), dev
        for i in range(len(frames)):
            assert _same(log[2 * i][1], _want(i)[0]), (dev, i)
    for a, b in zip(runs[True], runs[False]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
