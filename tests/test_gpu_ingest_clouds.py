"""-m gpu: per-event point clouds as a stage of the device ingest (xm_ingest_set_cloud_output / xm_ingest_copy_cloud) and the
pipe's cloud_callback.

The frames never come from the package: oracle/ingest_oracle.TriggerFinderOracle cuts them out of the very packets the device
gets.  Each frame's expected cloud is the group entry on those events (XMapsEngine.frames_to_point_clouds, which
tests/test_gpu_frame_clouds.py holds against the stage call and the CPU oracle); every comparison is bit for bit, and the
statistics are compared with tests/frame_cloud_cases.oracle as well.

The stream: ingest_helpers._tiny_stream(12, seed=6) on S.C_TINY's 64 x 48 camera in quarter-period packets -- five cut frames of
1948-2491 events (tests/test_gpu_ingest_surfaces.py uses the same)."""
import functools

import numpy as np
import pytest

import frame_cloud_cases as K
import ingest_oracle as IO
from ingest_helpers import Window, _check_frames, _cpu_chain, _packets, _processor_params, _tiny_stream
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
INGEST = dict(capacity_events=1 << 13, max_packet_events=1 << 11, result_ring=16)
MAX_POINTS = 4096


@functools.lru_cache(maxsize=None)
def _tables():
    return K.add_cloud_tables(S.make_tables(CFG))


@functools.lru_cache(maxsize=None)
def _case():
    """(packets, the CPU chain's frames)"""
    packets = _packets(_tiny_stream(12, seed=6), int(1e6 / 60 / 4))
    tf = IO.TriggerFinderOracle(60)
    for p in packets:
        tf.process_events(IO.polarity_filter(p))
    assert len(_cpu_chain(packets)[0].frames) == len(tf.frames) == 5 and all(len(f) > 1000 for f in tf.frames)
    return packets, tf.frames


@pytest.fixture(scope="module")
def want():
    """the group entry on every cut frame, one frame per call: [(cloud, stats)], computed once"""
    frames = _case()[1]
    with XMapsEngine(_tables()) as eng:
        out = [eng.frames_to_point_clouds([f])[0] for f in frames]
    for (cloud, st), f in zip(out, frames):
        cloud.setflags(write=False)
        assert _stats(st) == K.oracle(_tables(), f)["stats"] and 100 < st.n_inliers < MAX_POINTS
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stats(st):
    return {f: int(getattr(st, f)) for f in K.STAT_FIELDS}


def _same(got, want):
    return got is not None and got[0].shape == want[0].shape and np.array_equal(_bits(got[0]), _bits(want[0])) and _stats(got[1]) == _stats(want[1])


def test_every_frames_cloud_equals_the_group_entry_and_the_frames_do_not_change(want):
    packets, frames = _case()
    runs = {}
    for on in (True, False):
        with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
            assert ing.cloud(0) is None  # before the stage was ever set
            if on:
                ing.set_cloud_output(True, MAX_POINTS)
            got, clouds = [], {}
            for p in packets + [None]:
                if p is not None:
                    ing.push(p)
                else:
                    ing.flush()
                for fr in ing.poll():
                    got.append(fr)
                    clouds[fr.seq] = ing.cloud(fr.seq, with_stats=True)  # right behind the poll that handed the frame out
            runs[on] = (got, clouds)
    got, clouds = runs[True]
    plain, none = runs[False]
    _check_frames(_tables(), got, frames)
    assert len(got) == len(plain) == len(frames) and all(v is None for v in none.values())  # stage off: the copy returns 0
    for a, b in zip(got, plain):  # identical to a run with the stage off
        assert np.array_equal(a.depth, b.depth) and np.array_equal(a.bgr, b.bgr) and (a.n_events, a.n_inliers) == (b.n_events, b.n_inliers)
    for i, fr in enumerate(got):
        assert _same(clouds[fr.seq], want[i]), i
        st = clouds[fr.seq][1]
        assert (st.n_events, st.t_min, st.t_max) == (fr.n_events, fr.t_first, fr.t_last), i


def test_a_small_max_points_keeps_the_first_rows(want):
    packets, frames = _case()
    small = 100
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        with pytest.raises(ValueError):
            ing.set_cloud_output(True, 0)  # max_points > 0 is required
        ing.set_cloud_output(True, small, ring=4)
        with pytest.raises(ValueError):
            ing.set_cloud_output(True, small + 1, ring=4)  # fixed by the first call that switched the stage on
        for p in packets:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        assert len(got) == len(frames) == 5
        held = [ing.cloud(fr.seq, with_stats=True) for fr in got]
        assert [h is not None for h in held] == [False, True, True, True, True]  # a ring of four, lapped once
        for i in range(1, 5):
            cloud, st = held[i]
            assert cloud.shape == (small, 3) and np.array_equal(_bits(cloud), _bits(want[i][0][:small])), i
            assert _stats(st) == _stats(want[i][1]) and st.n_inliers > small, i  # the true count: truncation is visible


def test_a_ring_of_two_is_lapped(want):
    """the twin of tests/test_gpu_ingest_surfaces.py's test: five frames through a ring of two"""
    packets, frames = _case()
    small = 100
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        ing.set_cloud_output(True, small, ring=2)
        for p in packets:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        assert len(got) == len(frames) == 5
        held = [ing.cloud(fr.seq, with_stats=True) for fr in got]
        assert [h is not None for h in held] == [False, False, False, True, True]
        for i in (3, 4):
            cloud, st = held[i]
            assert cloud.shape == (small, 3) and np.array_equal(_bits(cloud), _bits(want[i][0][:small])), i
            assert _stats(st) == _stats(want[i][1]), i
        assert ing.cloud(17) is None and ing.cloud(5) is None
        with pytest.raises(ValueError, match="the cloud ring holds 2 entries of 100 rows since the first call that switched the stage on"):
            ing.set_cloud_output(True, small, ring=3)  # the ring's length is fixed by the first call
        assert _same(ing.cloud(got[4].seq, with_stats=True), (want[4][0][:small], want[4][1]))  # the refused call changed nothing


def test_reset_empties_both_stages_rings(want):
    """one ingest with the surface and the cloud stage on: after reset() neither ring names any earlier frame"""
    packets, frames = _case()
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        ing.set_surface_output("last", np.float32)
        ing.set_cloud_output(True, MAX_POINTS)
        seen = []
        for rnd in range(2):
            for p in packets:
                ing.push(p)
            ing.flush()
            got = ing.poll()
            assert len(got) == len(frames)
            for i, fr in enumerate(got):
                assert _same(ing.cloud(fr.seq, with_stats=True), want[i]), (rnd, i)
                surf, st = ing.surface(fr.seq, with_stats=True)
                assert surf.shape == (CFG.cam_h, CFG.cam_w) and st.n_events == fr.n_events and st.n_pixels == np.count_nonzero(surf) > 0, (rnd, i)
            seen += [fr.seq for fr in got]
            ing.reset()
            assert all(ing.cloud(s) is None and ing.surface(s) is None for s in seen), rnd
        assert seen == list(range(10))


def test_switched_off_and_reset(want):
    packets, frames = _case()
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        ing.set_cloud_output(True, MAX_POINTS)
        seqs = []
        for rnd in range(2):
            for p in packets:
                ing.push(p)
            ing.flush()
            got = ing.poll()
            assert len(got) == len(frames)
            seqs.append([fr.seq for fr in got])
            for i, fr in enumerate(got):
                assert _same(ing.cloud(fr.seq, with_stats=True), want[i]), (rnd, i)
            ing.reset()  # keeps the setting, drops the ring's contents
            assert all(ing.cloud(fr.seq) is None for fr in got)
        assert seqs == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]
        ing.set_cloud_output(False)  # off: frames cut from here on have no cloud
        for p in packets:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        assert len(got) == len(frames) and all(ing.cloud(fr.seq) is None for fr in got)


def test_cloud_callback_on_both_chains(want):
    """DepthReprojectionProcessor with cloud_callback, the reference's loop without flush(): device ingest and host chain deliver
    equal arrays, each immediately before its frame and behind its surface"""
    tb = _tables()
    packets, frames = _case()
    runs = {}
    for dev in (True, False):
        log = []

        class W(Window):
            def show_async(self, img):
                log.append(("frame", img))

        params = _processor_params(tb, device_ingest=dev, activity_filter=False, cloud_callback=lambda c: log.append(("cloud", c)),
                                   surface_callback=lambda s: log.append(("surface", s)), cloud_max_points=MAX_POINTS)
        with DepthReprojectionProcessor(params, window=W(None)) as proc:
            for p in packets:
                proc.process_events(p)
        runs[dev] = log
    for dev, log in runs.items():
        assert [k for k, _ in log] == ["surface", "cloud", "frame"] * len(frames), dev
        for i in range(len(frames)):
            assert np.array_equal(_bits(log[3 * i + 1][1]), _bits(want[i][0])), (dev, i)
    # tables without the float maps / Q: refused when the pipe is constructed (the processor makes it on entry), on either chain
    bare = {k: v for k, v in tb.items() if k not in ("cam_mapx_f32", "cam_mapy_f32", "Q")}
    for dev in (True, False):
        with pytest.raises(ValueError):
            with DepthReprojectionProcessor(_processor_params(bare, device_ingest=dev, activity_filter=False, cloud_callback=lambda c: None),
                                            window=W(None)):
                pass
