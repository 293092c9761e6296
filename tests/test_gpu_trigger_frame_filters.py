"""-m gpu: the frame event filters as a stage on runs of ready triggered frames (xm_trigframes_set_frame_filter /
xm_trigframes_ready_filtered; csrc/xmaps_trigfilter.hpp, stage 2).  Per frame the survivors equal
frame_filter_ref.filter_events(frame, xp, filter, intended) field for field -- the frames are the CPU chain's
(tests/trigger_filter_cases.py), xp comes from the tables' cam_mapx_i16 -- and the offsets are the running sum of their lengths."""
import numpy as np
import pytest

import frame_filter_ref as FR
import trigger_filter_cases as TC
from test_gpu_ext_trigger import _decoder
from x_maps_amd import XMapsEngine
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
FILTERS = (FR.FIRST_PER_YT, FR.FIRST_PER_XY, FR.LAST_PER_XY, FR.MEAN_PER_XY)
FMT = 2
W, H = S.C_TINY.cam_w, S.C_TINY.cam_h


@pytest.fixture(scope="module")
def tb():
    return S.make_tables(S.C_TINY)


@pytest.fixture(scope="module")
def eng(tb):
    with XMapsEngine(tb) as e:
        yield e


def _want(tb, frame, fid, intended):
    """(survivors, index errors) of one frame: events off the sensor are left out and counted, the rest go through the restatement"""
    ok = (frame["x"] < W) & (frame["y"] < H)
    on = frame[ok]
    if len(on) == 0:
        return np.zeros(0, S.EVENT_CD_DTYPE), int((~ok).sum())
    xp = np.asarray(tb["cam_mapx_i16"])[on["y"], on["x"]]
    return FR.filter_events(on, xp, fid, intended), int((~ok).sum())


class Rig:
    def __init__(self, eng, tb, thresh=None, **cfg):
        self.tb = tb
        self.dec = _decoder(eng, FMT, max_words=1 << 16)
        self.dec.set_ext_triggers(1024)
        self.tf = X.TriggeredFrames(eng, positive_only=True, activity_thresh_us=thresh, **cfg)
        self.chain = TC.Chain(thresh, **cfg)
        self.ref = TC.R.machine(FMT)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tf.close()
        self.dec.close()
        return False

    def push(self, words):
        ev, tr = self.ref.feed(words)
        assert self.tf.push(self.dec, words) == self.chain.feed(ev, tr)

    def take(self, cap, fid, intended, twice=True):
        """one ready_filtered(cap) against the restatement on the cutter's run; released on both sides; -> the run's frames"""
        run = self.chain.cut.ready(cap)
        ptr, offs, opening, bad = self.tf.ready_filtered(cap)
        assert len(offs) - 1 == len(run) == len(opening) == len(bad) and offs[0] == 0
        got = self.tf.download(ptr, offs)
        want = [_want(self.tb, ev, fid, intended) for ev, _ in run]
        assert offs.tolist() == np.concatenate(([0], np.cumsum([len(w) for w, _ in want]))).astype(np.uint64).tolist()
        for f, ((w, n_bad), (_, trig)) in enumerate(zip(want, run)):
            for k in ("x", "y", "p", "t"):
                assert np.array_equal(got[f][k], w[k]), (f, k, fid, intended)
            assert int(bad[f]) == n_bad and opening[f].tobytes() == trig.tobytes()
        if twice:  # a second call right behind the first: the maps were left zero (a cell left behind would rank a stale survivor)
            ptr2, offs2, _, bad2 = self.tf.ready_filtered(cap)
            assert offs2.tolist() == offs.tolist() and bad2.tolist() == bad.tolist()
            assert [g.tobytes() for g in self.tf.download(ptr2, offs2)] == [g.tobytes() for g in got]
        self.tf.release(len(run))
        self.chain.cut.release(len(run))
        return run, want


@pytest.mark.parametrize("intended", (False, True))
@pytest.mark.parametrize("fid", FILTERS)
def test_runs_of_one_two_and_five_frames(eng, tb, fid, intended):
    """stream A twice with min_events = 0: thirteen ready frames (each pass closes six, the trigger behind the first pass opens an
    empty seventh) -- runs of 1, 2, 5 and, capped by max_frames, the last 5"""
    words, _ = TC.stream_a(FMT)
    with Rig(eng, tb, cap_events=1 << 16, id=0, edge="rising") as r:
        r.tf.set_frame_filter(fid, intended, max_frames=5)
        r.push(words)
        r.push(words)
        sizes, kept, n_in, n_empty = [], 0, 0, 0
        for cap in (1, 2, 5, 64):
            run, want = r.take(cap, fid, intended)
            sizes.append(len(run))
            kept += sum(len(w) for w, _ in want)
            n_in += sum(len(ev) for ev, _ in run)
            n_empty += sum(len(ev) == 0 for ev, _ in run)
        assert sizes == [1, 2, 5, 5] and 0.5 * n_in < kept < 0.8 * n_in and n_empty == 1
        st = r.tf.filter_stats()
        assert (st["frames_filtered"], st["events_after_frame_filter"], st["index_errors"]) == (2 * 13, 2 * kept, 0)
        assert r.tf.ready_filtered(8)[1].tolist() == [0]


def test_the_two_semantics_differ_on_this_stream(tb):
    (ev, tr), = TC.decoded_chunks(FMT, [TC.stream_a(FMT)[0]])
    frame = ev[:3000][ev[:3000]["p"] == 1]
    a, b = _want(tb, frame, FR.FIRST_PER_XY, False)[0], _want(tb, frame, FR.FIRST_PER_XY, True)[0]
    assert len(a) == len(b) < len(frame) and not np.array_equal(a["t"], b["t"])


def test_a_skipped_frame_ends_a_run_and_filter_0_is_ready(eng, tb):
    words, _ = TC.stream_a(FMT)
    with Rig(eng, tb, cap_events=1 << 16, id=0, edge="rising", min_events=1000) as r:
        r.tf.set_frame_filter(FR.LAST_PER_XY, False, max_frames=8)
        r.push(words)
        assert [len(r.take(64, FR.LAST_PER_XY, False)[0]) for _ in range(3)] == [2, 3, 0]
        # no filter selected: exactly ready()
        r.tf.set_frame_filter(0)
        r.tf.reset(), r.dec.reset(), r.chain.cut.reset()
        r.ref = TC.R.machine(FMT)
        r.push(words)
        ptr, offs, opening = r.tf.ready(64)
        ptr2, offs2, opening2, bad = r.tf.ready_filtered(64)
        assert ptr2 == ptr and offs2.tolist() == offs.tolist() and len(offs) == 3 and opening2.tobytes() == opening.tobytes()
        assert bad.tolist() == [0, 0]


@pytest.mark.parametrize("fid", (FR.LAST_PER_XY, FR.FIRST_PER_YT))
def test_events_off_the_sensor_are_counted(eng, tb, fid):
    _, evs = TC.stream_a(FMT)
    evs = evs.copy()
    pos = np.nonzero(evs["p"] == 1)[0]
    evs["x"][pos[[100, 900, 1700]]] = W          # frame 0
    evs["y"][pos[[8000, 8001]]] = H + 3          # a later frame
    words = X.insert_ext_triggers(TC.ENCODE[FMT](evs), FMT, np.concatenate(([0], np.cumsum(TC.N_EVENTS))), 0, 1)
    with Rig(eng, tb, cap_events=1 << 16, id=0, edge="rising") as r:
        r.tf.set_frame_filter(fid, False, max_frames=6)
        r.push(words)
        run, want = r.take(6, fid, False)
        counts = [n for _, n in want]
        assert counts[0] == 3 and sorted(counts) == [0, 0, 0, 0, 2, 3] and r.tf.filter_stats()["index_errors"] == 2 * 5


@pytest.mark.parametrize("intended", (False, True))
def test_negative_yt_columns_wrap_at_each_frames_own_width(tb, intended):
    """cam_mapx_i16 - 12: negative columns wrap at the frame's own max(xr) + 1 -- frames of different widths in one run"""
    tb2 = dict(tb)
    tb2["cam_mapx_i16"] = (np.asarray(tb["cam_mapx_i16"]) - 12).astype(np.int16)
    _, evs = TC.stream_a(FMT)
    keep = np.ones(len(evs), bool)
    keep[3000:5600] = evs[3000:5600]["x"] < 50  # the second frame loses its right columns: a narrower map of its own
    evs2 = np.zeros(int(keep.sum()), S.EVENT_CD_DTYPE)
    evs2[:] = evs[keep]
    starts = np.concatenate(([0], np.cumsum(keep)))[np.concatenate(([0], np.cumsum(TC.N_EVENTS)))]
    words = X.insert_ext_triggers(TC.ENCODE[FMT](evs2), FMT, starts, 0, 1)
    with XMapsEngine(tb2) as eng2, Rig(eng2, tb2, cap_events=1 << 16, id=0, edge="rising") as r:
        r.tf.set_frame_filter(FR.FIRST_PER_YT, intended, max_frames=6)
        r.push(words[:len(words) // 2])
        r.push(words[len(words) // 2:])
        run = r.chain.cut.ready(6)
        xr = [np.asarray(tb2["cam_mapx_i16"])[ev["y"], ev["x"]] for ev, _ in run]
        assert len(run) == 6 and sum(int((v < 0).sum()) for v in xr) > 20 and len({int(v.max()) for v in xr}) > 1  # (widths differ)
        r.take(6, FR.FIRST_PER_YT, intended)


def test_the_cell_limit_refuses_first_per_yt_and_changes_nothing():
    """a 640 x 480 rig whose rectify table holds one entry of 9000: 480 x 9001 cells exceed XM_INGEST_YT_MAX_CELLS"""
    tb = dict(S.make_tables(S.C_1M))
    m = np.array(tb["cam_mapx_i16"])
    m[0, 0] = 9000
    tb["cam_mapx_i16"] = m
    with XMapsEngine(tb) as eng, X.TriggeredFrames(eng, cap_events=1 << 12, positive_only=True) as tf:
        tf.set_frame_filter(FR.LAST_PER_XY, False, max_frames=2)
        with pytest.raises(ValueError):
            tf.set_frame_filter(FR.FIRST_PER_YT, False, max_frames=2)
        with pytest.raises(ValueError):
            tf.set_frame_filter(7)
        with pytest.raises(ValueError):
            tf.set_frame_filter(FR.LAST_PER_XY, False, max_frames=0)
        ptr, offs, _, _ = tf.ready_filtered(4)  # the filter selected before the refusals is still the one
        assert ptr != tf.ready(4)[0] and offs.tolist() == [0]


def test_both_stages_together(eng, tb):
    """the frame filter on activity-filtered frames (T = 500, chunks under 4 ms)"""
    words, _ = TC.stream_a(FMT)
    with Rig(eng, tb, thresh=500, cap_events=1 << 16, id=0, edge="rising", min_events=1000) as r:
        r.tf.set_frame_filter(FR.MEAN_PER_XY, True, max_frames=4)
        for c in TC.chunks_spanning_under(words, FMT, 4000):
            r.push(c)
        run, want = r.take(4, FR.MEAN_PER_XY, True)
        assert [len(ev) for ev, _ in run] == [1876, 1514] and all(len(w) < len(ev) for (w, _), (ev, _) in zip(want, run))
        run, _ = r.take(4, FR.MEAN_PER_XY, True)
        assert [len(ev) for ev, _ in run] == [2228, 1804, 1928]
        st = r.tf.filter_stats()
        assert st["events_active"] == 9586 and st["frames_filtered"] == 2 * 5
