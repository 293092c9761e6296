"""-m gpu: the activity filter as a stage of xm_trigframes_push (xm_trigframes_set_activity; csrc/xmaps_trigfilter.hpp, stage 1)
against the CPU chain of tests/trigger_filter_cases.py: the word-by-word checker -> p == 1 on the sensor -> the activity rule's
oracle over the WHOLE stream -> keep_where -> TriggerFrameCutter.  After every push the ready count and all counters are
compared, every ready frame is downloaded and compared byte for byte with its opening trigger, and at the end the stage's own
counters -- among them chunks_sequential against the CPU predicate that restates k_act_first's proviso."""
import numpy as np
import pytest

import ext_trigger_cases as K
import ext_trigger_ref as R
import trigger_filter_cases as TC
from test_gpu_ext_trigger import _decoder
from x_maps_amd import XMapsEngine, evt2
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
CUT = dict(cap_events=1 << 16, id=0, edge="rising", min_events=1000)


@pytest.fixture(scope="module")
def eng():
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


class Rig:
    """a decoder + a TriggeredFrames with the stage on, and the CPU chain, fed in lockstep"""

    def __init__(self, eng, fmt, thresh, include_self=False, max_words=1 << 16, c_form=False, decode=None, **cfg):
        self.fmt = fmt
        self.dec = _decoder(eng, fmt, max_words=max_words)
        self.dec.set_ext_triggers(1024)
        self.tf = X.TriggeredFrames(eng, positive_only=True, activity_thresh_us=thresh, activity_include_self=include_self, **cfg)
        self.ref = decode or R.machine(fmt).feed
        self.chain = TC.Chain(thresh, include_self, c_form, **cfg)
        self.frames = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.tf.close()
        self.dec.close()
        return False

    def push(self, words):
        ev, tr = self.ref(words)
        want = self.chain.feed(ev, tr)
        assert self.tf.push(self.dec, words) == want
        assert self.tf.stats() == self.chain.cut.stats
        while self.take():
            pass

    def take(self):
        ptr, offs, opening = self.tf.ready(64)
        want = self.chain.cut.ready(64)
        assert len(offs) - 1 == len(opening) == len(want)
        got = self.tf.download(ptr, offs)
        for f, (ev, tr) in enumerate(want):
            assert got[f].tobytes() == ev.tobytes(), (len(self.frames) + f, len(got[f]), len(ev))
            assert opening[f].tobytes() == tr.tobytes()
        self.frames += want
        self.tf.release(len(want))
        self.chain.cut.release(len(want))
        assert self.tf.stats() == self.chain.cut.stats
        return len(want)

    def check_filter_stats(self):
        st = self.tf.filter_stats()
        c = self.chain
        assert (st["events_positive"], st["events_active"], st["chunks_sequential"]) == (c.n_positive, c.n_active, c.n_sequential), st
        return st


CHUNKERS = {"one": TC.one_chunk, "uneven": TC.uneven_chunks, "under_4ms": lambda w, fmt: TC.chunks_spanning_under(w, fmt, 4000)}
# chunks judged sequentially, per (T, chunking): what tests/test_trigger_filter_cases_cpu.py pins of the CPU predicate
N_SEQUENTIAL = {(16_666, "one"): 0, (16_666, "uneven"): 0, (16_666, "under_4ms"): 0, (500, "one"): 1, (500, "uneven"): 4, (500, "under_4ms"): 0}


def _chunks(name, words, fmt):
    return CHUNKERS[name](words, fmt) if name == "under_4ms" else CHUNKERS[name](words)


@pytest.mark.parametrize("chunking", sorted(CHUNKERS))
@pytest.mark.parametrize("thresh", (16_666, 500))
@pytest.mark.parametrize("fmt", K.FMTS)
def test_stream_a_in_every_chunking(eng, fmt, thresh, chunking):
    words, _ = TC.stream_a(fmt)
    with Rig(eng, fmt, thresh, **CUT) as r:
        for c in _chunks(chunking, words, fmt):
            r.push(c)
        st = r.check_filter_stats()
        assert st["chunks_sequential"] == N_SEQUENTIAL[(thresh, chunking)]
        assert st["events_positive"] == TC.N_POSITIVE and st["events_active"] == TC.TABLE[thresh][0] == r.tf.stats()["events_kept"]
        assert len(r.frames) == 5 and r.tf.stats()["frames_skipped"] == 1
        if thresh == 500:
            assert [len(f) for f, _ in r.frames] == [n for n in TC.TABLE[500][1] if n > 1000]


@pytest.mark.parametrize("chunking", ("one", "under_4ms"))
def test_self_counts_and_min_events_behind_the_filter(eng, chunking):
    """T = 200: the frame of 991 kept events is skipped only because min_events applies to the filtered stream; with self_counts
    the own pixel's earlier events qualify too (another, larger set)"""
    fmt = 2
    words, _ = TC.stream_a(fmt)
    kept = {}
    for own in (False, True):
        with Rig(eng, fmt, 200, include_self=own, **CUT) as r:
            for c in _chunks(chunking, words, fmt):
                r.push(c)
            kept[own] = r.check_filter_stats()["events_active"]
            if not own:
                assert [len(f) for f, _ in r.frames] == [1285, 1594, 1228, 1320] and r.tf.stats()["frames_skipped"] == 2
    assert kept[True] > kept[False]


def test_reset_empties_the_history_and_switching_on_starts_empty(eng):
    fmt = 3
    words, _ = TC.stream_a(fmt)
    chunks = TC.chunks_spanning_under(words, fmt, 4000)
    half = len(chunks) // 2
    with Rig(eng, fmt, 500, **CUT) as r:
        for c in chunks:
            r.push(c)
        first = [(f.tobytes(), t.tobytes()) for f, t in r.frames]
        # reset in mid-stream, then the whole stream again: the second pass equals the first
        for c in chunks[:half]:
            r.push(c)
        r.tf.reset(), r.dec.reset(), r.chain.cut.reset(), r.chain.reset_history()
        r.ref = R.machine(fmt).feed
        n = len(r.frames)
        for c in chunks:
            r.push(c)
        assert [(f.tobytes(), t.tobytes()) for f, t in r.frames[n:]] == first
        # off: today's chain (polarity only); on again in mid-stream: an empty history, not the one the stage had before
        r.tf.reset(), r.dec.reset(), r.chain.cut.reset()
        r.ref = R.machine(fmt).feed
        r.tf.set_activity(None)
        r.chain.thresh = None
        r.chain.reset_history()
        for c in chunks[:half]:
            r.push(c)
        r.tf.set_activity(500)
        r.chain.thresh = 500
        r.chain.reset_history()
        before = r.chain.n_active
        for c in chunks[half:]:
            r.push(c)
        r.check_filter_stats()
        assert r.chain.n_active > before
    # (the CPU chain with the history carried over the switch keeps more of the chunk behind it: the case can tell)
    carried, fresh = TC.Chain(500, **CUT), TC.Chain(500, **CUT)
    dec = TC.decoded_chunks(fmt, chunks)
    for ev, tr in dec[:half]:
        carried.feed(ev, tr)
    carried.n_active = 0
    carried.feed(*dec[half]), fresh.feed(*dec[half])
    assert carried.n_active > fresh.n_active


def test_the_stage_off_is_todays_chain_and_needs_positive_only(eng):
    fmt = 21
    words, _ = TC.stream_a(fmt)
    with Rig(eng, fmt, None, **CUT) as r:  # never switched on
        for c in TC.uneven_chunks(words):
            r.push(c)
        assert len(r.frames) == 5 and sum(len(f) for f, _ in r.frames) > TC.TABLE[16_666][0] - 627
        st = r.tf.filter_stats()
        assert st == dict.fromkeys(X.TriggeredFrames.FILTER_COUNTERS, 0)
        want = TC.expected(TC.decoded_chunks(fmt, TC.uneven_chunks(words)), None, **CUT)
        assert [f.tobytes() for f, _ in r.frames] == [f.tobytes() for f, _ in want["frames"]]
    with X.TriggeredFrames(eng, cap_events=1 << 12) as tf:  # created without positive_only
        with pytest.raises(ValueError):
            tf.set_activity(500)
        tf.set_activity(None)  # off is always allowed
    with pytest.raises(ValueError):
        X.TriggeredFrames(eng, cap_events=1 << 12, activity_thresh_us=500)
    with X.TriggeredFrames(eng, cap_events=1 << 12, positive_only=True) as tf:
        with pytest.raises(ValueError):
            tf.set_activity((1 << 31) - 2)  # act_alloc's range


def _words_of(fmt, evs, at):
    return X.insert_ext_triggers(TC.ENCODE[fmt](evs), fmt, at, 0, 1)


def test_records_off_the_sensor_are_dropped_and_join_no_history(eng):
    """EVT 2.0 words carry x up to 2047: positive records at x = 64 .. 69 (beside the sensor's last column) and y = 48 .. 51 are not
    kept and qualify nobody -- the neighbours on the last column and row that only they could have vouched for are dropped too.
    Two chunks of about 1.5 ms at T = 300: the parallel path."""
    fmt = 2
    rng = np.random.default_rng(4)
    n = 6000
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["t"] = 1_000_000 + np.sort(rng.integers(0, 3000, n))
    ev["x"] = rng.integers(0, 70, n)  # 64 .. 69 are off the sensor
    ev["y"] = rng.integers(0, 52, n)  # ... 48 .. 51 too
    ev["p"] = rng.random(n) < 0.9
    off = (ev["x"] >= 64) | (ev["y"] >= 48)
    assert 0.1 < off.mean() < 0.25
    words = _words_of(fmt, ev, [0, n])
    with Rig(eng, fmt, 300, cap_events=1 << 14, id=0, edge="rising") as r:
        for c in (words[:len(words) // 2], words[len(words) // 2:]):
            r.push(c)
        st = r.check_filter_stats()
        assert st["chunks_sequential"] == 0
        (frame, _), = r.frames
        assert len(frame) == st["events_active"] and (frame["x"] < 64).all() and (frame["y"] < 48).all()
        on_pos = int(((ev["p"] == 1) & ~off).sum())
        assert 0.1 * on_pos < len(frame) < 0.9 * on_pos
    # a rule that let the off-sensor records into the history would keep more
    loose = TC.IO.ActivityFilterOracle(128, 64, 300).process(ev[ev["p"] == 1])
    assert int(((loose["x"] < 64) & (loose["y"] < 48)).sum()) > len(frame)


def test_a_chunk_whose_first_blocks_keep_nothing(eng):
    """three blocks of negative records in front of a frame: the fold of the counts in front starts with zeros, the triggers in
    front of and inside the dropped run map to kept index 0"""
    fmt = 2
    words_a, evs = TC.stream_a(fmt)
    neg = np.zeros(3 * 2048 + 100, S.EVENT_CD_DTYPE)
    neg["t"] = 4_990_000 + np.arange(len(neg))
    neg["x"], neg["y"] = np.arange(len(neg)) % 64, np.arange(len(neg)) % 48
    frame = evs[:3000]
    both = np.zeros(len(neg) + len(frame), S.EVENT_CD_DTYPE)
    both[:len(neg)], both[len(neg):] = neg, frame
    words = _words_of(fmt, both, [0, 1000, len(neg), len(both)])
    with Rig(eng, fmt, 16_666, cap_events=1 << 14, id=0, edge="rising") as r:
        r.push(words)
        st = r.check_filter_stats()
        assert [len(f) for f, _ in r.frames] == [0, 0, st["events_active"]] and st["events_active"] == 2028
        assert [int(t["event_index"]) for _, t in r.frames] == [0, 0, 0]


def test_one_chunk_of_more_than_256_blocks(eng):
    """600 000 records in one chunk (293 blocks of 2048: the fold of the counts takes its second trip), one in 500 positive so
    that the rule both keeps and drops; expected flags from the C form of the oracle, events and triggers from the host extractor."""
    fmt = 2
    n = 600_000
    rng = np.random.default_rng(9)
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["t"] = 3_000_000 + np.sort(rng.integers(0, 100_000, n))
    ev["x"], ev["y"] = rng.integers(0, 64, n), rng.integers(0, 48, n)
    ev["p"] = rng.random(n) < 1 / 500
    words = evt2.encode_evt2(ev)
    trig = K.arr(fmt, [K.trig(fmt, 0, 1)])
    words = np.concatenate((words[:len(words) // 3], trig, words[len(words) // 3:], trig))
    assert not TC.takes_sequential_path(ev, 16_666)
    with Rig(eng, fmt, 16_666, max_words=1 << 20, c_form=True, decode=X.ExtTriggerExtractor(fmt).extract, cap_events=1 << 20, id=0,
             edge="rising") as r:
        r.push(words)
        st = r.check_filter_stats()
        assert st["chunks_sequential"] == 0 and r.tf.stats()["events_in"] == n
        assert 0.1 * st["events_positive"] < st["events_active"] < 0.9 * st["events_positive"]
        (frame, opening), = r.frames
        assert 0 < int(opening["event_index"]) < st["events_active"] and len(frame) > 100
