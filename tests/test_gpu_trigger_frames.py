"""-m gpu: xm_trigframes -- the device-resident buffer whose frames are cut at a recording's trigger words (csrc/xmaps_exttrigger.hpp:
the append kernels; csrc/host/xm_api_exttrigger.hpp; the rule: csrc/host/xm_trigger_cut.hpp) -- against the oracle: the
word-by-word checker's events and triggers (tests/ext_trigger_ref.py), optionally p == 1 only (ext_trigger.keep_positive), cut
by TriggerFrameCutter (pinned by literals in tests/test_ext_trigger_cpu.py).  The records of every ready frame are downloaded
and compared bit for bit, the opening triggers and all counters too, after every push."""
import numpy as np
import pytest

import ext_trigger_cases as K
import ext_trigger_ref as R
from test_gpu_ext_trigger import _decoder
from x_maps_amd import XMapsEngine
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


def cds(fmt, n, rng, p=None):
    """n CD words (EVT 2.1: one to three events each), polarities random or all `p`"""
    pol = rng.integers(0, 2, n) if p is None else np.full(n, p)
    x, y, low = rng.integers(0, 600, n), rng.integers(0, 400, n), rng.integers(0, 64, n)
    mask = [int(m) for m in (1 << rng.integers(0, 32, n)) | (1 << rng.integers(0, 32, n)) | (1 << rng.integers(0, 32, n))]
    return [K.cd(fmt, int(x[i]), int(y[i]), int(pol[i]), int(low[i]), mask[i]) for i in range(n)]


class Rig:
    """a decoder + a TriggeredFrames and their oracle, fed in lockstep"""

    def __init__(self, eng, fmt, positive_only=False, max_words=4096, **cfg):
        self.eng, self.fmt, self.positive_only = eng, fmt, positive_only
        self.dec = _decoder(eng, fmt, max_words=max_words)
        self.dec.set_ext_triggers(1024)
        self.tf = X.TriggeredFrames(eng, positive_only=positive_only, **cfg)
        self.ref = R.machine(fmt)
        self.cut = X.TriggerFrameCutter(**cfg)
        self.frames = []  # every frame delivered: (events, opening trigger)

    def close(self):
        self.tf.close()
        self.dec.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def push(self, words, drain=True):
        w = K.arr(self.fmt, words) if isinstance(words, list) else words
        ev, tr = self.ref.feed(w)
        kept, trk = X.keep_positive(ev, tr) if self.positive_only else (ev, tr)
        want = self.cut.push(kept, trk, n_in=len(ev))
        assert self.tf.push(self.dec, w) == want
        assert self.tf.stats() == self.cut.stats
        if drain:
            while self.take():
                pass
        return want

    def take(self, cap=64):
        """one ready() / release() round against the oracle's; returns the number of frames"""
        ptr, offs, opening = self.tf.ready(cap)
        want = self.cut.ready(cap)
        assert len(offs) - 1 == len(opening) == len(want)
        assert ptr % 16 == 0
        got = self.tf.download(ptr, offs)
        for f, (ev, tr) in enumerate(want):
            assert got[f].tobytes() == ev.tobytes(), (len(self.frames) + f, len(got[f]), len(ev))
            assert opening[f].tobytes() == tr.tobytes()
        self.frames += want
        self.tf.release(len(want))
        self.cut.release(len(want))
        assert self.tf.stats() == self.cut.stats
        return len(want)


@pytest.mark.parametrize("positive_only", (False, True))
@pytest.mark.parametrize("fmt", K.FMTS)
def test_random_streams(eng, fmt, positive_only):
    rng = np.random.default_rng(10 * fmt + positive_only)
    with Rig(eng, fmt, positive_only, cap_events=1 << 16) as r:
        for c in range(12):
            n = int(rng.integers(1000, 4000))
            r.push(K.random_words(fmt, n, rng, trig_at=(0, n - 1) if c % 3 == 0 else (), trig_rate=0.003))
        # a chunk without a positive event between two triggers, then events again
        r.push([K.th(fmt, 900), K.trig(fmt, 0, 1)] + cds(fmt, 300, rng, p=0) + [K.trig(fmt, 0, 1)])
        r.push(cds(fmt, 200, rng) + [K.trig(fmt, 0, 1)])
        st = r.tf.stats()
        assert st["frames_cut"] == len(r.frames) > 20 and st["triggers_selected"] < st["triggers_seen"]
        if positive_only:
            assert st["events_kept"] < st["events_in"] and len(r.frames[-2][0]) == 0  # (the remap was not the identity)
            assert all((ev["p"] == 1).all() for ev, _ in r.frames)
        else:
            assert st["events_kept"] == st["events_in"] and len(r.frames[-2][0]) >= 300


@pytest.mark.parametrize("fmt", K.FMTS)
def test_index_zero_index_count_a_frame_over_three_chunks_and_five_in_one(eng, fmt):
    rng = np.random.default_rng(fmt)
    with Rig(eng, fmt, positive_only=True, cap_events=1 << 14) as r:
        assert r.push([K.th(fmt, 7), K.trig(fmt, 0, 1)] + cds(fmt, 500, rng)) == 0    # event_index 0
        assert r.push(cds(fmt, 700, rng)) == 0
        assert r.push(cds(fmt, 300, rng) + [K.trig(fmt, 0, 1)]) == 1                    # event_index = the chunk's event count
        assert len(r.frames) == 1 and len(r.frames[0][0]) > 500
        five = []
        for k in range(5):
            five += cds(fmt, 40 + 10 * k, rng) + [K.trig(fmt, 0, 1)]
        assert r.push(five) == 5
        assert len(r.frames) == 6 and r.cut.stats["events_before_first_trigger"] == 0


@pytest.mark.parametrize("positive_only", (False, True))
def test_front_moves_with_a_small_buffer(eng, positive_only):
    """cap_events = 8192, frames of about 3000 events over 20 chunks: the live part moves to the front several times"""
    fmt = 2
    rng = np.random.default_rng(5)
    with Rig(eng, fmt, positive_only, cap_events=8192) as r:
        r.push([K.th(fmt, 3)])
        for c in range(20):
            w = cds(fmt, 3000 if positive_only else 1500, rng, p=None if positive_only else 1)  # (about 1500 kept either way)
            if c % 2 == 0:
                w.insert(len(w) // 2, K.trig(fmt, 0, 1))
            r.push(w)
        st = r.tf.stats()
        assert st["front_moves"] >= 3 and st["events_dropped_open_frame"] == 0
        assert len(r.frames) == 9 and all(2700 < len(ev) < 3300 for ev, _ in r.frames)


def test_an_open_frame_that_overflows_is_dropped(eng):
    fmt = 3
    rng = np.random.default_rng(6)
    with Rig(eng, fmt, cap_events=8192) as r:
        r.push([K.th(fmt, 3), K.tl3(5), K.y3(9), K.trig(fmt, 0, 1)] + cds(fmt, 1000, rng) + [K.trig(fmt, 0, 1)])
        for _ in range(6):
            r.push(cds(fmt, 1500, rng))  # 9000 events without a trigger
        assert r.cut.stats["events_dropped_open_frame"] >= 7500 and not r.cut.open
        r.push(cds(fmt, 100, rng) + [K.trig(fmt, 0, 1)] + cds(fmt, 900, rng))
        r.push(cds(fmt, 500, rng) + [K.trig(fmt, 0, 1)])
        assert [len(ev) for ev, _ in r.frames] == [1000, 1400]
        assert r.tf.stats()["events_dropped_open_frame"] == 9000 + 100 and r.tf.stats()["events_before_first_trigger"] == 0


def test_min_events_selection_reset_and_max_frames_ready(eng):
    fmt = 21
    rng = np.random.default_rng(8)
    with Rig(eng, fmt, cap_events=1 << 14, min_events=100, id=3, edge="falling", max_frames_ready=2) as r:
        w = [K.th(fmt, 1)]
        for k in range(7):  # channel 3 falling edges cut; channel 1 and rising edges lie in between
            w += [K.trig(fmt, 3, 0, k)] + cds(fmt, 10 if k == 2 else 120, rng) + [K.trig(fmt, 1, 0, 1)] + cds(fmt, 10, rng) + [K.trig(fmt, 3, 1, 2)]
        w += [K.trig(fmt, 3, 0)]
        assert r.push(w, drain=False) == 6
        assert r.cut.stats["frames_skipped"] == 1 and r.cut.stats["triggers_selected"] == 8 and r.cut.stats["triggers_seen"] == 22
        # max_frames_ready = 2, and the skipped frame ends a run: 2, then 2 + (skipped) -> the rest at the next calls
        assert [r.take(), r.take(), r.take(), r.take()] == [2, 2, 2, 0]
        assert all(int(tr["id"]) == 3 and int(tr["value"]) == 0 for _, tr in r.frames)
        # reset: the open frame is not a frame, the stream starts over on both sides
        r.push([K.trig(fmt, 3, 0)] + cds(fmt, 200, rng), drain=False)
        r.tf.reset(), r.cut.reset(), r.dec.reset()
        r.ref = R.machine(fmt)
        n_before = len(r.frames)
        r.push(cds(fmt, 150, rng) + [K.trig(fmt, 3, 0)] + cds(fmt, 150, rng) + [K.trig(fmt, 3, 0)])
        assert len(r.frames) == n_before + 1 and r.tf.stats()["events_before_first_trigger"] >= 150


def test_push_needs_extraction_on(eng):
    with _decoder(eng, 2, max_words=64) as dec, X.TriggeredFrames(eng, cap_events=1024) as tf:
        with pytest.raises(ValueError):
            tf.push(dec, K.arr(2, [K.th(2, 1)]))
        ptr, offs, opening = tf.ready(4)
        assert len(offs) == 1 and len(opening) == 0
