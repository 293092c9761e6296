"""-m gpu: EVT 3.0 words of the cut frames as a stage of the device ingest (xm_ingest_set_record_output / xm_ingest_copy_record).

The frames never come from the package: oracle/ingest_oracle.TriggerFinderOracle cuts them out of the very packets the device
gets (behind oracle/ingest_oracle's polarity and activity filters).  Each frame's expected words are the group entry on those events
(XMapsEngine.frames_to_evt3_words, which tests/test_gpu_evt3_record.py holds against the host encoder) AND the host encoder itself;
every comparison is bit for bit.

The stream: ingest_helpers._tiny_stream(12, seed=6) on S.C_TINY's 64 x 48 camera -- whose stamps are all different -- with one
event in twelve followed by one to three events of the same stamp, row and polarity in the next columns (vector runs), in
quarter-period packets: five cut frames of about 2 300-2 900 events."""
import functools

import numpy as np
import pytest

import evt3_record_cases as K
import frame_filter_ref as R
import ingest_oracle as IO
from ingest_helpers import _check_frames, _cpu_chain, _packets, _tiny_stream
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
INGEST = dict(capacity_events=1 << 13, max_packet_events=1 << 11, result_ring=16)
MAX_WORDS = 1 << 14


@functools.lru_cache(maxsize=None)
def _tables():
    return S.make_tables(CFG)


@functools.lru_cache(maxsize=None)
def _stream():
    base = _tiny_stream(12, seed=6)
    rng = np.random.default_rng(8)
    extra = np.where((rng.random(len(base)) < 1 / 12) & (base["x"] < CFG.cam_w - 3), rng.integers(1, 4, len(base)), 0)
    out = base.repeat(1 + extra)
    first = np.cumsum(1 + extra) - (1 + extra)
    out["x"] += (np.arange(len(out)) - first.repeat(1 + extra)).astype(np.uint16)
    assert (np.diff(out["t"]) >= 0).all() and out["x"].max() < CFG.cam_w
    return out


@functools.lru_cache(maxsize=None)
def _case(act):
    """(packets, the CPU chain's frames) with the activity filter on or off"""
    packets = _packets(_stream(), int(1e6 / 60 / 4))
    tf = _cpu_chain(packets, act=IO.ActivityFilterC(CFG.cam_w, CFG.cam_h, int(1e6 / 60)) if act else None)[0]
    assert len(tf.frames) == 5 and all(len(f) > 1000 for f in tf.frames)
    return packets, tf.frames


def _cut_by(packets):
    """per cut frame, the index of the packet that cut it (no activity filter)"""
    tf, by = IO.TriggerFinderOracle(60), []
    for i, p in enumerate(packets):
        n = len(tf.frames)
        tf.process_events(IO.polarity_filter(p))
        by += [i] * (len(tf.frames) - n)
    return by


@pytest.fixture(scope="module")
def want():
    """{(act, vec): [(words, stats)]}: the group entry on every cut frame, equal to the host encoder; computed once"""
    out = {}
    with XMapsEngine(_tables()) as eng:
        for act in (False, True):
            frames = _case(act)[1]
            for vec in (True, False):
                words, stats = eng.frames_to_evt3_words(frames, use_vectors=vec)
                for w, st, f in zip(words, stats, frames):
                    ref, ref_st = K.oracle(f, vec)
                    assert np.array_equal(w, ref) and _stats(st) == ref_st and len(w) < MAX_WORDS
                    w.setflags(write=False)
                out[act, vec] = list(zip(words, stats))
    assert len(_case(True)[1][0]) < len(_case(False)[1][0])  # the activity filter drops events of this stream
    assert all(st.n_vector_runs > 50 for _, st in out[False, True] + out[True, True])
    return out


def _stats(st):
    return {f: int(getattr(st, f)) for f in K.STAT_FIELDS}


def _same(got, want):
    return got is not None and got[0] is not None and np.array_equal(got[0], want[0]) and _stats(got[1]) == _stats(want[1])


def _run(act, setup=None, after_push=None):
    """the packets through a DeviceIngest -> (frames, {seq: record right behind the poll that handed the frame out})"""
    packets = _case(act)[0]
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=act, **INGEST) as ing:
        assert ing.record(0) is None  # before the stage was ever set
        if setup:
            setup(ing)
        got, recs = [], {}
        for i, p in enumerate(packets + [None]):
            if p is not None:
                ing.push(p)
                if after_push:
                    after_push(ing, i)
            else:
                ing.flush()
            for fr in ing.poll():
                got.append(fr)
                recs[fr.seq] = ing.record(fr.seq)
    return got, recs


@pytest.mark.parametrize("act", [False, True], ids=["plain", "activity"])
def test_every_frames_words_equal_the_group_entry_and_the_frames_do_not_change(want, act):
    frames = _case(act)[1]
    on, recs = _run(act, lambda ing: ing.set_record_output(True, True, MAX_WORDS))
    off, none = _run(act)
    _check_frames(_tables(), on, frames)
    assert len(on) == len(off) == len(frames) and all(v is None for v in none.values())  # stage off: nothing published, the copy returns 0
    for a, b in zip(on, off):  # byte-identical to a run with the stage off
        assert a.depth.tobytes() == b.depth.tobytes() and a.bgr.tobytes() == b.bgr.tobytes() and (a.n_events, a.n_inliers) == (b.n_events, b.n_inliers)
    for i, fr in enumerate(on):
        assert _same(recs[fr.seq], want[act, True][i]), i
        st = recs[fr.seq][1]
        assert (st.n_events, st.t_first, st.t_last) == (fr.n_events, fr.t_first, fr.t_last), i


def test_single_events_and_a_setting_that_changes_between_pushes(want):
    """use_vectors may change from call to call (ordered like a push); off in between launches nothing: no record for those frames"""
    frames = _case(False)[1]
    got, recs = _run(False, lambda ing: ing.set_record_output(True, False, MAX_WORDS))
    for i, fr in enumerate(got):
        assert _same(recs[fr.seq], want[False, False][i]), i
    by = _cut_by(_case(False)[0])
    assert by[0] + 1 < by[1] and by[2] + 1 < by[3]
    off_behind, on_behind = by[0], by[2]  # off behind the packet that cuts frame 0, on again behind the one that cuts frame 2

    def switch(ing, i):
        if i == off_behind:
            ing.set_record_output(False)
        if i == on_behind:
            ing.set_record_output(True, True, MAX_WORDS)
    got, recs = _run(False, lambda ing: ing.set_record_output(True, False, MAX_WORDS), switch)
    assert len(got) == len(frames)
    kinds = [None if recs[fr.seq] is None else [v for v in (True, False) if _same(recs[fr.seq], want[False, v][i])] for i, fr in enumerate(got)]
    assert kinds == [[False], None, None, [True], [True]], kinds  # a frame has the setting its cutting packet was pushed under


def test_a_frame_event_filter_does_not_change_the_record(want):
    frames = _case(False)[1]

    def setup(ing):
        ing.set_record_output(True, True, MAX_WORDS)
        ing.set_frame_filter(R.LAST_PER_XY, False)
    got, recs = _run(False, setup)
    assert len(got) == len(frames)
    for i, fr in enumerate(got):
        assert fr.n_kept < fr.n_events == len(frames[i]), i  # the filter ran
        assert _same(recs[fr.seq], want[False, True][i]), i    # ... behind the record stage: the cut frame's words


def test_overflow_is_all_or_nothing(want):
    frames = _case(False)[1]
    n_words = sorted(int(st.n_words) for _, st in want[False, True])
    small = n_words[2]  # three frames fit, two do not
    assert n_words[2] < n_words[3]
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        with pytest.raises(ValueError):
            ing.set_record_output(True, True, 0)  # max_words > 0 is required
        ing.set_record_output(True, True, small)
        with pytest.raises(ValueError, match=f"the record ring holds 16 entries of {small} words since the first call that switched the stage on"):
            ing.set_record_output(True, True, small + 1)  # fixed by the first call that switched the stage on
        with pytest.raises(ValueError):
            ing.set_record_output(True, True, small, ring=4)
        for p in _case(False)[0]:
            ing.push(p)
        ing.flush()
        got = ing.poll()
        assert len(got) == len(frames)
        fits = 0
        for i, fr in enumerate(got):
            rec = ing.record(fr.seq)
            assert rec is not None and _stats(rec[1]) == _stats(want[False, True][i][1]), i  # the true n_words either way
            if rec[1].n_words <= small:
                assert np.array_equal(rec[0], want[False, True][i][0]), i
                fits += 1
            else:
                assert rec[0] is None, i
                # the C entry: 1, the statistics, and not one word copied
                import ctypes as C
                from x_maps_amd import _native as N
                dst = np.full(small + 8, 0xBEEF, np.uint16)
                st = N.xm_evt3_record_stats()
                assert ing._lib.xm_ingest_copy_record(ing._g, fr.seq, C.c_void_p(dst.ctypes.data), N.XM_MEM_HOST, C.byref(st)) == 1
                assert st.n_words == rec[1].n_words > small and (dst == 0xBEEF).all(), i
        assert fits == 3


def test_a_ring_of_two_is_lapped_and_reset_keeps_the_setting(want):
    packets, frames = _case(False)
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=False, **INGEST) as ing:
        ing.set_record_output(True, True, MAX_WORDS, ring=2)
        seqs = []
        for rnd in range(2):
            for p in packets:
                ing.push(p)
            ing.flush()
            got = ing.poll()
            assert len(got) == len(frames)
            held = [ing.record(fr.seq) for fr in got]
            assert [h is not None for h in held] == [False, False, False, True, True], rnd  # five frames through a ring of two
            for i in (3, 4):
                assert _same(held[i], want[False, True][i]), (rnd, i)
            assert ing.record(got[-1].seq + 1) is None and ing.record(got[-1].seq + 12) is None  # never produced
            seqs += [fr.seq for fr in got]
            ing.reset()  # keeps the setting, drops the ring's contents
            assert all(ing.record(s) is None for s in seqs), rnd
        assert seqs == list(range(10))
