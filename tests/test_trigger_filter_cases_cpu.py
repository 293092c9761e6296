"""CPU: what the GPU tests of the triggered frames' two filters rely on (tests/trigger_filter_cases.py), pinned without a GPU --
stream A's counts under the activity rule, which chunking takes which path of the device's evaluation, the host form of the
append for an arbitrary keep mask (ext_trigger.keep_where) against literals, and that no case is vacuous."""
import numpy as np
import pytest

import ext_trigger_cases as K
import ingest_oracle as IO
import trigger_filter_cases as TC
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S
from x_maps_amd.evt3 import EXT_TRIGGER_DTYPE

CUT = dict(cap_events=1 << 22, id=0, edge="rising")


def _decoded(fmt, chunker):
    words, _ = TC.stream_a(fmt)
    return TC.decoded_chunks(fmt, chunker(words))


def test_stream_a_is_the_pipe_tests_stream():
    for fmt in K.FMTS:
        words, evs = TC.stream_a(fmt)
        (ev, tr), = TC.decoded_chunks(fmt, [words])
        assert ev.tobytes() == evs.tobytes() and int((evs["p"] == 1).sum()) == TC.N_POSITIVE
        assert len(evs) == sum(TC.N_EVENTS) and abs((evs["p"] != 1).mean() - 0.2) < 0.02
        sel = tr[(tr["id"] == 0) & (tr["value"] == 1)]
        assert sel["event_index"].tolist() == np.concatenate(([0], np.cumsum(TC.N_EVENTS))).tolist()  # a trigger at every frame start


@pytest.mark.parametrize("thresh", sorted(TC.TABLE))
def test_stream_a_under_the_activity_rule(thresh):
    kept_all, per_frame, shown, skipped = TC.TABLE[thresh]
    dec = _decoded(3, TC.one_chunk)
    every = TC.expected(dec, thresh, min_events=0, **CUT)
    assert every["n_positive"] == TC.N_POSITIVE
    if kept_all is not None:
        assert every["n_active"] == kept_all
    if per_frame is not None:
        assert tuple(len(f) for f, _ in every["frames"]) == per_frame and sum(per_frame) == every["n_active"]
        cut = TC.expected(dec, thresh, min_events=TC.MIN_EVENTS, **CUT)["cutter"].stats
        assert (cut["frames_cut"], cut["frames_skipped"]) == (shown, skipped)
    # not vacuous: the rule drops at least a tenth and keeps at least a tenth of the positive events -- at T = 16 666 of the
    # stream's first frame, which has no history in front of it
    if thresh == 16_666:
        first = TC.expected(dec, None, min_events=0, **CUT)["frames"][0][0]
        kept_first = len(every["frames"][0][0])
        assert 0.10 <= 1 - kept_first / len(first) <= 0.9 and round(100 * (1 - kept_first / len(first))) == 15
    else:
        assert 0.10 <= every["n_active"] / TC.N_POSITIVE <= 0.90
    if thresh == 500:
        assert round(100 * (1 - every["n_active"] / TC.N_POSITIVE)) == 24
    if thresh == 200:  # the frame of 991 is skipped only because min_events applies behind the filter
        assert per_frame[1] == 991 <= TC.MIN_EVENTS < TC.expected(dec, None, min_events=0, **CUT)["frames"][1][0].shape[0]


def test_the_oracles_agree_and_include_self_is_another_rule():
    dec = _decoded(2, TC.uneven_chunks)
    a = TC.expected(dec, 500, min_events=0, **CUT)
    b = TC.expected(dec, 500, c_form=True, min_events=0, **CUT)
    c = TC.expected(dec, 500, include_self=True, min_events=0, **CUT)
    assert [f.tobytes() for f, _ in a["frames"]] == [f.tobytes() for f, _ in b["frames"]]
    assert c["n_active"] > a["n_active"] and 0.1 <= c["n_active"] / TC.N_POSITIVE <= 0.9


@pytest.mark.parametrize("fmt", K.FMTS)
def test_which_chunking_takes_which_path(fmt):
    words, _ = TC.stream_a(fmt)
    seq = lambda chunks, T: [TC.takes_sequential_path(ev, T) for ev, _ in TC.decoded_chunks(fmt, chunks)]  # noqa: E731
    assert seq(TC.one_chunk(words), 500) == [True]  # 96 ms in one chunk: 192 buckets
    short = TC.chunks_spanning_under(words, fmt, 4000)
    assert len(short) > 20 and np.concatenate(short).tobytes() == words.tobytes()
    spans = [int(ev["t"].max() - ev["t"].min()) for ev, _ in TC.decoded_chunks(fmt, short) if len(ev)]
    assert max(spans) < 4000 and max(spans) > 3000
    assert not any(seq(short, 500))
    for chunker in (TC.one_chunk, TC.uneven_chunks):
        assert not any(seq(chunker(words), 16_666))  # (the whole stream is 96 ms: under 8 buckets of 16.667 ms)
    assert sum(seq(TC.uneven_chunks(words), 500)) == 4  # (the one-word chunk is the parallel one)


def test_the_proviso_on_literals():
    def ev(ts):
        e = np.zeros(len(ts), S.EVENT_CD_DTYPE)
        e["t"] = ts
        return e
    T = 99  # buckets of 100 us
    assert not TC.takes_sequential_path(ev([]), T)
    assert not TC.takes_sequential_path(ev([1000, 1099, 1100, 1799]), T)
    assert TC.takes_sequential_path(ev([1000, 1800]), T)             # the ninth bucket
    assert TC.takes_sequential_path(ev([1000, 999]), T)              # in front of the chunk's first stamp
    assert not TC.takes_sequential_path(ev([1000, 1150, 1101]), T)   # backwards inside a bucket
    assert TC.takes_sequential_path(ev([1000, 1100, 1099]), T)       # backwards by a bucket


def _ev(ps):
    e = np.zeros(len(ps), S.EVENT_CD_DTYPE)
    e["p"] = ps
    e["x"] = np.arange(len(ps))
    e["t"] = 100 + np.arange(len(ps))
    return e


def _tr(idx):
    t = np.zeros(len(idx), EXT_TRIGGER_DTYPE)
    t["event_index"] = idx
    t["value"] = 1
    return t


def test_keep_where_against_literals():
    ev = _ev([1, 1, 1, 1, 1, 1])
    #        keep:  0  1  0  0  1  1
    mask = [False, True, False, False, True, True]
    kept, tr = X.keep_where(ev, _tr([0, 1, 2, 3, 4, 5, 6, 9]), mask)
    assert kept["x"].tolist() == [1, 4, 5]
    # in front of a dropped record (0), in front of a kept one (1), between dropped ones (2, 3), behind them (4), the end (6), past it (9)
    assert tr["event_index"].tolist() == [0, 0, 1, 1, 1, 2, 3, 3]
    kept, tr = X.keep_where(ev, _tr([0, 3, 6]), np.zeros(6, bool))  # an all-dropped chunk
    assert len(kept) == 0 and kept.dtype == S.EVENT_CD_DTYPE and tr["event_index"].tolist() == [0, 0, 0]
    kept, tr = X.keep_where(_ev([]), _tr([0, 0]), np.zeros(0, bool))  # an empty chunk
    assert len(kept) == 0 and tr["event_index"].tolist() == [0, 0]
    kept, tr = X.keep_where(ev, _tr([]), np.ones(6, bool))
    assert kept.tobytes() == ev.tobytes() and len(tr) == 0
    with pytest.raises(ValueError):
        X.keep_where(ev, _tr([]), [True])


def test_keep_positive_is_keep_where_of_p_equal_1():
    rng = np.random.default_rng(3)
    ev = _ev(rng.integers(0, 2, 500))
    trg = _tr(np.sort(rng.integers(0, 501, 40)))
    a, ta = X.keep_positive(ev, trg)
    b, tb = X.keep_where(ev, trg, ev["p"] == 1)
    assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes() and 100 < len(a) < 400
    for fmt in K.FMTS:  # ... and on stream A, chunk by chunk
        for e, t in _decoded(fmt, TC.uneven_chunks):
            a, ta = X.keep_positive(e, t)
            assert ta["event_index"].tolist() == [int((e["p"][:i] == 1).sum()) for i in t["event_index"]]
            assert a.tobytes() == e[e["p"] == 1].tobytes()


def test_act_mask_marks_what_the_oracle_returns():
    (ev, _), = _decoded(3, TC.one_chunk)
    ev = ev.copy()
    ev["x"][[10, 20]] = 2047  # (EVT words can carry that: off the sensor, judged by nobody)
    mask, n_part = TC.act_mask(IO.ActivityFilterOracle(TC.CFG.cam_w, TC.CFG.cam_h, 500), ev)
    on = ev[(ev["p"] == 1) & (ev["x"] < TC.CFG.cam_w)]
    want = IO.ActivityFilterOracle(TC.CFG.cam_w, TC.CFG.cam_h, 500).process(on)
    assert n_part == len(on) and all(np.array_equal(ev[mask][k], want[k]) for k in ("x", "y", "p", "t"))  # (not the padding bytes)
    assert not mask[[10, 20]].any() and not mask[ev["p"] != 1].any()
