"""-m gpu: the EXT_TRIGGER words of a recording as trigger records on the device (csrc/xmaps_exttrigger.hpp: two launches behind the
decoder's emit kernel) against the independent word-by-word checker (tests/ext_trigger_ref.py), on each of the three encodings,
bit for bit: the records, and the decoded events, which must be what the decoder gives with extraction off.  The streams are
tests/ext_trigger_cases.py's (tests/test_ext_trigger_cpu.py asserts that they hold what they are for)."""
import numpy as np
import pytest

import ext_trigger_cases as K
import ext_trigger_ref as R
from x_maps_amd import XMapsEngine, dat, evt2, evt21, evt3
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
MAX_WORDS = K.BIG


@pytest.fixture(scope="module")
def eng():
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


def _decoder(eng, fmt, max_words=MAX_WORDS, max_events=0, wait_for_time_base=False, legacy_halves=False):
    if fmt == 3:
        return evt3.DeviceEvt3Decoder(eng, max_words, max_events, wait_for_time_base)
    if fmt == 2:
        return evt2.DeviceEvt2Decoder(eng, max_words, max_events, wait_for_time_base)
    return evt21.DeviceEvt21Decoder(eng, max_words, max_events, wait_for_time_base, legacy_halves)


def _decode(eng, dec, words):
    ptr, n = dec.decode_device(words)
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    if n:
        eng.dev_download(ev, ptr)
    return ev


@pytest.fixture(scope="module")
def decoders(eng):
    """per (fmt, options): a decoder with extraction on and one with it off, made once (reset per case)"""
    made = {}

    def get(fmt, opt):
        key = (fmt, tuple(sorted(opt.items())))
        if key not in made:
            on, off = _decoder(eng, fmt, **opt), _decoder(eng, fmt, **opt)
            on.set_ext_triggers(1 << 12)
            made[key] = (on, off)
        on, off = made[key]
        on.reset()
        off.reset()
        return on, off
    yield get
    for on, off in made.values():
        on.close()
        off.close()


def _run_cases(eng, decoders, cases):
    n_trig = 0
    for name, fmt, chunks, opt in cases:
        on, off = decoders(fmt, opt)
        ref = R.machine(fmt, **opt)
        for i, c in enumerate(chunks):
            ev_r, tr_r = ref.feed(c)
            ev = _decode(eng, on, c)
            tr = on.last_ext_triggers()
            assert tr.tobytes() == tr_r.tobytes(), (name, i, len(tr), len(tr_r))
            assert ev.tobytes() == ev_r.tobytes(), (name, i)
            assert _decode(eng, off, c).tobytes() == ev.tobytes(), (name, i)
            assert len(off.last_ext_triggers()) == 0
            n_trig += len(tr)
    return n_trig


@pytest.mark.parametrize("fmt", K.FMTS)
def test_chunk_sizes(eng, decoders, fmt):
    assert _run_cases(eng, decoders, K.sized_cases(fmt)) > 250


@pytest.mark.parametrize("fmt", K.FMTS)
def test_word_level_cases(eng, decoders, fmt):
    assert _run_cases(eng, decoders, K.small_cases(fmt)) > 300


@pytest.mark.parametrize("fmt", K.FMTS)
def test_split_at_every_position_around_a_trigger(eng, decoders, fmt):
    cases = K.split_cases(fmt)
    _run_cases(eng, decoders, cases)
    # ... and the pieces give the whole stream's result: records with the first piece's events added to the second piece's indices
    whole = R.decode(cases[0][2][0], fmt)
    on, _ = decoders(fmt, {})
    for name, _, (a, b), _ in cases[1::9]:
        on.reset()
        ev_a = _decode(eng, on, a)
        tr_a = on.last_ext_triggers().copy()
        ev_b = _decode(eng, on, b)
        tr_b = on.last_ext_triggers().copy()
        tr_b["event_index"] += len(ev_a)
        assert ev_a.tobytes() + ev_b.tobytes() == whole[0].tobytes(), name
        assert tr_a.tobytes() + tr_b.tobytes() == whole[1].tobytes(), name


@pytest.mark.parametrize("fmt", K.FMTS)
def test_too_many_triggers_leave_the_state_unchanged(eng, fmt):
    rng = np.random.default_rng(fmt)
    w = K.random_words(fmt, 3000, rng)
    w = w[~K.is_trigger(fmt, w)]
    at = np.sort(rng.choice(len(w), 65, replace=False))
    w[at] = K.arr(fmt, [K.trig(fmt, i % 16, i & 1, i % 64) for i in range(65)])
    want_ev, want_tr = R.decode(w, fmt)
    with _decoder(eng, fmt, max_words=4096) as dec:
        dec.set_ext_triggers(64)
        head = K.random_words(fmt, 500, rng, trig_rate=0.01)  # (a stream in front: the state the refused chunk must leave alone)
        ref = R.machine(fmt)
        ref.feed(head)
        _decode(eng, dec, head)
        before = dec.last_ext_triggers().copy()
        with pytest.raises(N.XMapsTooMany):
            dec.decode_device(w)
        assert dec.last_ext_triggers().tobytes() == before.tobytes()  # (the records of the last SUCCESSFUL decode)
        half = len(w) // 2
        ev_a, tr_a = ref.feed(w[:half])
        ev_b, tr_b = ref.feed(w[half:])
        got_a = _decode(eng, dec, w[:half])
        rec_a = dec.last_ext_triggers().copy()
        got_b = _decode(eng, dec, w[half:])
        rec_b = dec.last_ext_triggers().copy()
        assert got_a.tobytes() == ev_a.tobytes() and got_b.tobytes() == ev_b.tobytes()
        assert rec_a.tobytes() == tr_a.tobytes() and rec_b.tobytes() == tr_b.tobytes()
        assert len(rec_a) + len(rec_b) == 65 == len(want_tr) and len(want_ev) == len(ev_a) + len(ev_b)
        # exactly max_triggers fit
        dec.reset()
        keep = np.ones(len(w), bool)
        keep[at[-1]] = False
        _decode(eng, dec, w[keep])
        assert len(dec.last_ext_triggers()) == 64


@pytest.mark.parametrize("fmt", K.FMTS)
def test_extraction_off_reset_and_empty_chunk(eng, fmt):
    w = K.arr(fmt, [K.th(fmt, 4), K.trig(fmt, 1, 1, 2), K.cd(fmt, 3, 3, 1), K.trig(fmt, 2, 0, 5)])
    with _decoder(eng, fmt, max_words=64) as dec:
        _decode(eng, dec, w)
        assert len(dec.last_ext_triggers()) == 0  # off by default
        dec.set_ext_triggers(16)
        dec.reset()
        _decode(eng, dec, w)
        assert dec.last_ext_triggers()["id"].tolist() == [1, 2]
        _decode(eng, dec, w[:0])
        assert len(dec.last_ext_triggers()) == 0  # an empty chunk
        _decode(eng, dec, w)
        assert len(dec.last_ext_triggers()) == 2
        dec.reset()
        assert len(dec.last_ext_triggers()) == 0
        _decode(eng, dec, w)
        dec.set_ext_triggers(0)
        assert len(dec.last_ext_triggers()) == 0
        _decode(eng, dec, w)
        assert len(dec.last_ext_triggers()) == 0


def test_a_dat_decoder_is_refused(eng):
    with dat.DeviceDatDecoder(eng, max_words=64) as dec:
        with pytest.raises(ValueError):
            dec.set_ext_triggers(16)
        assert len(dec.last_ext_triggers()) == 0
