"""CPU: the EVT 2.1 host decoder (x_maps_amd/evt21.py: forward fills over the whole buffer, the masks expanded by popcount) against
hand-derived word sequences and against the independent word-by-word state machine (tests/evt21_ref.py), whole and in chunks;
encoder round trip with and without vectors; legacy half order; RAW files and the header rules.  (Metavision's reader is closed:
parity against it is unpinned)"""
import importlib.util
import os

import numpy as np
import pytest

import evt21_ref as ER
from x_maps_amd import evt2, evt21, evt3
from x_maps_amd import synthetic as S


def vec(p, t6, x_base, y, valid):
    return (p << 60) | (t6 << 54) | (x_base << 43) | (y << 32) | valid


def th(v, low=0):
    return (0x8 << 60) | (v << 32) | low


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("x", "y", "p", "t"))


def _tuples(evs):
    return [(int(e["x"]), int(e["y"]), int(e["p"]), int(e["t"])) for e in evs]


# (words, expected (x, y, p, t) tuples), derived by hand from the format description
HAND = [
    # a mask with bits 0 and 31: the first and the last column of the word; time base 3 -> t = 3 * 64 + 5
    ([th(3), vec(1, 5, 64, 20, 0x80000001)], [(64, 20, 1, 197), (95, 20, 1, 197)]),
    # a zero mask is no event at all
    ([th(1), vec(1, 0, 32, 7, 0), vec(0, 2, 32, 7, 0b100)], [(34, 7, 0, 66)]),
    # an all-ones mask: 32 events in ascending column order
    ([th(2), vec(0, 1, 0, 9, 0xFFFFFFFF)], [(n, 9, 0, 129) for n in range(32)]),
    # x_base need not be a multiple of 32: x_base + n as it stands, up to 2047 + 31; the largest row and low field
    ([th(0), vec(1, 63, 2047, 2047, 0x80000001), vec(0, 0, 5, 1, 0b1010)],
     [(2047, 2047, 1, 63), (2078, 2047, 1, 63), (6, 1, 0, 0), (8, 1, 0, 0)]),
    # both polarities, an EVT_TIME_HIGH between two vector words (whose low 32 bits are ignored)
    ([th(1), vec(1, 1, 32, 1, 0b11), th(2, 0xDEADBEEF), vec(0, 1, 32, 1, 0b11)],
     [(32, 1, 1, 65), (33, 1, 1, 65), (32, 1, 0, 129), (33, 1, 0, 129)]),
    # triggers / vendor / continued words and unknown types are skipped, whatever their low halves hold
    ([th(1), (0xA << 60) | 0x123456789, vec(1, 2, 0, 0, 1), (0xE << 60) | 0xFFFFFFFF, (0xF << 60) | 0xFFFFFFFF,
      (0x3 << 60) | 0xFFFFFFFF, (0x9 << 60) | (5 << 32), vec(1, 3, 0, 0, 2)], [(0, 0, 1, 66), (1, 0, 1, 67)]),
    # the 28-bit field wraps: 0x0fffffff -> 0 is one loop = 2^34 us more; a small step back is not one
    ([th(0x0FFFFFFF), vec(1, 63, 0, 2, 1), th(0), vec(1, 0, 0, 4, 0b110), th(100), vec(0, 0, 0, 0, 1), th(99), vec(0, 0, 0, 0, 1)],
     [(0, 2, 1, (0x0FFFFFFF << 6) | 63), (1, 4, 1, 1 << 34), (2, 4, 1, 1 << 34), (0, 0, 0, (1 << 34) + 6400), (0, 0, 0, (1 << 34) + 6336)]),
]
# events in front of the first EVT_TIME_HIGH: (words, expected with the time base at its initial 0, expected with wait_for_time_base)
HAND_WAIT = [
    ([vec(1, 5, 0, 3, 0b101), vec(0, 6, 32, 3, 0), th(4), vec(1, 0, 0, 3, 1)],
     [(0, 3, 1, 5), (2, 3, 1, 5), (0, 3, 1, 256)], [(0, 3, 1, 256)]),
    ([vec(1, 1, 0, 0, 0xFFFFFFFF)], [(n, 0, 1, 1) for n in range(32)], []),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_derived_sequences(case):
    words, want = HAND[case]
    w = np.array(words, dtype="<u8")
    assert _tuples(evt21.decode_evt21(w)) == want
    assert _tuples(ER.decode(w)) == want


@pytest.mark.parametrize("case", range(len(HAND_WAIT)))
def test_events_in_front_of_the_first_time_high(case):
    words, want_off, want_on = HAND_WAIT[case]
    w = np.array(words, dtype="<u8")
    for wait, want in ((False, want_off), (True, want_on)):
        assert _tuples(evt21.decode_evt21(w, wait_for_time_base=wait)) == want
        assert _tuples(ER.decode(w, wait_for_time_base=wait)) == want


def random_words(n, seed):
    """uniformly random 64-bit words: every type, masks of ~16 bits, EVT_TIME_HIGH values all over their 28 bits"""
    return np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64).astype("<u8")


@pytest.mark.parametrize("wait", [False, True])
def test_uniformly_random_words_whole_and_chunked(wait):
    w = random_words(20_000, 21)
    ref = ER.decode(w, wait_for_time_base=wait)
    assert len(ref) > 30_000 and int(ref["t"].max()) >> 34 > 10  # vector words of many events, many loops
    assert _same(evt21.decode_evt21(w, wait_for_time_base=wait), ref)
    rng = np.random.default_rng(5)
    dec, sm = evt21.Evt21Decoder(wait), ER.Evt21StateMachine(wait)
    cuts = np.sort(rng.integers(0, len(w) + 1, 12))
    for a, b in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [len(w)]))):
        assert _same(dec.decode(w[a:b]), sm.feed(w[a:b])), (a, b)
    assert (dec.t_high, dec.t_loops) == (sm.time_high, sm.loops)


def clustered_events(n, t0, seed, span=1 << 14):
    """time-ordered events in runs that share (t, y, p) with rising columns -- what the encoder merges into vector words"""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    run = np.cumsum(rng.random(n) < 0.2)  # a new run with probability 0.2
    n_runs = int(run[-1]) + 1
    ev["t"] = (t0 + np.sort(rng.integers(0, span, n_runs)))[run]
    ev["y"] = rng.integers(0, 720, n_runs)[run]
    ev["p"] = rng.integers(0, 2, n_runs)[run]
    x0 = rng.integers(0, 1200, n_runs)[run]
    first = np.concatenate(([True], run[1:] != run[:-1]))
    step = np.where(first, 0, rng.integers(1, 4, n))
    pos = np.cumsum(step)
    ev["x"] = x0 + pos - np.maximum.accumulate(np.where(first, pos, 0))
    return ev


@pytest.mark.parametrize("use_vectors", [True, False])
@pytest.mark.parametrize("t0", [1000, (1 << 34) - 5000, (1 << 34) - (1 << 13)])
def test_encoder_round_trip(use_vectors, t0):
    ev = clustered_events(6000, t0, seed=3)
    if t0 > 1000:
        assert ev["t"][0] < (1 << 34) <= ev["t"][-1]  # the stream crosses the 34-bit clock's end
    for every in (0, 16, 1000):
        w = evt21.encode_evt21(ev, use_vectors=use_vectors, time_high_every_us=every)
        assert _same(evt21.decode_evt21(w), ev) and _same(ER.decode(w), ev)
    cd = w[(w >> np.uint64(60)) <= 1]
    per_word = np.array([bin(int(m)).count("1") for m in cd & np.uint64(0xFFFFFFFF)])
    assert per_word.sum() == len(ev)
    assert (per_word.max() > 3 and len(cd) < len(ev) // 2) if use_vectors else (per_word.max() == 1 and len(cd) == len(ev))


def test_legacy_halves():
    ev = clustered_events(3000, 77, seed=8)
    w = evt21.encode_evt21(ev)
    sw = evt21.swap_halves(w)
    assert not np.array_equal(sw, w) and np.array_equal(evt21.swap_halves(sw), w)
    assert np.array_equal(sw.view("<u4")[0::2], w.view("<u4")[1::2])  # the HIGH half is stored first
    assert _same(evt21.decode_evt21(sw, legacy_halves=True), ev) and _same(ER.decode(sw, legacy_halves=True), ev)
    r = random_words(5000, 4)
    assert _same(evt21.decode_evt21(evt21.swap_halves(r), legacy_halves=True), ER.decode(r))
    dec, sm = evt21.Evt21Decoder(legacy_halves=True), ER.Evt21StateMachine()
    for a in range(0, len(r), 777):
        assert _same(dec.decode(evt21.swap_halves(r[a:a + 777])), sm.feed(r[a:a + 777]))


def test_empty_and_eventless_chunks():
    dec = evt21.Evt21Decoder()
    assert len(dec.decode(np.zeros(0, "<u8"))) == 0
    assert len(dec.decode(np.array([th(7), 0xE << 60, vec(1, 0, 0, 0, 0)], "<u8"))) == 0 and dec.t_high == 7
    assert _tuples(dec.decode(np.array([vec(1, 1, 2, 3, 1)], "<u8"))) == [(2, 3, 1, 7 * 64 + 1)]  # the base survives chunks without events
    assert len(evt21.encode_evt21(np.zeros(0, S.EVENT_CD_DTYPE))) == 0


def _cat(parts):
    out = np.zeros(sum(len(p) for p in parts), S.EVENT_CD_DTYPE)
    o = 0
    for p in parts:
        out[o:o + len(p)] = p
        o += len(p)
    return out


@pytest.mark.parametrize("legacy", [False, True])
def test_raw_file_round_trip(tmp_path, legacy):
    ev = clustered_events(3000, 5000, seed=2)
    p = tmp_path / "rec21.raw"
    evt21.write_raw(str(p), ev, width=1280, height=720, legacy_halves=legacy)
    assert evt21.raw_legacy_halves(str(p)) == legacy
    got = list(evt21.read_raw(str(p), chunk_words=300))
    assert len(got) > 1 and _same(_cat(got), ev)
    words = np.concatenate(list(evt21.read_raw_words(str(p), chunk_words=512)))
    want = evt21.encode_evt21(ev)
    assert np.array_equal(words, evt21.swap_halves(want) if legacy else want)  # as the file stores them


def test_header_rules(tmp_path):
    ev = clustered_events(500, 5000, seed=1)
    assert evt21.header_legacy_halves({"format": "EVT21;height=720;width=1280;endianness=legacy"})
    assert not evt21.header_legacy_halves({"format": "EVT21;height=720;width=1280;endianness=little"})
    assert not evt21.header_legacy_halves({"format": "EVT21;height=720;width=1280"}) and not evt21.header_legacy_halves({"evt": "2.1"})
    for fields in ({"evt": "2.1"}, {"format": "EVT21;height=720;width=1280"}, {"format": "evt2.1"}):
        assert evt21._is_evt21(fields) and not evt2._is_evt2(fields)
    assert not evt21._is_evt21({"evt": "2.0"}) and not evt21._is_evt21({"evt": "3.0"}) and not evt21._is_evt21({})
    p21, p2, p3 = (tmp_path / n for n in ("rec21.raw", "rec2.raw", "rec3.raw"))
    evt21.write_raw(str(p21), ev)
    evt2.write_raw(str(p2), ev)
    evt3.write_raw(str(p3), ev)
    with pytest.raises(ValueError, match="EVT 3.0"):  # each reader refuses the other encodings and says which one the file holds
        list(evt3.read_raw(str(p21)))
    with pytest.raises(ValueError, match="EVT 2.0"):
        list(evt2.read_raw(str(p21)))
    for other in (p2, p3):
        with pytest.raises(ValueError, match="EVT 2.1"):
            list(evt21.read_raw(str(other)))


def tool():
    spec = importlib.util.spec_from_file_location(
        "run_esl_on_arrival", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_esl_on_arrival.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_picks_the_decoder_from_the_header(tmp_path):
    from x_maps_amd import dat
    t = tool()
    ev = clustered_events(200, 5000, seed=1)
    paths = {k: str(tmp_path / n) for k, n in ((3, "a.raw"), (2, "b.raw"), (21, "c.raw"), ("dat", "d.dat"))}
    evt3.write_raw(paths[3], ev)
    evt2.write_raw(paths[2], ev)
    evt21.write_raw(paths[21], ev)
    dat.write_raw(paths["dat"], ev)
    for k, p in paths.items():
        assert t.raw_format(p) == k
    renamed = str(tmp_path / "e.raw")  # a DAT file under another suffix: its header fields decide
    dat.write_raw(renamed, ev)
    assert t.raw_format(renamed) == "dat"
    bare = str(tmp_path / "f.raw")  # a header that names no encoding: EVT 3.0, as before
    with open(bare, "wb") as f:
        f.write(b"% geometry 640x480\n% end\n" + evt3.encode_evt3(ev).tobytes())
    assert t.raw_format(bare) == 3
    for line in (b"% evt 4.0\n% end\n", b"% format EVT9;height=720;width=1280\n% end\n"):
        unknown = str(tmp_path / "g.raw")
        with open(unknown, "wb") as f:
            f.write(line + evt21.encode_evt21(ev).tobytes())
        with pytest.raises(ValueError, match="4.0|EVT9"):  # named, never decoded as EVT 3.0
            t.raw_format(unknown)
