"""CPU: the DAT host decoder (x_maps_amd/dat.py) against hand-derived records and against the independent record-by-record
checker (tests/dat_ref.py), whole and in chunks; encoder round trip across the 32-bit clock's end; files and the header rules.
(Metavision's reader is closed: parity against it is unpinned)"""
import numpy as np
import pytest

import dat_ref as DR
from x_maps_amd import dat
from x_maps_amd import synthetic as S


def rec(ts, x, y, p):
    return (ts, x | (y << 14) | (p << 28))


def records(pairs):
    return np.array(pairs, dtype=dat.DAT_DTYPE)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("x", "y", "p", "t"))


def _tuples(evs):
    return [(int(e["x"]), int(e["y"]), int(e["p"]), int(e["t"])) for e in evs]


# (records, expected (x, y, p, t) tuples), derived by hand from the format description
HAND = [
    ([rec(5, 10, 20, 1)], [(10, 20, 1, 5)]),
    # the largest coordinates; p is the four top bits as they stand; both polarities
    ([rec(0, 0, 0, 0), rec(7, 16383, 16383, 1), rec(8, 1, 2, 15)], [(0, 0, 0, 0), (16383, 16383, 1, 7), (1, 2, 15, 8)]),
    # a small step BACK is kept as it is; one of more than 2^31 is a loop = 2^32 us more
    ([rec(1000, 1, 1, 1), rec(900, 2, 2, 1), rec(0xFFFFFFFF, 3, 3, 0), rec(3, 4, 4, 1)],
     [(1, 1, 1, 1000), (2, 2, 1, 900), (3, 3, 0, 0xFFFFFFFF), (4, 4, 1, (1 << 32) + 3)]),
    # exactly 2^31 back is not a loop, 2^31 + 1 is
    ([rec(1 << 31, 0, 0, 1), rec(0, 0, 0, 1), rec((1 << 31) + 1, 0, 0, 1), rec(0, 0, 0, 1)],
     [(0, 0, 1, 1 << 31), (0, 0, 1, 0), (0, 0, 1, (1 << 31) + 1), (0, 0, 1, 1 << 32)]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_derived_records(case):
    pairs, want = HAND[case]
    r = records(pairs)
    assert _tuples(dat.decode_dat(r)) == want and _tuples(DR.decode(r)) == want
    assert _tuples(dat.decode_dat(r.view("<u8"))) == want  # (the same 8 bytes as 64-bit words: ts is the low half)


def random_records(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, n, dtype=np.uint64).astype("<u8")


def test_uniformly_random_records_whole_and_chunked():
    r = random_records(20_000, 31)
    ref = DR.decode(r)
    assert len(ref) == len(r) and int(ref["t"].max()) >> 32 > 1000  # a loop wherever the stamp falls far enough
    assert _same(dat.decode_dat(r), ref)
    rng = np.random.default_rng(6)
    dec, sm = dat.DatDecoder(), DR.DatStateMachine()
    cuts = np.sort(rng.integers(0, len(r) + 1, 12))
    for a, b in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [len(r)]))):
        assert _same(dec.decode(r[a:b]), sm.feed(r[a:b])), (a, b)
    assert (dec.last_ts, dec.t_loops) == (sm.last_ts, sm.loops)


def stream(n, t0, seed, span=1 << 14):
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["t"] = t0 + np.sort(rng.integers(0, span, n))
    ev["x"], ev["y"], ev["p"] = rng.integers(0, 1280, n), rng.integers(0, 720, n), rng.integers(0, 2, n)
    return ev


@pytest.mark.parametrize("t0", [1000, (1 << 32) - 5000, (1 << 32) - (1 << 13)])
def test_encoder_round_trip(t0):
    ev = stream(6000, t0, seed=3)
    if t0 > 1000:
        assert ev["t"][0] < (1 << 32) <= ev["t"][-1]  # the stream crosses the 32-bit clock's end
    r = dat.encode_dat(ev)
    assert r.dtype == dat.DAT_DTYPE and len(r) == len(ev)
    assert _same(dat.decode_dat(r), ev) and _same(DR.decode(r), ev)


def test_empty_chunks_keep_the_state():
    dec = dat.DatDecoder()
    assert len(dec.decode(records([]))) == 0
    assert _tuples(dec.decode(records([rec(0xFFFFFFF0, 1, 1, 1)]))) == [(1, 1, 1, 0xFFFFFFF0)]
    assert len(dec.decode(np.zeros(0, "<u8"))) == 0
    assert _tuples(dec.decode(records([rec(2, 1, 1, 1)]))) == [(1, 1, 1, (1 << 32) + 2)]  # the loop is seen across the chunks


def test_file_round_trip(tmp_path):
    ev = stream(3000, 5000, seed=2)
    p = tmp_path / "rec.dat"
    dat.write_raw(str(p), ev, width=1280, height=720)
    got = list(dat.read_raw(str(p), chunk_words=700))
    cat = np.zeros(sum(len(g) for g in got), S.EVENT_CD_DTYPE)
    o = 0
    for g in got:
        cat[o:o + len(g)] = g
        o += len(g)
    assert len(got) > 1 and _same(cat, ev)
    chunks = list(dat.read_raw_words(str(p), chunk_words=512))
    assert all(c.dtype == dat.DAT_DTYPE for c in chunks) and np.array_equal(np.concatenate(chunks), dat.encode_dat(ev))
    blob = open(p, "rb").read()
    fields, off = dat.split_dat_header(blob)
    assert (fields["Version"], fields["Height"], fields["Width"]) == ("2", "720", "1280") and blob[off - 2:off] == b"\x0c\x08"
    assert dat.is_dat(str(p)) and dat.is_dat("x.DAT", {}) and dat.is_dat("x.raw", fields) and not dat.is_dat("x.raw", {"evt": "3.0"})


@pytest.mark.parametrize("header, tail, field", [
    (b"% Version 1\n% Height 480\n% Width 640\n", b"\x0c\x08", "Version"),
    (b"% Height 480\n% Width 640\n", b"\x0c\x08", "Version"),
    (b"% Version 2\n% Height 480\n% Width 640\n", b"\x00\x08", "event type"),
    (b"% Version 2\n% Height 480\n% Width 640\n", b"\x0c\x10", "event size"),
    (b"% Version 2\n", b"\x0c", "event type"),
])
def test_rejected_variants_name_the_file_and_the_field(tmp_path, header, tail, field):
    p = tmp_path / "bad.dat"
    with open(p, "wb") as f:
        f.write(header + tail + dat.encode_dat(stream(10, 0, 1)).tobytes()[:0 if len(tail) < 2 else None])
    with pytest.raises(ValueError) as e:
        list(dat.read_raw_words(str(p)))
    assert "bad.dat" in str(e.value) and field in str(e.value)
