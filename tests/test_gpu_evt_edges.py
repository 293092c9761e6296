"""-m gpu: the device EVT 3.0 / EVT 2.0 decoders (csrc/xmaps_evt3.hpp, xmaps_evt2.hpp: three scan launches per chunk;
xmaps_evt.hpp: the block geometry, state record and block scan the two share) past the bound of the prefix kernels' carry loop.
Such a kernel walks the block aggregates THREADS (256) at a time and carries a combined record from trip to trip; one trip
covers 256 blocks x 2048 words = 524 288 words.  Every case here decodes ONE chunk longer than that (or exactly that long), so
the second trip, the state it leaves for the next chunk and the emit blocks whose prefix came out of it all run.  The reference
is the independent word-at-a-time checker (oracle/evt3_oracle.py, oracle/evt2_oracle.py) in one go; x, y, p, t and the event
count must be equal exactly.  Every case first asserts on the words themselves that the stream has what it is for.  (The
unmarked test at the end checks TRIP against the headers on the CPU.)"""
import functools
import os
import re

import numpy as np
import pytest

import evt2_oracle as EO2
import evt3_oracle as EO3
from x_maps_amd import evt2, evt3
from x_maps_amd import synthetic as S

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

THREADS, PER_BLOCK = 256, 2048  # EVT_THREADS, EVT_PER_BLOCK of csrc/xmaps_evt.hpp (checked at the end)
TRIP = THREADS * PER_BLOCK      # 524 288 words: what one trip of the prefix kernel's carry loop covers
N_PRE = 3000                    # event words in front of the stream's first time-high word (wait_for_time_base)

FORMATS = {3: (evt3.DeviceEvt3Decoder, EO3, "<u2", 12), 2: (evt2.DeviceEvt2Decoder, EO2, "<u4", 28)}  # class, oracle, dtype, type shift


@pytest.fixture(scope="module")
def eng():
    from x_maps_amd import XMapsEngine
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


def _random_events(rng, n, t_lo, t_hi):
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["t"] = np.sort(rng.integers(t_lo, t_hi, n))
    ev["x"], ev["y"], ev["p"] = rng.integers(0, 1280, n), rng.integers(0, 720, n), rng.integers(0, 2, n)
    return ev


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def _words(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "evt3_vectors":  # single and vector events, redundant TIME_HIGH words, skipped types, empty vectors
        from test_gpu_evt3 import _random_stream
        w = _random_stream(0, 300_000)
    elif name == "evt3_wraps":  # the 24-bit time base wraps at t = 2^24 and at t = 2^25
        w = evt3.encode_evt3(_random_events(rng, 262_000, (1 << 24) - (1 << 20), (1 << 25) + 400_000))
    elif name == "evt3_tail":  # 64 words behind a chunk: events that show every field of the state first, then any words
        w = np.concatenate((rng.choice([0x2, 0x4, 0x5], 32) << 12 | rng.integers(0, 4096, 32), rng.integers(0, 65536, 32))).astype("<u2")
    elif name == "evt3_pre":  # event words only (ADDR_X, VECT_12, VECT_8), no time word
        w = (rng.choice([0x2, 0x2, 0x4, 0x5], N_PRE) << 12 | rng.integers(0, 4096, N_PRE)).astype("<u2")
    elif name == "evt2_loops":  # the 28-bit time base loops at t = 2^34 and at t = 2^35
        w = evt2.encode_evt2(_random_events(rng, 270_000, (1 << 34) - (1 << 30), (1 << 35) + (1 << 28)))
    elif name == "evt2_arbitrary":
        w = rng.integers(0, 1 << 32, 526_000, dtype=np.uint64).astype("<u4")
    elif name == "evt2_tail":
        w = np.concatenate((rng.integers(0, 2, 32, dtype=np.uint64) << 28 | rng.integers(0, 1 << 28, 32, dtype=np.uint64),
                            rng.integers(0, 1 << 32, 32, dtype=np.uint64))).astype("<u4")
    elif name == "evt2_pre":  # CD words only
        w = (rng.integers(0, 2, N_PRE, dtype=np.uint64) << 28 | rng.integers(0, 1 << 28, N_PRE, dtype=np.uint64)).astype("<u4")
    return _frozen(w)


@functools.lru_cache(maxsize=None)
def _reference(fmt, name, stop=None, wait=False):
    """the oracle on _words(name)[:stop] in one go"""
    return _frozen(FORMATS[fmt][1].decode(_words(name)[:stop], wait))


def _typ(fmt, w):
    return w >> FORMATS[fmt][3]


def _wrap_positions(fmt, w):
    """index of every time-high word whose field falls back by more than half its range (the oracles' rule), from the words alone"""
    at = np.nonzero(_typ(fmt, w) == 0x8)[0]
    v = w[at].astype(np.int64) & ((1 << 12) - 1 if fmt == 3 else (1 << 28) - 1)
    return at[1:][v[:-1] - v[1:] > (0x800 if fmt == 3 else 1 << 27)]


def _assert_same(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k in ("x", "y", "p", "t"):
        assert np.array_equal(got[k], ref[k]), (what, k, int(np.flatnonzero(got[k] != ref[k])[0]))


def _one_chunk(eng, fmt, words, ref, wait=False):
    with FORMATS[fmt][0](eng, max_words=len(words), max_events=len(ref) + 64, wait_for_time_base=wait) as dec:
        ptr, n = dec.decode_device(words)  # (one call = one chunk)
        assert n == len(ref), (n, len(ref))
        got = np.zeros(n, S.EVENT_CD_DTYPE)
        eng.dev_download(got, ptr)
    return got


@gpu
def test_evt3_vectors_and_filler_past_one_trip(eng):
    w, ref = _words("evt3_vectors"), _reference(3, "evt3_vectors")
    vec = np.nonzero(np.isin(_typ(3, w), (0x4, 0x5)) & ((w & 0xfff) != 0))[0]
    assert len(w) > TRIP and len(ref) > 300_000 and (vec >= TRIP).sum() > 1000
    assert (_typ(3, w)[TRIP:] == 0x3).any() and np.isin(_typ(3, w)[TRIP:], (0x7, 0xA, 0xE, 0xF)).any()
    _assert_same(_one_chunk(eng, 3, w, ref), ref, "evt3_vectors")


@gpu
@pytest.mark.parametrize("fmt,name", [(3, "evt3_wraps"), (2, "evt2_loops")])
def test_a_wrap_of_the_time_base_on_each_side_of_the_trip(eng, fmt, name):
    w, ref = _words(name), _reference(fmt, name)
    wraps = _wrap_positions(fmt, w)
    assert len(w) > TRIP + PER_BLOCK and len(wraps) == 2 and wraps[0] < TRIP <= wraps[1], (len(w), wraps)
    assert int(ref["t"][-1]) >> (24 if fmt == 3 else 34) == 2  # (both are in the stamps)
    _assert_same(_one_chunk(eng, fmt, w, ref), ref, name)


@gpu
def test_evt2_arbitrary_words_past_one_trip(eng):
    w, ref = _words("evt2_arbitrary"), _reference(2, "evt2_arbitrary")
    assert len(w) == 526_000 > TRIP and (_typ(2, w)[TRIP:] <= 1).sum() > 100 and (_typ(2, w)[TRIP:] == 0x8).sum() > 50
    assert len(_wrap_positions(2, w)) > 1000 and (_wrap_positions(2, w) >= TRIP).any()
    _assert_same(_one_chunk(eng, 2, w, ref), ref, "evt2_arbitrary")


@gpu
@pytest.mark.parametrize("fmt,name", [(3, "evt3_wraps"), (2, "evt2_loops")])
@pytest.mark.parametrize("n", [TRIP, TRIP + 1])
def test_the_exact_edge_of_one_trip(eng, fmt, name, n):
    """TRIP words: a full single trip; TRIP + 1: a second trip of one block that holds one word"""
    w, ref = _words(name)[:n], _reference(fmt, name, n)
    assert len(w) == n and -(-n // PER_BLOCK) == THREADS + (n > TRIP) and 100_000 < len(ref) < len(_reference(fmt, name))
    _assert_same(_one_chunk(eng, fmt, w, ref), ref, (name, n))


@gpu
@pytest.mark.parametrize("fmt,name,tail", [(3, "evt3_wraps", "evt3_tail"), (2, "evt2_loops", "evt2_tail")])
def test_the_state_after_two_trips(eng, fmt, name, tail):
    """one decoder: the long stream in one chunk, then 64 more words; both chunks together == the oracle on all the words at once
    (the second chunk starts from the state the prefix kernel wrote after its second trip)"""
    w, t = _words(name), _words(tail)
    whole = FORMATS[fmt][1].decode(np.concatenate((w, t)))
    ref = _reference(fmt, name)
    # the tail starts with event words alone: their row, time and vector base are what the first chunk left
    assert len(w) > TRIP and len(t) == 64 and np.isin(_typ(fmt, t)[:32], (0x2, 0x4, 0x5) if fmt == 3 else (0, 1)).all()
    assert len(whole) >= len(ref) + 32
    assert np.array_equal(whole["t"][:len(ref)], ref["t"])
    with FORMATS[fmt][0](eng, max_words=len(w), max_events=len(whole) + 64) as dec:
        got = [dec.decode(w), dec.decode(t)]
    assert len(got[0]) == len(ref) and len(got[0]) + len(got[1]) == len(whole)
    _assert_same(got[0], whole[:len(ref)], (name, "first chunk"))
    _assert_same(got[1], whole[len(ref):], (name, "the 64 words behind it"))


@gpu
@pytest.mark.parametrize("fmt,name,pre", [(3, "evt3_wraps", "evt3_pre"), (2, "evt2_loops", "evt2_pre")])
def test_events_in_front_of_the_first_time_base_are_dropped_across_the_trips(eng, fmt, name, pre):
    """wait_for_time_base: the count of the events in front of the stream's first time-high word rides through the scan (n_pre),
    the trips of the prefix kernel included, and is taken off every record's position"""
    w = _frozen(np.concatenate((_words(pre), _words(name))))
    ref = _frozen(FORMATS[fmt][1].decode(w, True))
    typ = _typ(fmt, w)
    n_pre_events = len(FORMATS[fmt][1].decode(w[:N_PRE]))
    assert np.nonzero(typ == 0x8)[0][0] == N_PRE and len(w) > TRIP + N_PRE and n_pre_events >= N_PRE
    assert len(ref) == len(_reference(fmt, name)) and (ref["t"] >= ((1 << 24) - (1 << 20) if fmt == 3 else (1 << 34) - (1 << 30))).all()
    _assert_same(_one_chunk(eng, fmt, w, ref, wait=True), ref, (name, "wait"))


def test_the_streams_reach_the_second_trip_of_the_prefix_loop():
    """CPU: TRIP against the decoders' block geometry"""
    csrc = os.path.join(ROOT, "x_maps_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if re.fullmatch(r"xmaps_evt\w*\.hpp", f))
    m = re.search(r"constexpr\s+int\s+\w*THREADS\s*=\s*(\d+)\s*,\s*\w*IPT\s*=\s*(\d+)\s*,", src)
    assert m and int(m.group(1)) == THREADS and int(m.group(1)) * int(m.group(2)) == PER_BLOCK
    assert re.search(r"b0\s*<\s*n_blocks;\s*b0\s*\+=\s*\w*THREADS", src)  # the carry loop walks THREADS aggregates per trip
    assert TRIP == 524_288
