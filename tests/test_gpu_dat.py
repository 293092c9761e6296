"""-m gpu: the device DAT decoder (csrc/xmaps_dat.hpp: the loop count as three scan launches, the emit elementwise) against the
independent record-by-record checker (tests/dat_ref.py) and the hand-derived records of tests/test_dat.py -- x, y, p, t and the
count exactly, whole and in chunks (state carried on the device).  The ingest, the processor's process_dat_records and a DAT file
through tools/run_esl_on_arrival.py are compared with the other formats in tests/test_gpu_evt21.py."""
import numpy as np
import pytest

import dat_ref as DR
from test_dat import HAND, _same, _tuples, random_records, records, stream
from x_maps_amd import XMapsEngine, dat
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
PER_BLOCK = 2048  # csrc/xmaps_evt.hpp: EVT_PER_BLOCK


@pytest.fixture(scope="module")
def eng():
    with XMapsEngine(S.make_tables(S.C_TINY)) as e:
        yield e


def test_hand_derived_records(eng):
    for pairs, want in HAND:
        with dat.DeviceDatDecoder(eng, max_words=64) as dec:
            assert _tuples(dec.decode(records(pairs))) == want
        with dat.DeviceDatDecoder(eng, max_words=64, wait_for_time_base=True) as dec:  # (nothing to wait for in this format)
            assert _tuples(dec.decode(records(pairs).view("<u8"))) == want


def test_prefix_carry_second_trip_and_chunks(eng):
    """more than 256 blocks of uniformly random records (a loop in every eighth): one chunk, then cut inside the second trip"""
    r = random_records(526_000, 32)
    ref = DR.decode(r)
    assert len(r) > 256 * PER_BLOCK and len(ref) == len(r) and int(ref["t"][-1]) >> 32 > 50_000
    with dat.DeviceDatDecoder(eng, max_words=len(r)) as dec:
        assert _same(dec.decode(r), ref)
        dec.reset()
        cut = 256 * PER_BLOCK + 1000
        assert _same(dec.decode(r[:cut]), ref[:cut])
        assert _same(dec.decode(r[cut:]), ref[cut:])
        dec.reset()
        sm = DR.DatStateMachine()
        for a in range(0, 3 * PER_BLOCK + 5, 1777):  # blocks' edges inside chunks, chunks' edges inside blocks
            piece = r[a:min(a + 1777, 3 * PER_BLOCK + 5)]
            assert _same(dec.decode(piece), sm.feed(piece)), a


def test_loops(eng):
    """encoded events across t = 2^32 and t = 2^33; the loop that falls between two chunks"""
    ev = np.zeros(9000, S.EVENT_CD_DTYPE)
    ev[:3000], ev[6000:] = stream(3000, (1 << 32) - 6000, seed=4), stream(3000, (1 << 33) - 6000, seed=5)
    ev[3000:6000] = stream(3000, (1 << 32) + (1 << 31) - 6000, seed=6)  # (no single step of the clock is more than 2^31)
    assert ev["t"][0] < (1 << 32) < ev["t"][2999] and ev["t"][6000] < (1 << 33) < ev["t"][-1] and (np.diff(ev["t"]) < (1 << 31)).all()
    r = dat.encode_dat(ev)
    assert _same(DR.decode(r), ev)
    wrap = int(np.nonzero(np.diff(r["ts"].astype(np.int64)) < 0)[0][0]) + 1  # the first record behind the clock's end
    with dat.DeviceDatDecoder(eng, max_words=len(r)) as dec:
        assert _same(dec.decode(r), ev)
        dec.reset()
        assert _same(dec.decode(r[:wrap]), ev[:wrap]) and _same(dec.decode(r[wrap:]), ev[wrap:])


def test_limits(eng):
    r = dat.encode_dat(stream(500, 1000, seed=1))
    with dat.DeviceDatDecoder(eng, max_words=len(r), max_events=300) as dec:
        with pytest.raises(N.XMapsTooMany, match="decodes to 500 events"):
            dec.decode_device(r)
        assert _same(dec.decode(r[:250]), DR.decode(r[:250]))  # (the state did not advance)
    with dat.DeviceDatDecoder(eng, max_words=100) as dec:
        with pytest.raises(N.XMapsTooMany, match="max_words"):
            dec.decode_device(r)
        assert dec.decode_device(r[:0]) [1] == 0
