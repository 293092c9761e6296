"""-m gpu: the pause detection (xm_find_pauses: k_pause_flags, k_filter_scan_blocks, k_filter_scan_sums, k_pause_emit of
csrc/xmaps_filters.hpp) against np.nonzero(np.diff(t) >= thresh)[0], exactly, past the bound of the scan of the block totals
(more than SCAN_BLOCK * SCAN_BLOCK stamps: the second trip of k_filter_scan_sums), with dense flags, pauses on the edges of the
scan blocks and of the chunk, and in all four input forms: host SoA, host EventCD, device SoA, device EventCD.  (The unmarked
test at the end checks the lengths against SCAN_BLOCK on the CPU.)"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from x_maps_amd import synthetic as S

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCAN_BLOCK = 1024  # csrc/xmaps_filters.hpp (checked at the end)
N_LONG = 1024 * 1025 + 3  # 1 049 603 stamps: 1026 scan blocks, the last with 3 stamps
EDGES = (1022, 1023, 1024, 1_048_574, 1_048_575, 1_048_576, N_LONG - 2)  # both sides of a block edge, of the chunk edge; the last diff


@pytest.fixture(scope="module")
def engine():
    from x_maps_amd.engine import XMapsEngine
    with XMapsEngine(S.make_tables(S.C_TINY)) as eng:
        yield eng


def _from_gaps(gaps):
    return np.concatenate(([5_000_000], 5_000_000 + np.cumsum(gaps))).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _stream(name):
    """-> (t int64, thresh_us)"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "long_random":
        t = _from_gaps(rng.integers(0, 60, N_LONG - 1))
        t += 1 << 40  # stamps that need all 64 bits of the difference's operands
        thresh = 40
    elif name == "long_all_equal":  # with thresh 0 every index but the last is a pause: the scan at full occupancy
        t, thresh = np.full(N_LONG, 77_777, np.int64), 0
    elif name == "long_edges":
        gaps = np.ones(N_LONG - 1, np.int64)
        gaps[list(EDGES)] = 1000
        t, thresh = _from_gaps(gaps), 40
    elif name == "long_no_pause":
        t, thresh = _from_gaps(rng.integers(0, 40, N_LONG - 1)), 40
    elif name in ("n1024", "n1025"):
        n = int(name[1:])
        gaps = rng.integers(0, 60, n - 1)
        gaps[[0, n - 2]] = 50  # the first and the last difference
        t, thresh = _from_gaps(gaps), 40
    elif name == "n2_pause":
        t, thresh = np.array([10, 50], np.int64), 40
    elif name == "n2_none":
        t, thresh = np.array([10, 49], np.int64), 40
    elif name == "unsorted":  # negative differences must never count
        t, thresh = rng.integers(0, 2000, 3 * SCAN_BLOCK + 1).astype(np.int64) + (1 << 33), 40
    elif name == "negative_thresh":  # ... unless the threshold asks for them
        t, thresh = rng.integers(0, 200, 3 * SCAN_BLOCK + 1).astype(np.int64), -25
    t.flags.writeable = False
    return t, thresh


STREAMS = ("long_random", "long_all_equal", "long_edges", "long_no_pause", "n1024", "n1025", "n2_pause", "n2_none", "unsorted",
           "negative_thresh")


def _conditions(name, t, thresh, ref):
    """from NumPy alone: the stream has what it is for"""
    d = np.diff(t)
    if name == "long_random":
        assert len(t) == N_LONG and 0.25 < len(ref) / len(d) < 0.45 and ref[-1] > SCAN_BLOCK * SCAN_BLOCK and t.min() > 1 << 40
    elif name == "long_all_equal":
        assert len(t) == N_LONG and np.array_equal(ref, np.arange(N_LONG - 1))
    elif name == "long_edges":
        assert len(t) == N_LONG and ref.tolist() == list(EDGES)
    elif name == "long_no_pause":
        assert len(t) == N_LONG and len(ref) == 0 and d.max() == 39
    elif name in ("n1024", "n1025"):
        assert len(t) == int(name[1:]) and ref[0] == 0 and ref[-1] == len(t) - 2 and 100 < len(ref) < len(t) - 100
    elif name.startswith("n2"):
        assert len(t) == 2 and ref.tolist() == ([0] if name == "n2_pause" else []) and d[0] == (40 if name == "n2_pause" else 39)
    elif name == "unsorted":
        assert (d < -thresh).sum() > 1000 and (d >= thresh).sum() > 1000 and len(ref) == (d >= thresh).sum()
    elif name == "negative_thresh":
        assert thresh < 0 and ((d < 0) & (d >= thresh)).sum() > 100 and (d < thresh).sum() > 100 and (d == thresh).sum() > 3


@gpu
@pytest.mark.parametrize("name", STREAMS)
def test_all_four_input_forms_equal_numpy(engine, name):
    t, thresh = _stream(name)
    ref = np.nonzero(np.diff(t) >= thresh)[0]
    _conditions(name, t, thresh, ref)
    ev = np.zeros(len(t), S.EVENT_CD_DTYPE)
    ev["t"] = t
    ev["x"], ev["y"], ev["p"] = 0xFFFF, 0xFFFF, -1  # every bit of a record that is not its time stamp
    got = {"host_soa": engine.find_pauses(t=t, thresh_us=thresh), "host_eventcd": engine.find_pauses(evs=ev, thresh_us=thresh)}
    d_t, d_ev = engine.to_device(t), engine.to_device(ev)
    try:
        got["device_soa"] = engine.find_pauses(device_ptr=d_t, n=len(t), thresh_us=thresh)
        got["device_eventcd"] = engine.find_pauses(device_ptr=d_ev, n=len(t), thresh_us=thresh, aos=True)
    finally:
        engine.dev_free(d_t)
        engine.dev_free(d_ev)
    for form, idx in got.items():
        assert idx.dtype == np.int64 and len(idx) == len(ref), (form, len(idx), len(ref))
        assert np.array_equal(idx, ref), (form, int(np.flatnonzero(idx != ref)[0]))


@gpu
def test_idx_capacity_smaller_than_the_count(engine):
    """include/xmaps.h: *n_out may exceed idx_capacity; then only the first idx_capacity indices are written"""
    from x_maps_amd import _native as N
    t, thresh = _stream("n1025")
    ref = np.nonzero(np.diff(t) >= thresh)[0]
    k = len(ref)
    assert k > 10
    sentinel = 0xDEADBEEF
    buf = np.full(16, sentinel, np.uint32)
    n_out = C.c_size_t(0)
    N.check(engine._lib.xm_find_pauses(engine._h, C.c_void_p(t.ctypes.data), None, len(t), N.XM_MEM_HOST, thresh,
                                       C.c_void_p(buf.ctypes.data), 10, C.byref(n_out)))
    assert n_out.value == k and np.array_equal(buf[:10], ref[:10]) and (buf[10:] == sentinel).all()
    n_out = C.c_size_t(0)
    N.check(engine._lib.xm_find_pauses(engine._h, C.c_void_p(t.ctypes.data), None, len(t), N.XM_MEM_HOST, thresh, None, 0,
                                       C.byref(n_out)))
    assert n_out.value == k


def test_long_streams_reach_the_second_trip_of_the_sums_scan():
    """CPU: the lengths against the scan's constant"""
    src = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_filters.hpp")).read()
    sb = int(re.search(r"constexpr\s+int\s+SCAN_BLOCK\s*=\s*(\d+)\s*;", src).group(1))
    assert sb == SCAN_BLOCK and -(-N_LONG // sb) == sb + 2 > sb and N_LONG % sb == 3
    assert EDGES == (sb - 2, sb - 1, sb, sb * sb - 2, sb * sb - 1, sb * sb, N_LONG - 2)
    assert N_LONG * 16 <= 25_000_000  # the EventCD form of a long stream on the host
