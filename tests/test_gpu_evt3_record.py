"""-m gpu: the frame -> EVT 3.0 group entry (xm_frames_to_evt3_words) on the frames of tests/evt3_record_cases.py (what each is
for: test_evt3_record_cases_cpu.py, without a GPU).

The oracle is the host encoder, x_maps_amd.evt3.encode_evt3 (vectors off: encode_evt3_singles); every comparison is bit for bit,
statistics included: host and device memory, vectors on and off, XM_ENC_MAX_BLOCKS at 1 and at its default, words behind n_words
untouched, independence from the group, handles of either view, every XM_ERR_INVALID case.

Kernel geometry the cases cross (csrc/xmaps_evt3enc.hpp): 64 events per word count, 1 024 events per block and chunk trip (the
3 572-event frame takes four blocks, or -- with XM_ENC_MAX_BLOCKS = 1 -- four trips of one), 32 frames per launch sequence, and
the scan block's threads take two counts each on the 65 765-event frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import evt3_record_cases as K
from conftest import xm_option
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
SENTINEL = 0xBEEF  # (type 0xB: no encoder writes it)


@functools.lru_cache(maxsize=None)
def _want(name, vec):
    """the host encoder on a case: computed once, shared, never written to"""
    words, st = K.oracle(K.big_frame() if name == "big" else K.cases()[name], vec)
    words.setflags(write=False)
    return words, st


@pytest.fixture(scope="module")
def engines():
    from x_maps_amd.engine import XMapsEngine
    made = {}

    def get(camera=False):
        if camera not in made:
            made[camera] = XMapsEngine(S.make_tables(S.C_TINY), camera_perspective=camera)
        return made[camera]
    yield get
    for e in made.values():
        e.close()


def _stats(st):
    return {f: int(getattr(st, f)) for f in K.STAT_FIELDS}


def _check(got, names, vec):
    words, stats = got
    assert len(words) == len(stats) == len(names)
    for w, st, name in zip(words, stats, names):
        want, want_st = _want(name, vec)
        assert _stats(st) == want_st, (name, vec)
        assert w.dtype == np.uint16 and np.array_equal(w, want), (name, vec)


@pytest.mark.parametrize("vec", [True, False], ids=["vectors", "singles"])
@pytest.mark.parametrize("max_blocks", [None, 1], ids=["grid", "one_block"])
def test_every_case_equals_the_host_encoder(engines, vec, max_blocks):
    eng = engines()
    names = list(K.cases())
    frames = [K.cases()[k] for k in names]
    xm_option("XM_ENC_MAX_BLOCKS", max_blocks)
    _check(eng.frames_to_evt3_words(frames, use_vectors=vec), names, vec)
    # the same group again in another frame order: the results follow the frames (and nothing of the first call is left over)
    order = list(range(len(names)))[::-1]
    order = order[5:] + order[:5]
    _check(eng.frames_to_evt3_words([frames[i] for i in order], use_vectors=vec), [names[i] for i in order], vec)
    for n in (33, 65):  # launch sequences of 32 + 1 and 32 + 32 + 1 frames
        pick, group = K.group(n)
        _check(eng.frames_to_evt3_words(group, use_vectors=vec), pick, vec)


@pytest.mark.parametrize("max_blocks", [None, 1], ids=["grid", "one_block"])
def test_the_scan_past_its_first_trip(engines, max_blocks):
    """a frame of more than 1 024 counts: two per thread of the scan block (one block of the per-event passes: 65 trips)"""
    xm_option("XM_ENC_MAX_BLOCKS", max_blocks)
    _check(engines().frames_to_evt3_words([K.cases()["n65"], K.big_frame(), K.cases()["run12"]]), ["n65", "big", "run12"], True)


def test_a_frame_does_not_depend_on_its_group(engines):
    eng = engines()
    c = K.cases()
    for vec in (True, False):
        for k in ("long_chain", "chain_ends_segment", "out_of_range", "n65"):
            _check(eng.frames_to_evt3_words([c[k]], use_vectors=vec), [k], vec)                                                  # alone
            _check(eng.frames_to_evt3_words([c[k], c["empty"], c["run12"]], use_vectors=vec), [k, "empty", "run12"], vec)         # first
            _check(eng.frames_to_evt3_words([c["random_3572"], c["empty"], c[k]], use_vectors=vec), ["random_3572", "empty", k], vec)  # last
            _check(eng.frames_to_evt3_words([c["wide_random"], c[k], c[k], c["n1"]], use_vectors=vec), ["wide_random", k, k, "n1"], vec)  # middle, twice
    # the array form with offsets, and a handle of the camera view
    names = list(c)
    evs, offs = K.concat([c[k] for k in names], lead=37)
    _check(eng.frames_to_evt3_words(evs, offs), names, True)
    _check(engines(camera=True).frames_to_evt3_words(evs, offs, use_vectors=False), names, False)


def _raw_call(eng, evs_ptr, offs, n, mem, words_ptr, st_ptr, vec=1):
    return eng._lib.xm_frames_to_evt3_words(eng._h, C.c_void_p(evs_ptr), offs.ctypes.data_as(C.POINTER(C.c_uint64)), n, vec, mem,
                                            C.c_void_p(words_ptr), C.c_void_p(st_ptr))


@pytest.mark.parametrize("vec", [True, False], ids=["vectors", "singles"])
def test_memory_kinds_untouched_words_and_a_first_offset(engines, vec):
    """XM_MEM_HOST == XM_MEM_DEVICE; words past n_words keep a sentinel in both; offsets[0] != 0"""
    eng = engines()
    names = list(K.cases())
    lead = 37
    evs, offs = K.concat([K.cases()[k] for k in names], lead=lead)
    n, room = len(names), 4 * int(offs[-1] - offs[0])
    host = np.full(room, SENTINEL, np.uint16)
    st_h = (N.xm_evt3_record_stats * n)()
    N.check(_raw_call(eng, evs.ctypes.data, offs, n, N.XM_MEM_HOST, host.ctypes.data, C.addressof(st_h), int(vec)))
    d_ev, d_words = eng.to_device(evs), eng.to_device(np.full(room, SENTINEL, np.uint16))
    d_st = eng.dev_alloc(n * C.sizeof(N.xm_evt3_record_stats))
    try:
        N.check(_raw_call(eng, d_ev, offs, n, N.XM_MEM_DEVICE, d_words, d_st, int(vec)))
        eng.sync()
        dev = np.empty(room, np.uint16)
        st = np.empty(n * C.sizeof(N.xm_evt3_record_stats), np.uint8)
        eng.dev_download(dev, d_words)
        eng.dev_download(st, d_st)
        # the Python entry on device records: the same words
        _check(eng.frames_to_evt3_words(d_ev, offs, use_vectors=vec, device=True), names, vec)
    finally:
        for p in (d_ev, d_words, d_st):
            eng.dev_free(p)
    st_d = (N.xm_evt3_record_stats * n).from_buffer_copy(st.tobytes())
    assert np.array_equal(host, dev) and bytes(st_h) == bytes(st_d)
    for i, name in enumerate(names):
        w0, w1, k = 4 * (int(offs[i]) - lead), 4 * (int(offs[i + 1]) - lead), int(st_h[i].n_words)
        want, want_st = _want(name, vec)
        assert _stats(st_h[i]) == want_st, name
        assert np.array_equal(host[w0:w0 + k], want), name
        assert (host[w0 + k:w1] == SENTINEL).all(), name
    assert any(0 < int(s.n_words) < 4 * int(offs[i + 1] - offs[i]) for i, s in enumerate(st_h))


def test_invalid_calls(engines):
    eng = engines()
    names = list(K.cases())
    evs, offs = K.concat([K.cases()[k] for k in names])
    n = len(names)
    out = np.full(4 * len(evs), SENTINEL, np.uint16)
    st = (N.xm_evt3_record_stats * n)()

    def call(offsets=offs, n_frames=n, mem=N.XM_MEM_HOST, words=out.ctypes.data, records=evs.ctypes.data, h=eng):
        return _raw_call(h, records, offsets, n_frames, mem, words, C.addressof(st))
    bad = offs.copy()
    i = names.index("long_chain")
    bad[i], bad[i + 1] = offs[i + 1], offs[i]  # decreasing
    assert offs[i + 1] > offs[i]
    for rc in (call(bad), call(n_frames=0), call(n_frames=-1), call(mem=5), call(words=None), call(records=None)):
        assert rc == N.XM_ERR_INVALID
    assert eng._lib.xm_frames_to_evt3_words(None, None, offs.ctypes.data_as(C.POINTER(C.c_uint64)), n, 1, 0, None, None) == N.XM_ERR_INVALID
    assert eng._lib.xm_frames_to_evt3_words(eng._h, C.c_void_p(evs.ctypes.data), None, n, 1, 0, C.c_void_p(out.ctypes.data), None) == N.XM_ERR_INVALID
    d = eng.dev_alloc(64)
    try:  # device records must be 16-byte aligned
        two = np.array([0, 1], np.uint64)
        assert _raw_call(eng, d + 8, two, 1, N.XM_MEM_DEVICE, d, 0) == N.XM_ERR_INVALID
    finally:
        eng.dev_free(d)
    assert (out == SENTINEL).all()  # nothing was written
    assert call() == N.XM_OK
    for i, name in enumerate(names):
        assert np.array_equal(out[4 * int(offs[i]):4 * int(offs[i]) + int(st[i].n_words)], _want(name, True)[0]), name
    # a group of empty frames needs no arrays at all
    zero = np.zeros(4, np.uint64)
    assert _raw_call(eng, 0, zero, 3, N.XM_MEM_HOST, 0, C.addressof(st)) == N.XM_OK
    assert all(_stats(st[k]) == _want("empty", True)[1] for k in range(3))
