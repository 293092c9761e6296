"""-m gpu: the frame -> time surface group entry (xm_frames_to_time_surfaces) against its NumPy oracle
(tests/frame_surface_cases.py), bit for bit: surfaces and all five statistics, both dtypes, both `select` values, with and
without the polarity rule, on the 70 x 37 sensor (2 590 cells: no multiple of 64 or 1024, three blocks of cells) and on C_TINY.

The group's frames and what each is for: frame_surface_cases.frames (checked without a GPU by test_frame_surface_cases_cpu.py).
Kernel geometry the cases cross (csrc/xmaps_framesurface.hpp): 1 024 events per block and chunk trip (the 5 000-event frame takes
five blocks, or -- with XM_FS_MAX_BLOCKS = 2 -- three trips of two), 1 024 cells per block of the cell pass, 16-byte stores where
a frame's place in the output allows them (70 x 37 float32 frames alternate between aligned and not), 32 frames per launch
sequence (the group of 12 repeated six times takes three)."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_surface_cases as K
from conftest import xm_option
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu

SIZES = {"70x37": (K.CAM_W, K.CAM_H), "tiny": (S.C_TINY.cam_w, S.C_TINY.cam_h)}
SEL = {"last": N.XM_SURFACE_LAST, "first": N.XM_SURFACE_FIRST}
DT = {np.dtype(np.float32): N.XM_T_FLOAT32, np.dtype(np.float64): N.XM_T_FLOAT64}


@pytest.fixture(scope="module")
def engines():
    from x_maps_amd.engine import XMapsEngine
    made = {}

    def get(size, camera=False):
        if (size, camera) not in made:
            tb = K.rig_tables(*SIZES[size]) if size != "tiny" else S.make_tables(S.C_TINY)
            made[size, camera] = XMapsEngine(tb, camera_perspective=camera)
        return made[size, camera]
    yield get
    for e in made.values():
        e.close()


@functools.lru_cache(maxsize=None)
def _group(size):
    return K.group(*SIZES[size])


@functools.lru_cache(maxsize=None)
def _want(size, select, dtype, pol):
    """the oracle on every frame of the group: computed once, shared, never written to"""
    out = [K.oracle(evs, *SIZES[size], select, dtype, pol) for evs in _group(size)[1]]
    for s, _ in out:
        s.setflags(write=False)
    return out


def _same_bits(a, b):
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def _stats(st):
    return {f: getattr(st, f) for f in K.STAT_FIELDS}


def _check(got, want, names, order=None):
    surfs, stats = got
    order = range(len(want)) if order is None else order
    assert len(surfs) == len(stats) == len(order)
    for k, i in enumerate(order):
        assert _same_bits(surfs[k], want[i][0]), (names[i], int((surfs[k] != want[i][0]).sum()))
        assert _stats(stats[k]) == want[i][1], names[i]


@pytest.mark.parametrize("pol", [False, True], ids=["all", "p1"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("select", K.SELECTS)
@pytest.mark.parametrize("size", list(SIZES))
def test_group_equals_the_oracle(engines, size, select, dtype, pol):
    eng = engines(size)
    names, frames = _group(size)
    want = _want(size, select, np.dtype(dtype), pol)
    _check(eng.frames_to_time_surfaces(frames, select, dtype, use_polarity=pol), want, names)
    # the same group again in another frame order: the results follow the frames (and nothing of the first call is left over)
    order = list(range(len(frames)))[::-1]
    order = order[3:] + order[:3]
    _check(eng.frames_to_time_surfaces([frames[i] for i in order], select, dtype, use_polarity=pol), want, names, order)


@pytest.mark.parametrize("select", K.SELECTS)
def test_further_trips_of_the_event_pass_and_more_frames_than_one_launch_sequence(engines, select):
    eng = engines("70x37")
    names, frames = _group("70x37")
    want = _want("70x37", select, np.dtype(np.float32), False)
    xm_option("XM_FS_MAX_BLOCKS", 2)  # the 5 000-event frame: three trips of two blocks
    _check(eng.frames_to_time_surfaces(frames, select, np.float32), want, names)
    xm_option("XM_FS_MAX_BLOCKS", None)
    order = list(range(len(frames))) * 6  # 72 frames: launch sequences of 32, 32 and 8 that reuse the winner maps
    _check(eng.frames_to_time_surfaces([frames[i] for i in order], select, np.float32), want, names, order)


def test_an_invalid_call_is_followed_by_a_correct_one(engines):
    eng = engines("70x37")
    names, frames = _group("70x37")
    evs, offs = K.concat(frames)
    n = len(frames)
    out = np.full((n, K.CAM_H, K.CAM_W), 7, np.float32)
    st = (N.xm_frame_surface_stats * n)()

    def call(offsets, n_frames=n, select=N.XM_SURFACE_LAST, dtype=N.XM_T_FLOAT32):
        return eng._lib.xm_frames_to_time_surfaces(eng._h, C.c_void_p(evs.ctypes.data), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   n_frames, 0, select, dtype, N.XM_MEM_HOST, C.c_void_p(out.ctypes.data), C.cast(st, C.c_void_p))
    bad = offs.copy()
    bad[3], bad[4] = offs[4], offs[3]  # decreasing
    assert offs[4] > offs[3]
    for rc in (call(bad), call(offs, select=0), call(offs, select=3), call(offs, dtype=N.XM_T_INT64), call(offs, n_frames=0),
               call(offs, n_frames=-1)):
        assert rc == N.XM_ERR_INVALID
    assert (out == 7).all()  # nothing was written
    assert call(offs) == N.XM_OK
    _check((out, list(st)), _want("70x37", "last", np.dtype(np.float32), False), names)


def test_device_surfaces_feed_the_time_surface_entry(engines):
    """Surfaces written to xm_dev_alloc memory go straight into xm_process_time_surfaces(XM_MEM_DEVICE) on a camera-view handle:
    depth maps equal to the host route on the downloaded surfaces, bit for bit."""
    eng = engines("70x37", camera=True)
    names, frames = _group("70x37")
    pick = [names.index(k) for k in ("long", "duplicates", "empty", "after_empty")]
    frames = [frames[i] for i in pick]
    want = [_want("70x37", "last", np.dtype(np.float32), False)[i] for i in pick]
    n, px = len(frames), K.CAM_W * K.CAM_H
    evs, offs = K.concat(frames)
    d_ev, d_surf, d_depth = eng.to_device(evs), eng.dev_alloc(n * px * 4), eng.dev_alloc(n * px * 4)
    d_st = eng.dev_alloc(n * C.sizeof(N.xm_frame_surface_stats))
    try:
        N.check(eng._lib.xm_frames_to_time_surfaces(eng._h, C.c_void_p(d_ev), offs.ctypes.data_as(C.POINTER(C.c_uint64)), n, 0,
                                                    N.XM_SURFACE_LAST, N.XM_T_FLOAT32, N.XM_MEM_DEVICE, C.c_void_p(d_surf), C.c_void_p(d_st)))
        N.check(eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(d_surf), N.XM_T_FLOAT32, n, N.XM_MEM_DEVICE, C.c_void_p(d_depth),
                                                  None, None))
        eng.sync()
        surfs, depth = np.empty((n, K.CAM_H, K.CAM_W), np.float32), np.empty((n, K.CAM_H, K.CAM_W), np.float32)
        st = np.empty(n * C.sizeof(N.xm_frame_surface_stats), np.uint8)
        eng.dev_download(surfs, d_surf)
        eng.dev_download(depth, d_depth)
        eng.dev_download(st, d_st)
    finally:
        for p in (d_ev, d_surf, d_depth, d_st):
            eng.dev_free(p)
    stats = (N.xm_frame_surface_stats * n).from_buffer_copy(st.tobytes())
    _check((surfs, list(stats)), want, [names[i] for i in pick])
    host = eng.process_time_surfaces(surfs)
    assert any(h[2].n_inliers > 100 for h in host)  # (the comparison below is about something)
    for i in range(n):
        assert _same_bits(depth[i], host[i][0]), i
