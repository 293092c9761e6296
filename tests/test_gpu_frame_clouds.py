"""-m gpu: the frame -> point cloud group entry (xm_frames_to_point_clouds) on the frames of tests/frame_cloud_cases.py (what
each is for: test_frame_cloud_cases_cpu.py, without a GPU).

 - against the stage call: row count, statistics and cloud bit for bit equal to engine.construct_point_cloud(Q, xr_f[mask],
   yr_f[mask], disp) on the oracle's rows -- the same device function, so the comparison is exact;
 - against the CPU oracle O.construct_point_cloud: equal finite / non-finite pattern, values to rtol = atol = 1e-5 (the tolerance
   tests/test_gpu_eval.py sets for this 4 x 4 float32 transform);
 - against the debug entry: disp and mask of xm_debug_event_outputs on the same frame give the same rows;
 - independence from the group, both memory kinds, untouched rows, both views, every XM_ERR_INVALID case.

Kernel geometry the cases cross (csrc/xmaps_framecloud.hpp): 64 events per inlier count, 1 024 events per block and chunk trip
(the 3 572-event frame takes four blocks, or -- with XM_FC_MAX_BLOCKS = 2 -- two trips of two), 32 frames per launch sequence."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_cloud_cases as K
import xmaps_oracle as O
from conftest import xm_option
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _tb():
    return K.rig_tables()


@functools.lru_cache(maxsize=None)
def _group():
    return K.group(_tb())


@functools.lru_cache(maxsize=None)
def _want(pol=False):
    """the oracle on every frame of the group: computed once, shared, never written to"""
    out = [K.oracle(_tb(), evs, pol) for evs in _group()[1]]
    for o in out:
        o["cloud"].setflags(write=False)
    return out


@pytest.fixture(scope="module")
def engines():
    from x_maps_amd.engine import XMapsEngine
    made = {}

    def get(camera=False):
        if camera not in made:
            made[camera] = XMapsEngine(_tb(), camera_perspective=camera)
        return made[camera]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def stage_clouds(engines):
    """engine.construct_point_cloud on the oracle's rows of every frame, with and without the polarity rule: computed once"""
    eng = engines()
    out = {}
    for pol in (False, True):
        out[pol] = [eng.construct_point_cloud(_tb()["Q"], o["xr_f"], o["yr_f"], o["disp"].astype(np.float32)) if len(o["disp"])
                    else np.zeros((0, 3), np.float32) for o in _want(pol)]
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stats(st):
    return {f: int(getattr(st, f)) for f in K.STAT_FIELDS}


def _check(got, pol, stage_clouds, order=None):
    names = _group()[0]
    want = _want(pol)
    order = range(len(want)) if order is None else order
    assert len(got) == len(order)
    for (cloud, st), i in zip(got, order):
        assert _stats(st) == want[i]["stats"], names[i]
        assert cloud.shape == stage_clouds[pol][i].shape and cloud.dtype == np.float32, names[i]
        assert np.array_equal(_bits(cloud), _bits(stage_clouds[pol][i])), names[i]


@pytest.mark.parametrize("pol", [False, True], ids=["all", "p1"])
def test_group_equals_the_stage_call_and_the_oracle(engines, stage_clouds, pol):
    eng = engines()
    names, frames = _group()
    got = eng.frames_to_point_clouds(frames, use_polarity=pol)
    _check(got, pol, stage_clouds)
    for (cloud, _), o, name in zip(got, _want(pol), names):  # the CPU oracle
        ref = o["cloud"]
        assert np.array_equal(np.isfinite(cloud), np.isfinite(ref)) and np.array_equal(np.isnan(cloud), np.isnan(ref)), name
        fin = np.isfinite(ref)
        assert np.array_equal(cloud[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), name  # (the infinities' signs)
        assert np.allclose(cloud[fin], ref[fin], rtol=1e-5, atol=1e-5), name
    # the same group again in another frame order: the results follow the frames (and nothing of the first call is left over)
    order = list(range(len(frames)))[::-1]
    order = order[3:] + order[:3]
    _check(eng.frames_to_point_clouds([frames[i] for i in order], use_polarity=pol), pol, stage_clouds, order)


def test_the_debug_entry_gives_the_same_rows(engines):
    eng = engines()
    tb = _tb()
    names, frames = _group()
    got = eng.frames_to_point_clouds(frames)
    for name, evs, (cloud, st) in zip(names, frames, got):
        on = (evs["x"] < tb["cam_w"]) & (evs["y"] < tb["cam_h"])
        ev = evs[on]
        if len(evs) == 0:
            assert len(cloud) == 0
            continue
        # the frame's extrema through the debug entry as well: two further events off the sensor hold them (mask 0 there)
        x = np.concatenate([ev["x"], [65535, 65535]]).astype(np.uint16)
        y = np.concatenate([ev["y"], [65535, 65535]]).astype(np.uint16)
        t = np.concatenate([ev["t"], [evs["t"].min(), evs["t"].max()]]).astype(np.int64)
        d = eng.debug_event_outputs(x, y, t)
        mask, disp = d["mask"][:-2], d["disp"][:-2]
        assert not d["mask"][-2:].any()
        xf, yf = O.rectify_cam_coords_f32(tb["cam_mapx_f32"], tb["cam_mapy_f32"], ev["x"][mask], ev["y"][mask])
        ref = eng.construct_point_cloud(tb["Q"], xf, yf, disp[mask].astype(np.float32)) if mask.any() else np.zeros((0, 3), np.float32)
        assert st.n_inliers == int(mask.sum()) and np.array_equal(_bits(cloud), _bits(ref)), name


def test_further_trips_of_the_chunk_loops_and_two_launch_sequences(engines, stage_clouds):
    eng = engines()
    names, frames = _group()
    xm_option("XM_FC_MAX_BLOCKS", 2)  # the 3 572-event frame: two trips of two blocks
    _check(eng.frames_to_point_clouds(frames), False, stage_clouds)
    xm_option("XM_FC_MAX_BLOCKS", None)
    order = K.group33(_tb())  # 33 frames with empties in between: launch sequences of 32 and 1
    _check(eng.frames_to_point_clouds([frames[i] for i in order]), False, stage_clouds, order)


def test_a_frame_does_not_depend_on_its_group(engines, stage_clouds):
    eng = engines()
    names, frames = _group()
    for k in ("long", "outside", "disp0", "n65"):
        i = names.index(k)
        _check(eng.frames_to_point_clouds([frames[i]]), False, stage_clouds, [i])  # alone
        j = names.index("after_empty")
        _check(eng.frames_to_point_clouds([frames[j], frames[i], frames[0]]), False, stage_clouds, [j, i, 0])  # at another place
        _check(eng.frames_to_point_clouds([frames[i], frames[i]]), False, stage_clouds, [i, i])  # twice, after other calls


def _raw_call(eng, evs_ptr, offs, n, mem, cloud_ptr, st_ptr, pol=0):
    return eng._lib.xm_frames_to_point_clouds(eng._h, C.c_void_p(evs_ptr), offs.ctypes.data_as(C.POINTER(C.c_uint64)), n, pol, mem,
                                              C.c_void_p(cloud_ptr), C.c_void_p(st_ptr))


def test_memory_kinds_untouched_rows_and_a_first_offset(engines, stage_clouds):
    """XM_MEM_HOST == XM_MEM_DEVICE; rows past n_inliers keep a sentinel in both; offsets[0] != 0"""
    eng = engines()
    eng.set_frame_cloud_tables()
    names, frames = _group()
    lead = 37
    evs, offs = K.concat(frames, lead=lead)
    n, rows = len(frames), int(offs[-1] - offs[0])
    sentinel = np.float32(-77.25)
    host = np.full((rows, 3), sentinel, np.float32)
    st_h = (N.xm_frame_cloud_stats * n)()
    N.check(_raw_call(eng, evs.ctypes.data, offs, n, N.XM_MEM_HOST, host.ctypes.data, C.addressof(st_h)))
    d_ev, d_cloud = eng.to_device(evs), eng.to_device(np.full((rows, 3), sentinel, np.float32))
    d_st = eng.dev_alloc(n * C.sizeof(N.xm_frame_cloud_stats))
    try:
        N.check(_raw_call(eng, d_ev, offs, n, N.XM_MEM_DEVICE, d_cloud, d_st))
        eng.sync()
        dev = np.empty((rows, 3), np.float32)
        st = np.empty(n * C.sizeof(N.xm_frame_cloud_stats), np.uint8)
        eng.dev_download(dev, d_cloud)
        eng.dev_download(st, d_st)
    finally:
        for p in (d_ev, d_cloud, d_st):
            eng.dev_free(p)
    st_d = (N.xm_frame_cloud_stats * n).from_buffer_copy(st.tobytes())
    assert np.array_equal(_bits(host), _bits(dev)) and bytes(st_h) == bytes(st_d)
    for i in range(n):
        r0, k = int(offs[i]) - lead, int(st_h[i].n_inliers)
        r1 = int(offs[i + 1]) - lead
        assert _stats(st_h[i]) == _want()[i]["stats"], names[i]
        assert np.array_equal(_bits(host[r0:r0 + k]), _bits(stage_clouds[False][i])), names[i]
        assert (host[r0 + k:r1] == sentinel).all(), names[i]
    assert any(0 < int(s.n_inliers) < int(offs[i + 1] - offs[i]) for i, s in enumerate(st_h))


def test_both_views_give_the_same_cloud(engines, stage_clouds):
    names, frames = _group()
    _check(engines(camera=True).frames_to_point_clouds(frames), False, stage_clouds)
    _check(engines(camera=True).frames_to_point_clouds(frames, use_polarity=True), True, stage_clouds)


def test_invalid_calls(stage_clouds):
    from x_maps_amd.engine import XMapsEngine
    names, frames = _group()
    evs, offs = K.concat(frames)
    n = len(frames)
    out = np.full((len(evs), 3), 7, np.float32)
    st = (N.xm_frame_cloud_stats * n)()
    with XMapsEngine(_tb()) as eng:
        def call(offsets=offs, n_frames=n, mem=N.XM_MEM_HOST, cloud=out.ctypes.data):
            return _raw_call(eng, evs.ctypes.data, offsets, n_frames, mem, cloud, C.addressof(st))
        assert call() == N.XM_ERR_INVALID  # cloud_out without tables
        assert (out == 7).all()
        assert call(cloud=None) == N.XM_OK  # ... statistics alone need none
        assert [_stats(s) for s in st] == [o["stats"] for o in _want()]
        eng.set_frame_cloud_tables()
        bad = offs.copy()
        bad[3], bad[4] = offs[4], offs[3]  # decreasing
        assert offs[4] > offs[3]
        for rc in (call(bad), call(n_frames=0), call(n_frames=-1), call(mem=5)):
            assert rc == N.XM_ERR_INVALID
        assert (out == 7).all()  # nothing was written
        assert call() == N.XM_OK
        for i in range(n):
            k = int(st[i].n_inliers)
            assert np.array_equal(_bits(out[int(offs[i]):int(offs[i]) + k]), _bits(stage_clouds[False][i])), names[i]
