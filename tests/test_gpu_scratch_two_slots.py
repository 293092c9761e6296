"""-m gpu: the three entries that keep ONE scratch per handle (xm_process_time_surfaces, xm_frames_to_time_surfaces,
xm_frames_to_point_clouds; csrc/host/xm_scratch_order.hpp orders their calls) on a handle with TWO slots, where consecutive calls
run on different streams.  Three XM_MEM_DEVICE calls back to back, no synchronisation between them:

  call 1  a group of 2 frames   slot 0's stream: the first call, the scratch is made
  call 2  a group of 5 frames   slot 1's stream: the scratch grows while call 1 may be in flight (the host waits for it first)
  call 3  the group of 2 again  slot 0's stream: call 2 may be in flight on the other stream (the stream waits for its event)

After one sync every output and statistic is bit-equal to the same three calls on a handle with one slot, where the stream alone
orders them; for the two frame entries also equal to the NumPy oracles (tests/frame_surface_cases.py bit for bit;
tests/frame_cloud_cases.py: statistics and row counts exactly, rows to the rtol = atol = 1e-5 tests/test_gpu_frame_clouds.py holds
that oracle to).  The 70 x 37 camera of tests/test_gpu_frame_surfaces.py; frames of 0, 1, 65 and 1 100 events (1 024 events per
block of the per-event passes: one chunk plus a tail)."""
import ctypes as C

import numpy as np
import pytest

import frame_cloud_cases as KC
import frame_surface_cases as KS
from x_maps_amd import _native as N
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu

W, H = KS.CAM_W, KS.CAM_H
PX = W * H


def _frame(rng, n, t0):
    ev = np.zeros(n, S.EVENT_CD_DTYPE)
    ev["x"], ev["y"], ev["p"] = rng.integers(0, W, n), rng.integers(0, H, n), 1
    ev["t"] = np.sort(rng.integers(0, 13_000, n)) + t0
    return ev


def _groups():
    """the three calls' frames: 2, 5 and the 2 again"""
    rng = np.random.default_rng(41)
    two = [_frame(rng, 65, 1_000_000), _frame(rng, 1100, 2_000_000)]
    five = [_frame(rng, 1100, 3_000_000), _frame(rng, 0, 0), _frame(rng, 1, 4_000_000), _frame(rng, 65, 5_000_000), _frame(rng, 1101, 6_000_000)]
    return [two, five, two]


@pytest.fixture(scope="module")
def rig():
    return KC.rig_tables(W, H)


@pytest.fixture(scope="module")
def engines(rig):
    from x_maps_amd.engine import XMapsEngine
    made = {n: XMapsEngine(rig, camera_perspective=True, n_slots=n) for n in (1, 2)}
    for e in made.values():
        e.set_cloud_tables(rig["cam_mapx_f32"], rig["cam_mapy_f32"], rig["Q"])
        e.set_frame_cloud_tables()
    yield made
    for e in made.values():
        e.close()


def _three_calls(eng, inputs, call, out_bytes):
    """inputs[k] / out_bytes[k]: call k's input arrays and the sizes of its outputs.  Everything is uploaded and allocated first; then
    call(k, device inputs, device outputs) three times with nothing in between, ONE sync, and the outputs come back as bytes."""
    d_in = [[eng.to_device(a) for a in arrs] for arrs in inputs]
    d_out = [[eng.to_device(np.full(nb, 0xA5, np.uint8)) for nb in sizes] for sizes in out_bytes]
    try:
        eng.sync()
        for k in range(3):
            call(k, d_in[k], d_out[k])
        eng.sync()
        got = []
        for ptrs, sizes in zip(d_out, out_bytes):
            got.append([np.empty(nb, np.uint8) for nb in sizes])
            for a, p in zip(got[-1], ptrs):
                eng.dev_download(a, p)
    finally:
        for p in [p for ptrs in d_in + d_out for p in ptrs]:
            eng.dev_free(p)
    return got


def _same(a, b):
    assert len(a) == len(b) == 3
    for k in range(3):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x, y), (k, i, int((x != y).sum()))


def _offs_ptr(offs):
    return offs.ctypes.data_as(C.POINTER(C.c_uint64))


def test_frames_to_time_surfaces(engines):
    groups = _groups()
    cat = [KS.concat(g) for g in groups]
    st_sz = C.sizeof(N.xm_frame_surface_stats)
    out_bytes = [[len(g) * PX * 4, len(g) * st_sz] for g in groups]

    def run(eng):
        def call(k, d_in, d_out):
            N.check(eng._lib.xm_frames_to_time_surfaces(eng._h, C.c_void_p(d_in[0]), _offs_ptr(cat[k][1]), len(groups[k]), 0, N.XM_SURFACE_LAST,
                                                        N.XM_T_FLOAT32, N.XM_MEM_DEVICE, C.c_void_p(d_out[0]), C.c_void_p(d_out[1])))
        return _three_calls(eng, [[c[0]] for c in cat], call, out_bytes)
    two, one = run(engines[2]), run(engines[1])
    _same(two, one)
    for k, g in enumerate(groups):
        surfs = two[k][0].view(np.float32).reshape(len(g), H, W)
        stats = (N.xm_frame_surface_stats * len(g)).from_buffer_copy(two[k][1].tobytes())
        for i, evs in enumerate(g):
            want, want_st = KS.oracle(evs, W, H, "last", np.float32)
            assert np.array_equal(surfs[i].view(np.uint32), want.view(np.uint32)), (k, i)
            assert {f: getattr(stats[i], f) for f in KS.STAT_FIELDS} == want_st, (k, i)


def test_frames_to_point_clouds(engines, rig):
    groups = _groups()
    cat = [KS.concat(g) for g in groups]
    st_sz = C.sizeof(N.xm_frame_cloud_stats)
    out_bytes = [[max(len(c[0]), 1) * 12, len(g) * st_sz] for g, c in zip(groups, cat)]

    def run(eng):
        def call(k, d_in, d_out):
            N.check(eng._lib.xm_frames_to_point_clouds(eng._h, C.c_void_p(d_in[0]), _offs_ptr(cat[k][1]), len(groups[k]), 0, N.XM_MEM_DEVICE,
                                                       C.c_void_p(d_out[0]), C.c_void_p(d_out[1])))
        return _three_calls(eng, [[c[0]] for c in cat], call, out_bytes)
    two, one = run(engines[2]), run(engines[1])
    _same(two, one)
    n_rows = 0
    for k, g in enumerate(groups):
        cloud = two[k][0].view(np.float32).reshape(-1, 3)
        stats = (N.xm_frame_cloud_stats * len(g)).from_buffer_copy(two[k][1].tobytes())
        for i, evs in enumerate(g):
            o = KC.oracle(rig, evs)
            assert {f: int(getattr(stats[i], f)) for f in KC.STAT_FIELDS} == o["stats"], (k, i)
            r0, ref = int(cat[k][1][i]), o["cloud"]
            got = cloud[r0:r0 + len(ref)]
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(ref)), (k, i)
            assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (k, i)
            assert np.allclose(got[fin], ref[fin], rtol=1e-5, atol=1e-5), (k, i)
            # rows past the frame's inliers are not touched
            assert (two[k][0][(r0 + len(ref)) * 12:int(cat[k][1][i + 1]) * 12] == 0xA5).all(), (k, i)
            n_rows += len(ref)
    assert n_rows > 300  # (the comparison is about something)


def test_process_time_surfaces(engines):
    groups = _groups()
    surfs = [np.stack([KS.oracle(evs, W, H, "last", np.float32)[0] for evs in g]) for g in groups]
    st_sz = C.sizeof(N.xm_surface_stats)
    out_bytes = [[len(g) * PX * 4, len(g) * PX * 12, len(g) * st_sz] for g in groups]

    def run(eng):
        def call(k, d_in, d_out):
            N.check(eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(d_in[0]), N.XM_T_FLOAT32, len(groups[k]), N.XM_MEM_DEVICE,
                                                      C.c_void_p(d_out[0]), C.c_void_p(d_out[1]), C.c_void_p(d_out[2])))
        return _three_calls(eng, [[s] for s in surfs], call, out_bytes)
    two, one = run(engines[2]), run(engines[1])
    _same(two, one)
    # ... and equal to the host route, one group per synchronous call
    inliers = 0
    for k, g in enumerate(groups):
        host = engines[1].process_time_surfaces(surfs[k], want_cloud=True)
        depth = two[k][0].view(np.float32).reshape(len(g), H, W)
        cloud = two[k][1].view(np.float32).reshape(len(g), PX, 3)
        stats = (N.xm_surface_stats * len(g)).from_buffer_copy(two[k][2].tobytes())
        for i in range(len(g)):
            rows = int(stats[i].n_inliers)
            assert rows == host[i][2].n_inliers and int(stats[i].n_events) == host[i][2].n_events, (k, i)
            assert np.array_equal(depth[i].view(np.uint32), host[i][0].view(np.uint32)), (k, i)
            assert np.array_equal(cloud[i, :rows].view(np.uint32), host[i][1].view(np.uint32)), (k, i)
            inliers += rows
    assert inliers > 300
