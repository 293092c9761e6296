"""-m gpu: the time-surface entry (xm_process_time_surfaces / XMapsEngine.process_time_surfaces) -- a group of camera time
surfaces in, depth maps and per-event point clouds out, in one device call -- against golden G7 (the reference's own functions),
bit for bit against the staged GPU path, and at the edges of its compaction, its groups and its C-ABI."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import xmaps_oracle as O
from time_surface_cases import with_cloud_tables as _with_cloud_tables
from x_maps_amd.synthetic import C_TINY, RigConfig, make_tables

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g7_tables(g):
    return {"cam_mapx_i16": g["mapx"], "cam_mapy_i16": g["mapy"], "proj_x_map": g["xmap"],
            "rect_w": int(g["rect_w"]), "rect_h": int(g["rect_h"]), "p03": float(g["p03"]), "z_near": 0.1, "z_far": 1.0,
            "cam_mapx_f32": g["mapx_f32"], "cam_mapy_f32": g["mapy_f32"], "Q": g["Q"]}


def _odd_tables():
    """a 70 x 37 camera: the pixel count is no multiple of 64 or of the block size, the rows are no multiple of the tile's.
    The rectified rows are clipped into the X-map's defined band so that the last camera row has inliers."""
    cfg = RigConfig("C-odd", 70, 37, 70, 37, 0)
    tb = make_tables(cfg)
    tb["cam_mapy_i16"] = np.clip(tb["cam_mapy_i16"], 8, cfg.rect_h - 8).astype(np.int16)
    return _with_cloud_tables(tb, 11)


def _oracle_mask(tb, surf):
    x, y, t = O.time_surface_to_events(surf)
    r = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t, camera_perspective=True, want_bgr=False)
    return x, y, r["mask"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _random_surface(rng, shape, fill, dtype):
    s = (rng.random(shape) * 0.8 + 0.1).astype(dtype)
    s[rng.random(shape) >= fill] = 0
    return s


@pytest.fixture(scope="module")
def g7(golden_dir):
    return np.load(os.path.join(golden_dir, "g7_eval_caller.npz"))


@pytest.fixture(scope="module")
def g7_maps(g7):
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    maps = CamProjMaps(_g7_tables(g7), camera_perspective=True)
    yield maps
    maps.engine.close()


@pytest.fixture(scope="module")
def tiny_maps():
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    maps = CamProjMaps(_with_cloud_tables(make_tables(C_TINY), 3), camera_perspective=True)
    yield maps
    maps.engine.close()


@pytest.fixture(scope="module")
def odd_maps():
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    maps = CamProjMaps(_odd_tables(), camera_perspective=True)
    yield maps
    maps.engine.close()


def _staged(maps, surf):
    from x_maps_amd.eval_depth import compute_depth_from_time_surface
    from x_maps_amd.x_maps_disparity import XMapsDisparity
    return compute_depth_from_time_surface(maps, XMapsDisparity(maps), surf, want_point_cloud=True, fused=False)


def _assert_equals_staged(maps, surf):
    depth_s, cloud_s = _staged(maps, surf)
    depth, cloud, st = maps.engine.process_time_surfaces([surf], want_cloud=True)[0]
    assert _same_bits(depth, depth_s)
    assert _same_bits(cloud, cloud_s)
    assert st.n_inliers == len(cloud_s) and st.n_index_errors == 0
    return depth, cloud, st


# ---- 1. golden G7 -----------------------------------------------------------------------------------------------------------
def test_golden_g7(g7, g7_maps):
    depth, cloud, st = g7_maps.engine.process_time_surfaces([g7["raw_time_surface"]], want_cloud=True)[0]
    assert depth.dtype == np.float32 and depth.shape == g7["depth"].shape
    assert np.array_equal(depth == 0, g7["depth"] == 0)
    np.testing.assert_allclose(depth, g7["depth"], rtol=1e-4, atol=0)
    ref = g7["cloud"]
    assert cloud.shape == (1268, 3) and cloud.shape == ref.shape and cloud.dtype == np.float32
    fin = np.isfinite(ref)
    assert not fin.all()  # (rows of disparity 0)
    assert np.array_equal(np.isfinite(cloud), fin)
    np.testing.assert_allclose(cloud[fin], ref[fin], rtol=1e-5, atol=1e-6)
    assert st.n_events == 2007 and st.n_inliers == 1268
    assert st.n_nonzero == int((g7["raw_time_surface"] != 0).sum())
    nz = g7["raw_time_surface"][g7["raw_time_surface"] != 0]
    assert st.lo == nz.min() and st.hi == nz.max()
    assert st.t_min == g7["event_t"].min() and st.t_max == g7["event_t"].max() == 1.0


def test_eval_entries_take_the_device_route(g7, g7_maps):
    """compute_depth_from_time_surface(fused=True, want_point_cloud=True) and the group entry of eval_depth"""
    from x_maps_amd.eval_depth import compute_depth_from_time_surface, compute_depths_from_time_surfaces
    from x_maps_amd.x_maps_disparity import XMapsDisparity
    surf = g7["raw_time_surface"]
    depth_s, cloud_s = _staged(g7_maps, surf)
    before = g7_maps.engine.path_counts()
    depth, cloud = compute_depth_from_time_surface(g7_maps, XMapsDisparity(g7_maps), surf, want_point_cloud=True, fused=True)
    assert g7_maps.engine.path_counts() == before  # stayed on the device: none of the frame kernels ran
    assert _same_bits(depth, depth_s) and _same_bits(cloud, cloud_s)
    assert compute_depth_from_time_surface(g7_maps, XMapsDisparity(g7_maps), np.zeros_like(surf), want_point_cloud=True,
                                           fused=True) == (None, None)
    out = compute_depths_from_time_surfaces(g7_maps, [surf, np.zeros_like(surf), surf.astype(np.float32)], want_point_cloud=True)
    assert _same_bits(out[0][0], depth_s) and _same_bits(out[0][1], cloud_s)
    assert out[1] == (None, None)
    assert out[2][0].shape == depth_s.shape and len(out[2][1]) > 0
    out = compute_depths_from_time_surfaces(g7_maps, surf[None], want_point_cloud=False)
    assert _same_bits(out[0][0], depth_s) and out[0][1] is None


# ---- 2. bit-identical to the staged GPU path ----------------------------------------------------------------------------------
def test_equals_staged_path_on_g7(g7, g7_maps):
    _assert_equals_staged(g7_maps, g7["raw_time_surface"])
    _assert_equals_staged(g7_maps, g7["raw_time_surface"].astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fill", [1.0, 0.65, 0.02])
def test_equals_staged_path_on_random_surfaces(tiny_maps, fill, dtype):
    rng = np.random.default_rng(2024 + int(fill * 100) + (dtype is np.float64))
    surf = _random_surface(rng, (C_TINY.cam_h, C_TINY.cam_w), fill, dtype)
    _, _, mask = _oracle_mask(tiny_maps.tables, surf)
    assert mask.mean() >= 0.4  # the CPU oracle: these surfaces do have clouds
    _, cloud, st = _assert_equals_staged(tiny_maps, surf)
    assert len(cloud) == int(mask.sum()) and st.n_events == len(mask)


# ---- 3. compaction edges --------------------------------------------------------------------------------------------------------
def test_compaction_edges_on_an_odd_camera(odd_maps):
    tb = odd_maps.tables
    rng = np.random.default_rng(7)
    full = rng.random((37, 70)) * 0.8 + 0.1
    last_row = np.zeros((37, 70))
    last_row[36] = full[36]
    last_row[0, 0] = 0.05  # the surface's lo: normalises to 0 and is dropped
    corners = np.zeros((37, 70))
    corners[0, 0], corners[36, 69], corners[10, 33], corners[20, 5] = 0.7, 0.9, 0.05, 0.5
    x, y, mask = _oracle_mask(tb, last_row)
    assert set(y.tolist()) == {36} and mask.sum() >= 32
    x, y, mask = _oracle_mask(tb, corners)
    assert (x[0], y[0], mask[0]) == (0, 0, True) and (x[-1], y[-1], mask[-1]) == (69, 36, True)
    for surf in (last_row, corners, full, full.astype(np.float32)):
        _, _, mask = _oracle_mask(tb, surf)
        _, cloud, st = _assert_equals_staged(odd_maps, surf)
        assert len(cloud) == int(mask.sum()) > 0


# ---- 4. groups ------------------------------------------------------------------------------------------------------------------
def test_groups_equal_single_surfaces_and_scratch_grows(tiny_maps):
    eng = tiny_maps.engine
    rng = np.random.default_rng(99)
    shape = (C_TINY.cam_h, C_TINY.cam_w)
    single = np.zeros(shape)
    single[17, 40] = 0.3  # one non-zero pixel: hi == lo, nothing normalises above 0
    group = [_random_surface(rng, shape, 1.0, np.float64), _random_surface(rng, shape, 0.1, np.float64), np.zeros(shape), single,
             _random_surface(rng, shape, 0.65, np.float32)]
    alone = [eng.process_time_surfaces([s.astype(np.float64)], want_cloud=True)[0] for s in group]  # (groups of 1, first)
    out = eng.process_time_surfaces(group, want_cloud=True)  # a larger group than any call before: the scratch grows
    assert len(out) == 5
    for (d, c, st), (d1, c1, st1) in zip(out, alone):
        assert _same_bits(d, d1) and _same_bits(c, c1) and st == st1
    for i in (2, 3):
        d, c, st = out[i]
        assert not d.any() and c.shape == (0, 3) and st.n_events == 0 and st.n_inliers == 0
    assert out[2][2].n_nonzero == 0 and out[3][2].n_nonzero == 1 and out[3][2].lo == out[3][2].hi == 0.3
    assert out[0][2].n_inliers > 500 and out[4][2].n_inliers > 300
    # a 3-D array, depth only, and a still larger group
    big = np.stack([s.astype(np.float64) for s in group] * 3)
    out3 = eng.process_time_surfaces(big, want_cloud=False)
    assert len(out3) == 15
    for i, (d, c, st) in enumerate(out3):
        assert c is None and _same_bits(d, alone[i % 5][0]) and st == alone[i % 5][2]
    # the float32 member as a float32 group of its own == its float64 cast (f32 -> f64 is exact)
    d32, c32, _ = eng.process_time_surfaces(group[4][None], want_cloud=True)[0]
    assert _same_bits(d32, alone[4][0]) and _same_bits(c32, alone[4][1])


# ---- 5. XM_MEM_DEVICE -------------------------------------------------------------------------------------------------------------
def test_device_pointers_equal_host_pointers(tiny_maps):
    from x_maps_amd import _native as N
    eng = tiny_maps.engine
    rng = np.random.default_rng(5)
    shape = (C_TINY.cam_h, C_TINY.cam_w)
    px = shape[0] * shape[1]
    grp = np.stack([_random_surface(rng, shape, f, np.float32) for f in (1.0, 0.5, 0.0)])
    want = eng.process_time_surfaces(grp, want_cloud=True)
    n = len(grp)
    d_in = eng.to_device(grp)
    d_depth, d_cloud, d_stats = eng.dev_alloc(n * px * 4), eng.dev_alloc(n * px * 12), eng.dev_alloc(n * C.sizeof(N.xm_surface_stats))
    try:
        for _ in range(2):  # twice: consecutive asynchronous calls share the handle's scratch
            N.check(eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(d_in), N.XM_T_FLOAT32, n, N.XM_MEM_DEVICE, C.c_void_p(d_depth),
                                                      C.c_void_p(d_cloud), C.c_void_p(d_stats)))
        eng.sync()
        depth = np.empty((n,) + shape, np.float32)
        cloud = np.empty((n, px, 3), np.float32)
        stats = np.empty(n * C.sizeof(N.xm_surface_stats), np.uint8)
        eng.dev_download(depth, d_depth)
        eng.dev_download(cloud, d_cloud)
        eng.dev_download(stats, d_stats)
    finally:
        for p in (d_in, d_depth, d_cloud, d_stats):
            eng.dev_free(p)
    st = (N.xm_surface_stats * n).from_buffer(stats)
    for i, (d, c, s) in enumerate(want):
        assert _same_bits(depth[i], d) and _same_bits(cloud[i, :s.n_inliers], c)
        assert (st[i].n_nonzero, st[i].n_events, st[i].n_inliers) == (s.n_nonzero, s.n_events, s.n_inliers)
        assert (st[i].lo, st[i].hi, st[i].t_min, st[i].t_max) == (s.lo, s.hi, s.t_min, s.t_max)
    assert want[0][2].n_inliers > 500 and want[2][2].n_nonzero == 0


# ---- 6. not one of the K1 variants ------------------------------------------------------------------------------------------------
def test_path_counts_do_not_move(tiny_maps):
    eng = tiny_maps.engine
    rng = np.random.default_rng(1)
    before = eng.path_counts()
    out = eng.process_time_surfaces([_random_surface(rng, (C_TINY.cam_h, C_TINY.cam_w), 0.8, np.float64)] * 2, want_cloud=True)
    assert out[0][2].n_inliers > 0
    assert eng.path_counts() == before


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_errors(tiny_maps):
    from x_maps_amd import _native as N
    from x_maps_amd.engine import XMapsEngine
    shape = (C_TINY.cam_h, C_TINY.cam_w)
    surf = np.full(shape, 0.5)
    surf[0, 0] = 0.1
    with XMapsEngine(_with_cloud_tables(make_tables(C_TINY), 3), camera_perspective=False) as proj:
        with pytest.raises((ValueError, N.XMapsNativeError), match="camera-view"):
            proj.process_time_surfaces([np.zeros((proj.cam_h, proj.cam_w))])
    with XMapsEngine(make_tables(C_TINY), camera_perspective=True) as bare:  # no float maps, no Q
        assert bare.process_time_surfaces([surf])[0][2].n_events == surf.size - 1
        with pytest.raises(ValueError, match="Q"):
            bare.process_time_surfaces([surf], want_cloud=True)
        depth = np.empty(shape, np.float32)
        cloud = np.empty(shape + (3,), np.float32)
        args = (bare._h, C.c_void_p(surf.ctypes.data), N.XM_T_FLOAT64, 1, N.XM_MEM_HOST, C.c_void_p(depth.ctypes.data))
        assert bare._lib.xm_process_time_surfaces(*args, C.c_void_p(cloud.ctypes.data), None) == N.XM_ERR_INVALID
        assert "xm_surface_set_cloud_tables" in N.last_error()
        assert bare._lib.xm_process_time_surfaces(*args, None, None) == N.XM_OK
    eng = tiny_maps.engine
    for bad in (np.zeros((shape[0], shape[1] + 1)), np.zeros((2, shape[0] - 1, shape[1])), np.zeros(shape[1])):
        with pytest.raises(ValueError):
            eng.process_time_surfaces(bad if bad.ndim == 3 else [bad])
    with pytest.raises(ValueError):
        eng.process_time_surfaces([])
    depth = np.empty(shape, np.float32)
    for dtype, n in ((N.XM_T_INT64, 1), (7, 1), (N.XM_T_FLOAT64, 0), (N.XM_T_FLOAT64, -3)):
        rc = eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(surf.ctypes.data), dtype, n, N.XM_MEM_HOST,
                                               C.c_void_p(depth.ctypes.data), None, None)
        assert rc == N.XM_ERR_INVALID and N.last_error()


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[-1])
    return np.frombuffer(body, "<f4").reshape(n, 3)


def test_tool_switch_writes_the_same_files(tmp_path, g7):
    spec = importlib.util.spec_from_file_location("run_esl_on_arrival", os.path.join(ROOT, "tools", "run_esl_on_arrival.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(8)
    scans = [g7["raw_time_surface"], _random_surface(rng, (48, 64), 0.6, np.float32), _random_surface(rng, (48, 64), 0.9, np.float64)]
    got = {}
    for mode in (False, True):
        d = tmp_path / ("dev" if mode else "host")
        (d / "scans_np").mkdir(parents=True)
        for i, s in enumerate(scans):
            np.save(d / "scans_np" / f"scans{i:03d}.npy", s)
        rep = tool.depth_from_scans(str(d), None, 64, 64, point_clouds=True, tables=_g7_tables(g7), surfaces_on_device=mode, group=2)
        assert rep["scans_processed"] == 3 and rep["scans_empty"] == 0
        got[mode] = [(np.load(d / "x_maps" / "depth_init" / f"scans{i:03d}.npy"), _read_ply(d / "x_maps" / "pointcloud_init" / f"scans{i:03d}.ply"))
                     for i in range(3)]
    for (d0, c0), (d1, c1) in zip(got[False], got[True]):
        assert _same_bits(d0, d1) and _same_bits(c0, c1) and len(c0) > 300
