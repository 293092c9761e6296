"""-m gpu: MC3D on the device (xm_mc3d_*, csrc/xmaps_mc3d.hpp) bit for bit against the reference's own outputs (golden G12) and the
NumPy restatement tests/mc3d_ref.py.  No tolerances: disparities, depth bits and statistics are compared for equality.

The shapes are golden G12's three rigs: cameras of 37 x 13, 70 x 9 and 45 x 6 pixels -- no multiple of the kernel's 64 x 4 pixels
per block; 70 columns take two blocks, 13 and 9 rows four and three -- against projectors of 5 x 100, 6 x 990 and 7 x 1920: windows
of 12 entries (narrower than a wave), 132 (two full trips of 64 and a partial one) and 256 (the reference's: four trips).  The
search without the blur is held against the reference; with it -- every border and corner pixel lit -- against the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import mc3d_cases as K
import mc3d_ref as R

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs(golden_dir):
    from x_maps_amd.mc3d import mc3d_int_maps
    return K.load_rigs(golden_dir, mc3d_int_maps)


@pytest.fixture(scope="module")
def want(rigs):
    """the restatement on the groups, computed once: (rig, dtype name, surface index, sign, blur) -> (depth, disp, stats)"""
    out = {}
    for name in K.RIGS:
        rig = rigs[name]
        for dt in (np.float32, np.float64):
            for i, s in enumerate(K.group(rig, dt)):
                for p in K.P1_03:
                    for blur in (True, False):
                        out[name, np.dtype(dt).name, i, p, blur] = R.mc3d(s, rig["cam_map"], rig["proj_map"], p, blur=blur)
    return out


def _same(got, want_):
    depth, disp, st = got
    w_depth, w_disp, w_st = want_
    assert depth.dtype == np.float32 and disp.dtype == np.uint16
    assert np.array_equal(disp, w_disp)
    assert np.array_equal(depth.view(np.uint32), w_depth.view(np.uint32))
    assert np.all(np.isfinite(depth)) and np.all((depth == 0) == (disp == 0))  # disparity 0 -> depth 0, never inf
    assert {k: getattr(st, k) for k in R.STAT_KEYS} == w_st, (st, w_st)


@gpu
@pytest.mark.parametrize("name", K.RIGS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_search_equals_the_reference(rigs, name, dtype):
    from x_maps_amd.mc3d import Mc3d
    rig = rigs[name]
    surf = rig[f"surf_{dtype}"]
    for sign, key in enumerate(("depth_pos", "depth_neg")):
        with Mc3d(K.tables(rig, K.P1_03[sign])) as mc:
            depth, disp, st = mc.depths_from_time_surfaces(surf, want_disparity=True, blur=False)[0]
        assert np.array_equal(disp, rig[f"disp_{dtype}"])
        assert st.n_matched == np.count_nonzero(disp) > 50 and st.n_positive == (surf > 0).sum() and st.n_disp_overflow == 0
        if dtype == "f32":  # (the fixture's depths belong to the float32 surface's disparities)
            assert np.array_equal(depth.view(np.uint32), rig[key].astype(np.float32).view(np.uint32))
        _same((depth, disp, st), R.mc3d(surf, rig["cam_map"], rig["proj_map"], K.P1_03[sign], blur=False))


@gpu
@pytest.mark.parametrize("name", K.RIGS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_blurred_search_equals_the_restatement(rigs, name, dtype):
    from x_maps_amd.mc3d import Mc3d
    rig = rigs[name]
    s = K.dense_surface(rig, dtype, 1)
    v = R.median_blur3(s)
    h, w = s.shape
    assert all(v[i, j] > 0 for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)))
    assert (v[0] > 0).any() and (v[-1] > 0).any() and (v[:, 0] > 0).any() and (v[:, -1] > 0).any() and ((v > 0) != (s > 0)).any()
    w_blur = R.mc3d(s, rig["cam_map"], rig["proj_map"], K.P1_03[0])
    w_plain = R.mc3d(s, rig["cam_map"], rig["proj_map"], K.P1_03[0], blur=False)
    assert w_blur[2]["n_matched"] > 20 and not np.array_equal(w_blur[1], w_plain[1])
    ring = np.ones((h, w), bool)
    ring[1:-1, 1:-1] = False
    assert (w_blur[1][ring] > 0).sum() >= 4  # (disparities on the ring: the replicated border decides them)
    with Mc3d(K.tables(rig, K.P1_03[0])) as mc:
        _same(mc.depths_from_time_surfaces(s, want_disparity=True)[0], w_blur)
        _same(mc.depths_from_time_surfaces(s, want_disparity=True, blur=False)[0], w_plain)


@gpu
@pytest.mark.parametrize("p1_03", K.P1_03)
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["a", "c"])
def test_groups_with_degenerate_surfaces(rigs, want, name, dtype, n, p1_03):
    from x_maps_amd.mc3d import Mc3d
    rig = rigs[name]
    surfaces = K.group(rig, dtype)[:n]
    with Mc3d(K.tables(rig, p1_03)) as mc:
        res = mc.depths_from_time_surfaces(surfaces, want_disparity=True)
        only_depth = mc.depths_from_time_surfaces(list(surfaces))  # (a list; disp_out == NULL)
    assert len(res) == n
    for i, got in enumerate(res):
        _same(got, want[name, np.dtype(dtype).name, i, p1_03, True])
        depth, disp, st = got
        assert np.array_equal(only_depth[i][0].view(np.uint32), depth.view(np.uint32)) and only_depth[i][1] is None
        assert {k: getattr(only_depth[i][2], k) for k in R.STAT_KEYS} == {k: getattr(st, k) for k in R.STAT_KEYS}
        if i == 1:  # all zero: zero maps, zero counts
            assert not depth.any() and not any(getattr(st, k) for k in R.STAT_KEYS)
        elif i == 2:  # every value >= 1: every pixel inside the rect names no projector pixel
            assert not depth.any() and st.n_positive == depth.size and st.n_out_of_range == st.n_in_rect > 0 and st.n_matched == 0
        elif i >= 3:
            assert st.n_matched > 20 and np.sign(depth[disp != 0]).min() == np.sign(depth[disp != 0]).max() == np.sign(p1_03)


@gpu
def test_device_memory_and_other_parameters(rigs):
    """the same group through XM_MEM_DEVICE pointers; nc / max_row_diff / rect limits other than the reference's; a disparity
    beyond 65535 is stored as 0 and counted"""
    import torch
    from x_maps_amd.mc3d import Mc3d
    rig = rigs["b"]
    surfaces = K.group(rig, np.float32)
    kw = dict(nc=40, max_row_diff=20, rect_x_limit=900, rect_y_limit=11)
    wants = [R.mc3d(s, rig["cam_map"], rig["proj_map"], 99.5, **kw) for s in surfaces]
    plain = R.mc3d(surfaces[3], rig["cam_map"], rig["proj_map"], 99.5)
    assert wants[3][2]["n_matched"] > 20 and not np.array_equal(wants[3][1], plain[1])
    with Mc3d(K.tables(rig, 99.5, **kw)) as mc:
        res = mc.depths_from_time_surfaces(surfaces, want_disparity=True)
        d_in = torch.from_numpy(surfaces).cuda()
        d_depth = torch.full(surfaces.shape, -1.0, dtype=torch.float32, device="cuda")
        d_disp = torch.full(surfaces.shape, 7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        mc.time_surfaces_device(d_in.data_ptr(), np.float32, len(surfaces), d_depth.data_ptr(), d_disp.data_ptr())
        dev_depth, dev_disp = d_depth.cpu().numpy(), d_disp.cpu().numpy().view(np.uint16)
    for i, got in enumerate(res):
        _same(got, wants[i])
        assert np.array_equal(dev_disp[i], got[1]) and np.array_equal(dev_depth[i].view(np.uint32), got[0].view(np.uint32))
    far = rig["proj_map"].copy()
    far[..., 0] = np.where(far[..., 0] == R.POISON, R.POISON, far[..., 0] + 70000)
    w_far = R.mc3d(surfaces[0], rig["cam_map"], far, 99.5, blur=False)
    assert w_far[2]["n_disp_overflow"] > 50 and w_far[2]["n_matched"] == 0
    with Mc3d(dict(K.tables(rig, 99.5), proj_map=far)) as mc:
        _same(mc.depths_from_time_surfaces(surfaces[0], want_disparity=True, blur=False)[0], w_far)


@gpu
def test_invalid_configurations_are_refused(rigs):
    from x_maps_amd import _native as N
    from x_maps_amd.mc3d import Mc3d
    rig = rigs["a"]
    for kw in (dict(nc=-1), dict(nc=51), dict(max_row_diff=-1), dict(rect_x_limit=-5, rect_y_limit=10), dict(rect_x_limit=2 ** 30, rect_y_limit=10),
               dict(nc=50, max_row_diff=2 ** 26)):  # (the last: a key of 27 + 7 bits)
        with pytest.raises(ValueError):
            Mc3d(K.tables(rig, 1.0, **kw))
    with pytest.raises(ValueError):
        Mc3d(K.tables(rig, 1.0, nc=50, max_row_diff=2 ** 25 - 2))  # (the largest key would be exactly 2^32)
    with Mc3d(K.tables(rig, 1.0, nc=50, max_row_diff=2 ** 25 - 3)):  # (2 * nc == proj_height and a key of 32 bits are fine)
        pass
    lib = N.load_library()
    h = C.c_void_p()
    big = np.zeros((4097, 4096, 2), np.int32)  # proj_width * proj_height == 2^24 + 4096
    cfg = N.xm_mc3d_config(C.sizeof(N.xm_mc3d_config), rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 0, 0, 0, 0, 0, 1.0,
                           rig["cam_map"].ctypes.data, rig["proj_map"].ctypes.data)
    for field, bad in (("struct_size", 8), ("cam_width", 0), ("proj_height", -3), ("proj_map", None), ("cam_map", None), ("nc", 51)):
        keep = getattr(cfg, field)
        setattr(cfg, field, bad)
        assert lib.xm_mc3d_create(0, C.byref(cfg), C.byref(h)) == N.XM_ERR_INVALID and not h.value and N.last_error()
        setattr(cfg, field, keep)
    cfg_big = N.xm_mc3d_config(C.sizeof(N.xm_mc3d_config), rig["cam_w"], rig["cam_h"], 4096, 4097, 0, 0, 0, 0, 0, 1.0,
                               rig["cam_map"].ctypes.data, big.ctypes.data)
    assert lib.xm_mc3d_create(0, C.byref(cfg_big), C.byref(h)) == N.XM_ERR_INVALID and "2^24" in N.last_error()
    assert lib.xm_mc3d_create(0, C.byref(cfg), C.byref(h)) == N.XM_OK and h.value
    depth = np.empty((rig["cam_h"], rig["cam_w"]), np.float32)
    s = np.ascontiguousarray(rig["surf_f32"])
    args = (s.ctypes.data, N.XM_T_FLOAT32, 1, N.XM_MEM_HOST, 0, depth.ctypes.data, None, None)
    for pos, bad in ((1, N.XM_T_INT64), (2, 0), (2, -1), (3, 7), (4, 2), (0, None), (5, None)):
        a = list(args)
        a[pos] = bad
        assert lib.xm_mc3d_time_surfaces(h, *a) == N.XM_ERR_INVALID
    assert lib.xm_mc3d_time_surfaces(None, *args) == N.XM_ERR_INVALID
    assert lib.xm_mc3d_time_surfaces(h, *args) == N.XM_OK  # (the object is still good)
    lib.xm_mc3d_destroy(h)
    lib.xm_mc3d_destroy(None)
    with pytest.raises(ValueError):
        Mc3d(dict(K.tables(rig, 1.0), cam_map=rig["cam_map"][:-1]))


@gpu
def test_on_arrival_tool_writes_depth_and_both_table_rows(rigs, tmp_path):
    """tools/run_esl_on_arrival.py's MC3D half on a sequence directory: the files it writes are the entry's maps, an all-zero scan
    is skipped as the reference skips it; mc3d_table_rows against the rows the same recipe (create_evaluation_table.py:126-161)
    gives on the restatement's maps, spelt out here"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import run_esl_on_arrival as T
    finally:
        sys.path.pop(0)
    from x_maps_amd.eval_metrics import evaluation_stats
    from x_maps_amd.eval_table import combine_depth_maps, load_and_filter, mc3d_table_rows
    rig = rigs["c"]
    p1_03 = 120000.0  # (disparities 1000 .. 6000 land inside the table's 20 .. 120)
    surfaces = np.stack([np.zeros((rig["cam_h"], rig["cam_w"]), np.float32) if i == 1 else K.dense_surface(rig, np.float32, 10 + i)
                         for i in range(5)])  # (dense scans: their medians, and the ground truth's, keep most pixels)
    os.makedirs(tmp_path / "scans_np")
    for i, s in enumerate(surfaces):
        np.save(tmp_path / "scans_np" / f"scans{i:03d}.npy", s)
    tables = K.tables(rig, p1_03)
    rep = T.mc3d_from_scans(str(tmp_path), None, 0, 0, tables=tables, group=2)
    assert rep["scans_found"] == 5 and rep["scans_processed"] == 4 and rep["scans_empty"] == 1
    ref_maps = {i: R.mc3d(s, rig["cam_map"], rig["proj_map"], p1_03)[0] for i, s in enumerate(surfaces)}
    written = sorted(os.listdir(tmp_path / "mc3d" / "depth"))
    assert written == [f"scans{i:03d}.npy" for i in (0, 2, 3, 4)]
    for name in written:
        assert np.array_equal(np.load(tmp_path / "mc3d" / "depth" / name), ref_maps[int(name[5:8])])
    rows = mc3d_table_rows(str(tmp_path))
    assert "no ground truth" in rows["mc3d"]["error"] and rows["mc3d"]["mc3d_files"] == 4 and "error" in rows["mc3d_1s"]
    # a ground truth: the restatement's maps, each with a band of pixels moved by half a unit and another band emptied
    os.makedirs(tmp_path / "esl" / "depth_optim_filtered")
    gts = []
    for k, i in enumerate((0, 2, 3, 4)):
        gt = ref_maps[i].copy()
        gt[k % gt.shape[0]] += np.float32(0.5) * (gt[k % gt.shape[0]] > 0)
        gt[:, k] = 0
        np.save(tmp_path / "esl" / "depth_optim_filtered" / f"scans{i:03d}.npy", gt)
        gts.append(str(tmp_path / "esl" / "depth_optim_filtered" / f"scans{i:03d}.npy"))
    rows = mc3d_table_rows(str(tmp_path), 20, 120)
    ref_dir = tmp_path / "ref_maps"
    os.makedirs(ref_dir)
    ests = []
    for i in (0, 2, 3, 4):
        np.save(ref_dir / f"scans{i:03d}.npy", ref_maps[i])
        ests.append(str(ref_dir / f"scans{i:03d}.npy"))
    gt_comb, _, _ = combine_depth_maps(gts, 20, 120)
    est_comb, _, _ = combine_depth_maps(ests, 20, 120)
    per, one_sec = [], []
    for g, e in zip(gts, ests):
        gt = load_and_filter(g, gt_comb, 20, 120)
        a, b = evaluation_stats(load_and_filter(e, gt_comb, 20, 120), gt), evaluation_stats(est_comb, gt)
        per.append((a.fillrate, a.rmse))
        one_sec.append((b.fillrate, b.rmse))
    for key, lst in (("mc3d", per), ("mc3d_1s", one_sec)):
        fr, rmse = np.mean(np.array(lst, np.float64), axis=0)
        assert "error" not in rows[key] and rows[key]["scans"] == 4
        assert rows[key]["fill_rate"] == float(fr) and rows[key]["rmse"] == float(rmse)
    assert 0 < rows["mc3d"]["fill_rate"] <= 1 and rows["mc3d"]["rmse"] > 0 and rows["mc3d"] != rows["mc3d_1s"]


def test_shapes_sit_astride_the_kernels_tiles(rigs):
    """CPU: the constants the shapes above were chosen against are the kernel's"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    geo = open(os.path.join(root, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()
    assert re.search(r"constexpr int BLOCK = 256;", geo)
    assert re.search(r"constexpr int MC3D_FW = 64, MC3D_FR = BLOCK / 64, MC3D_N_CNT = 7;", geo) and len(R.STAT_KEYS) == 7
    assert re.search(r"constexpr int MC3D_POISON = -2147483647 - 1, MC3D_SAT = 1 << 30;", geo)
    assert [(r["cam_w"], r["cam_h"]) for r in (rigs[n] for n in K.RIGS)] == [(37, 13), (70, 9), (45, 6)]
    assert [2 * int(rigs[n]["proj_h"] / 15) for n in K.RIGS] == [12, 132, 256]
