"""-m gpu: ESL-init on the device (xm_esl_init_*, csrc/xmaps_eslinit.hpp) bit for bit against the reference's own outputs (golden
G11) and the NumPy restatement tests/esl_init_ref.py.

Stage kernel (k_esl_stage: 256 columns of a row per block, the window offsets staged 1024 per pass): the fixture's 12 x 1100 and
3 x 2300 frames (4.3 and 9 tiles per row, neither width a multiple of 256: full, clipped and empty windows, every tie and
candidate-count case the fixture asserts) and a 5 x 700 frame on which every window is clipped; 1 / 70 on 300 columns for the
non-default bounds and 3 / 1500 on 1700 columns for a window that takes two passes.
Fused kernel (k_esl_fused: 64 camera pixels x 4 rows per block): a 37 x 13 camera -- neither a multiple of 64 nor of 4 -- over a
1100 x 20 rectified frame, random maps with entries outside both frames, float32 and float64 surfaces in groups of 1 and 5 (the
group holds an all-zero and a single-valued surface), both signs of P1[0, 3]: depth, disp_cam and the statistics all EQUAL; and
depth == f32(p1_03 / stage disparity[back map]), which holds the two kernels against each other."""
import ctypes as C
import os

import numpy as np
import pytest

import esl_init_cases as K
import esl_init_ref as R

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def g11(golden_dir):
    return dict(np.load(os.path.join(golden_dir, K.G11)))


def _stage_tables(proj_rect, **kw):
    """an object for the stage entry alone: a 1 x 1 camera whose maps point nowhere"""
    h, w = proj_rect.shape
    return dict({"cam_w": 1, "cam_h": 1, "rect_w": w, "rect_h": h, "cam_to_rect_map": np.full((h, w, 2), -1, np.int16),
                 "rect_to_cam_map": np.full((1, 1, 2), -1, np.int16), "proj_rect": proj_rect, "p1_03": 1.0}, **kw)


def _tables(rig, p1_03, **kw):
    return dict({"cam_w": rig["cam_w"], "cam_h": rig["cam_h"], "rect_w": rig["rect_w"], "rect_h": rig["rect_h"],
                 "cam_to_rect_map": rig["cam_to_rect"], "rect_to_cam_map": rig["rect_to_cam"], "proj_rect": rig["proj_rect"],
                 "p1_03": p1_03}, **kw)


@pytest.fixture(scope="module")
def rig():
    return K.make_rig()


@pytest.fixture(scope="module")
def want(rig):
    """the restatement's results, computed once: (dtype, surface index, sign) -> (depth, disp_cam, stats)"""
    out = {}
    for dt in (np.float32, np.float64):
        for i, s in enumerate(K.make_surfaces(rig, 5, dt)):
            for p in (812.25, -812.25):
                out[np.dtype(dt).name, i, p] = R.depth_init_fused(s, rig["cam_to_rect"], rig["rect_to_cam"], rig["proj_rect"], p)
    return out


@gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_stage_entry_equals_the_reference(g11, tag):
    from x_maps_amd.esl_init import EslInit
    cam, proj, ref = g11[f"{tag}_cam_rect"], g11[f"{tag}_proj_rect"], g11[f"{tag}_disparity"]
    assert cam.shape[1] % 256 != 0
    with EslInit(_stage_tables(proj)) as esl:
        got = esl.disparity_init(cam)
    assert got.dtype == np.uint16 and np.array_equal(got, ref)
    assert np.array_equal(got, R.disparity_init(cam, proj))


@gpu
def test_stage_entry_on_a_frame_of_clipped_windows():
    from x_maps_amd.esl_init import EslInit
    rng = np.random.default_rng(17)
    proj = K.projector_rows(rng, 5, 700)
    cam = rng.random((5, 700))
    cam[rng.random((5, 700)) < 0.3] = 0
    cam[rng.random((5, 700)) < 0.1] = -1.0
    cam[3, 256:512] = 0  # a tile without a positive pixel between two that have some
    want = R.disparity_init(cam, proj)
    assert np.count_nonzero(want) > 1000 and want.max() > 600
    with EslInit(_stage_tables(proj)) as esl:
        assert np.array_equal(esl.disparity_init(cam), want)
        assert not esl.disparity_init(np.zeros((5, 700))).any()  # every tile leaves early, and still writes its zeros


@gpu
@pytest.mark.parametrize("w,min_disp,max_disp", [(300, 1, 70), (1700, 3, 1500)])
def test_stage_entry_with_other_bounds(w, min_disp, max_disp):
    from x_maps_amd.esl_init import EslInit
    rng = np.random.default_rng(w + max_disp)
    proj = K.projector_rows(rng, 3, w, density=0.6)
    cam = rng.random((3, w))
    cam[rng.random((3, w)) < 0.4] = 0
    want = R.disparity_init(cam, proj, min_disp, max_disp)
    assert want.max() == max_disp - 1 and want[want > 0].min() == min_disp  # (both ends of the window win somewhere)
    with EslInit(_stage_tables(proj, min_disp=min_disp, max_disp=max_disp)) as esl:
        assert np.array_equal(esl.disparity_init(cam), want)


@gpu
@pytest.mark.parametrize("p1_03", [812.25, -812.25])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_entry_equals_the_restatement(rig, want, dtype, n, p1_03):
    from x_maps_amd.esl_init import EslInit
    assert rig["cam_w"] % 64 and rig["cam_h"] % 4
    surfaces = K.make_surfaces(rig, 5, dtype)[:n]
    with EslInit(_tables(rig, p1_03)) as esl:
        res = esl.depths_from_time_surfaces(surfaces, want_disparity=True)
        only_depth = esl.depths_from_time_surfaces(list(surfaces))  # (a list; disp_cam_out == NULL)
    assert len(res) == n
    for i, (depth, disp, st) in enumerate(res):
        w_depth, w_disp, w_st = want[np.dtype(dtype).name, i, p1_03]
        assert depth.dtype == np.float32 and disp.dtype == np.uint16
        assert np.array_equal(disp, w_disp), i
        assert np.array_equal(depth.view(np.uint32), w_depth.view(np.uint32)), i
        assert np.all(np.isfinite(depth)) and np.all((depth == 0) == (disp == 0))  # disparity 0 -> depth 0, never inf
        assert {k: getattr(st, k) for k in w_st} == w_st, (i, st, w_st)
        assert np.array_equal(only_depth[i][0], depth) and only_depth[i][1] is None
        if i in (1, 2):  # all zero; a single value: zero maps, and the statistics say why
            assert not depth.any() and st.n_searched == 0 and (st.n_nonzero == 0) == (i == 1) and st.lo == st.hi
        else:
            assert st.n_matched > 20 and np.sign(depth[disp != 0]).min() == np.sign(depth[disp != 0]).max() == np.sign(p1_03)


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_depth_is_the_stage_disparity_through_the_back_map(rig, dtype):
    from x_maps_amd.esl_init import EslInit
    p1_03 = -5821.0837
    s = K.make_surfaces(rig, 1, dtype)[0]
    v, _ = R.normalise(s)
    cam_rect = R.remap_nearest_i16(v, rig["cam_to_rect"])
    with EslInit(_tables(rig, p1_03)) as esl:
        staged = esl.disparity_init(cam_rect)
        depth, disp, st = esl.depths_from_time_surfaces(s[None], want_disparity=True)[0]
    back = R.remap_nearest_i16(staged, rig["rect_to_cam"])
    assert st.n_matched == np.count_nonzero(back) > 20
    assert np.array_equal(disp, back)
    with np.errstate(divide="ignore"):
        w_depth = np.where(back != 0, np.float64(p1_03) / back.astype(np.float64), 0.0).astype(np.float32)
    assert np.array_equal(depth.view(np.uint32), w_depth.view(np.uint32))


@gpu
def test_fused_entry_with_other_bounds_and_device_memory(rig):
    """min_disp / max_disp 1 / 70 on a 300-column frame; the same group through XM_MEM_DEVICE pointers"""
    import torch
    from x_maps_amd.esl_init import EslInit
    small = K.make_rig(seed=9, rect_w=300, rect_h=16, max_disp=70)
    surfaces = K.make_surfaces(small, 3, np.float32)
    wants = [R.depth_init_fused(s, small["cam_to_rect"], small["rect_to_cam"], small["proj_rect"], 99.5, 1, 70) for s in surfaces]
    assert wants[0][2]["n_matched"] > 20 and wants[0][1].max() > 40 and wants[0][1][wants[0][1] > 0].min() < 10
    with EslInit(_tables(small, 99.5, min_disp=1, max_disp=70)) as esl:
        res = esl.depths_from_time_surfaces(surfaces, want_disparity=True)
        d_in = torch.from_numpy(surfaces).cuda()
        d_depth = torch.full(surfaces.shape, -1.0, dtype=torch.float32, device="cuda")
        d_disp = torch.full(surfaces.shape, 7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        esl.time_surfaces_device(d_in.data_ptr(), np.float32, 3, d_depth.data_ptr(), d_disp.data_ptr())
        dev_depth, dev_disp = d_depth.cpu().numpy(), d_disp.cpu().numpy().view(np.uint16)
    for i, (depth, disp, st) in enumerate(res):
        assert np.array_equal(disp, wants[i][1]) and np.array_equal(depth.view(np.uint32), wants[i][0].view(np.uint32))
        assert {k: getattr(st, k) for k in wants[i][2]} == wants[i][2]
        assert np.array_equal(dev_disp[i], disp) and np.array_equal(dev_depth[i].view(np.uint32), depth.view(np.uint32))


@gpu
def test_invalid_configurations_are_refused(rig):
    from x_maps_amd import _native as N
    from x_maps_amd.esl_init import EslInit
    for lo, hi in ((-1, 900), (5, 5), (9, 5), (5, 65536), (0, 65536)):
        with pytest.raises(ValueError):
            EslInit(_tables(rig, 1.0, min_disp=lo, max_disp=hi))
    lib = N.load_library()
    h = C.c_void_p()
    cfg = N.xm_esl_init_config(C.sizeof(N.xm_esl_init_config), rig["cam_w"], rig["cam_h"], rig["rect_w"], rig["rect_h"], 5, 900, 0, 1.0,
                               rig["cam_to_rect"].ctypes.data, rig["rect_to_cam"].ctypes.data, rig["proj_rect"].ctypes.data)
    for field, bad in (("struct_size", 8), ("cam_width", 0), ("rect_height", -3), ("proj_rect", None), ("max_disp", 65536)):
        keep = getattr(cfg, field)
        setattr(cfg, field, bad)
        assert lib.xm_esl_init_create(0, C.byref(cfg), C.byref(h)) == N.XM_ERR_INVALID and not h.value and N.last_error()
        setattr(cfg, field, keep)
    assert lib.xm_esl_init_create(0, C.byref(cfg), C.byref(h)) == N.XM_OK and h.value
    depth = np.empty((rig["cam_h"], rig["cam_w"]), np.float32)
    s = K.make_surfaces(rig, 1, np.float32)
    args = (s.ctypes.data, N.XM_T_FLOAT32, 1, N.XM_MEM_HOST, depth.ctypes.data, None, None)
    for pos, bad in ((1, N.XM_T_INT64), (2, 0), (3, 7), (0, None), (4, None)):
        a = list(args)
        a[pos] = bad
        assert lib.xm_esl_init_time_surfaces(h, *a) == N.XM_ERR_INVALID
    assert lib.xm_esl_init_time_surfaces(None, *args) == N.XM_ERR_INVALID
    assert lib.xm_esl_init_stage_disparity(h, None, None) == N.XM_ERR_INVALID
    assert lib.xm_esl_init_time_surfaces(h, *args) == N.XM_OK  # (the object is still good)
    lib.xm_esl_init_destroy(h)
    lib.xm_esl_init_destroy(None)
    with pytest.raises(ValueError):
        with EslInit(_tables(rig, 1.0)) as esl:
            esl.disparity_init(np.zeros((3, 3)))


@gpu
def test_on_arrival_tool_writes_depth_init_and_the_table_row(rig, tmp_path):
    """tools/run_esl_on_arrival.py's ESL-init half on a sequence directory: the files it writes are the entry's maps, an all-zero
    scan is skipped as the reference skips it, and the "ESL (init)" row comes from the same function as the X-maps row"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import run_esl_on_arrival as T
    finally:
        sys.path.pop(0)
    from x_maps_amd.esl_init import EslInit
    from x_maps_amd.eval_table import esl_init_table_row, x_maps_table_row
    surfaces = K.make_surfaces(rig, 5, np.float32)
    os.makedirs(tmp_path / "scans_np")
    for i, s in enumerate(surfaces):
        np.save(tmp_path / "scans_np" / f"scans{i:03d}.npy", s)
    tables = _tables(rig, 8000.0)
    rep = T.esl_init_from_scans(str(tmp_path), None, 0, 0, tables=tables, group=2)
    assert rep["scans_found"] == 5 and rep["scans_processed"] == 4 and rep["scans_empty"] == 1
    with EslInit(tables) as esl:
        want = esl.depths_from_time_surfaces(surfaces)
    written = sorted(os.listdir(tmp_path / "esl" / "depth_init"))
    assert written == [f"scans{i:03d}.npy" for i in (0, 2, 3, 4)]
    for name in written:
        assert np.array_equal(np.load(tmp_path / "esl" / "depth_init" / name), want[int(name[5:8])][0])
    row = esl_init_table_row(str(tmp_path))
    assert "no ground truth" in row["error"] and row["esl_init_files"] == 4
    assert x_maps_table_row(str(tmp_path))["x_maps_files"] == 0  # (the same code, the other directory)
    os.makedirs(tmp_path / "esl" / "depth_optim_filtered")
    for name in written:  # the estimate as its own ground truth: every pixel the filters keep is hit exactly
        np.save(tmp_path / "esl" / "depth_optim_filtered" / name, np.load(tmp_path / "esl" / "depth_init" / name))
    row = esl_init_table_row(str(tmp_path), 20, 500)
    assert "error" not in row and row["scans"] == 4 and row["rmse"] == 0.0


def test_shapes_sit_astride_the_kernels_tiles():
    """CPU: the constants the shapes above were chosen against are the kernels'"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "x_maps_amd", "csrc", "xmaps_eslinit.hpp")).read()
    common = open(os.path.join(root, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()  # (BLOCK: shared with the host's plan)
    assert re.search(r"constexpr int BLOCK = 256;", common)
    assert re.search(r"constexpr int ESL_TX = BLOCK;", src) and re.search(r"constexpr int ESL_CHUNK = 1024;", src)
    assert re.search(r"constexpr int ESL_FW = 64, ESL_FR = BLOCK / 64;", src)
