"""-m gpu: ESL's depth optimisation on the device (xm_esl_optim_*, csrc/xmaps_esloptim.hpp) bit for bit against the reference's own
outputs (golden G13: depth_optimization on the installed scipy) and the scalar restatement tests/esl_optim_ref.py.  No tolerances
and no pixel left out: depth bits, evaluation counts and statistics are compared for equality -- a difference is an operation-order
bug, not noise.  Outputs are pre-filled with NaN / 0xFFFF, so an unwritten pixel shows.

Shapes: G13's rigs are 28 x 20 and 26 x 21 cameras (one block wide, five and six blocks tall); the seeded rigs sit astride the
kernel's 64 pixels per wave and 4 rows per block -- 63 x 7, 64 x 8, 65 x 9 -- and 7 x 7 is the smallest camera a window of 3 admits,
one optimised pixel, which a group of 65 538 surfaces (beyond a grid dimension's 65 535) repeats."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import esl_optim_cases as K
import esl_optim_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g13(golden_dir):
    return K.load_g13(golden_dir)


@pytest.fixture(scope="module")
def small():
    """a seeded 20 x 15 rig, its group of five surfaces in both dtypes, and the restatement on each: computed once"""
    rig = K.make_rig(20, 15, 40, 64, 41)
    rr = K.ref_rig(rig)
    want = {}
    for dt in (np.float32, np.float64):
        for i, s in enumerate(K.group(rig, dt, 5)):
            want[np.dtype(dt).name, i] = R.depth_optim(rr, s, rig["depth_init"])
    return rig, want


def run(opt, surfaces, depth_init, want_stats=True):
    """xm_esl_optim_time_surfaces on host memory with pre-filled outputs -> (depth [n], nfev [n], [stats dict])"""
    from x_maps_amd import _native as N
    grp = np.ascontiguousarray(surfaces if surfaces.ndim == 3 else surfaces[None])
    d0 = np.ascontiguousarray(np.broadcast_to(depth_init, grp.shape), dtype=np.float32)
    n = len(grp)
    depth = np.full(grp.shape, np.nan, np.float32)
    nfev = np.full(grp.shape, 0xFFFF, np.uint16)
    st = (N.xm_esl_optim_stats * n)()
    N.check(opt._lib.xm_esl_optim_time_surfaces(opt._h, grp.ctypes.data, N.XM_T_FLOAT32 if grp.dtype == np.float32 else N.XM_T_FLOAT64, n,
                                                N.XM_MEM_HOST, d0.ctypes.data, depth.ctypes.data, nfev.ctypes.data, C.cast(st, C.c_void_p)))
    return depth, nfev, [{k: getattr(s, k) for k in R.STAT_KEYS} for s in st] if want_stats else None


def same(depth, nfev, st, want):
    w_depth, w_nfev, w_st = want
    assert not np.isnan(depth).any() and not (nfev == 0xFFFF).any()  # (every pixel was written)
    assert np.array_equal(nfev, w_nfev)
    assert np.array_equal(depth.view(np.uint32), w_depth.view(np.uint32))
    assert st == w_st, (st, w_st)


@gpu
@pytest.mark.parametrize("name", K.G13_RIGS)
def test_depth_and_nfev_equal_the_reference_on_every_pixel(g13, name):
    from x_maps_amd.esl_optim import EslOptim
    rig = g13[name]
    with EslOptim(K.tables(rig)) as opt:
        depth, nfev, st = run(opt, rig["surface"], rig["depth_init"])
    print(name, "pixels differing: depth", int((depth[0].view(np.uint32) != rig["depth_optim"].view(np.uint32)).sum()), "nfev",
          int((nfev[0] != rig["nfev"]).sum()), st[0])
    assert not np.isnan(depth).any()
    assert np.array_equal(nfev[0], rig["nfev"])
    assert np.array_equal(depth[0].view(np.uint32), rig["depth_optim"].view(np.uint32))
    assert st[0]["n_optimised"] == np.count_nonzero(rig["nfev"]) >= 200 and st[0]["n_evals"] == int(rig["nfev"].sum())
    assert st[0]["n_hit_limit"] == 0 and st[0]["n_bad_bounds"] == 0


@gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_groups_with_degenerate_surfaces(small, dtype, n):
    from x_maps_amd.esl_optim import EslOptim
    rig, want = small
    surfaces = K.group(rig, dtype, n)
    with EslOptim(K.tables(rig)) as opt:
        depth, nfev, st = run(opt, surfaces, rig["depth_init"])
        res = opt.depths_from_time_surfaces(list(surfaces), [rig["depth_init"]] * n, want_nfev=True)
        only_depth = opt.depths_from_time_surfaces(surfaces, np.stack([rig["depth_init"]] * n))
    for i in range(n):
        w = want[np.dtype(dtype).name, i]
        same(depth[i], nfev[i], st[i], w)
        same(res[i][0], res[i][1], {k: getattr(res[i][2], k) for k in R.STAT_KEYS}, w)
        assert np.array_equal(only_depth[i][0].view(np.uint32), depth[i].view(np.uint32)) and only_depth[i][1] is None
        if i in (1, 2):  # all zero; hi == lo: zero maps, nothing optimised
            assert not depth[i].any() and not nfev[i].any() and st[i]["n_optimised"] == st[i]["n_evals"] == 0
            assert (st[i]["lo"], st[i]["hi"]) == ((0.0, 0.0) if i == 1 else (0.375, 0.375))
        else:
            assert st[i]["n_optimised"] > 80 and st[i]["n_evals"] > 20 * st[i]["n_optimised"]


@gpu
def test_chained_on_the_device_behind_esl_init(small):
    """XM_MEM_DEVICE: depth_init is the buffer xm_esl_init_time_surfaces has just filled"""
    import torch
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    from x_maps_amd.esl_optim import EslOptim, build_esl_optim_tables
    rig, _ = small
    cp = CamProjCalibrationParams(rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 3 * rig["proj_w"], 3 * rig["proj_h"], rig["cam_K"],
                                  rig["cam_D"], rig["proj_K"], rig["proj_D"], rig["R"], rig["T"].reshape(3, 1))
    t_opt = build_esl_optim_tables(cp)
    surfaces = K.group(rig, np.float32, 4)
    with EslInit(build_esl_init_tables(cp)) as esl, EslOptim(t_opt) as opt:
        d_in = torch.from_numpy(surfaces).cuda()
        d_init = torch.full(surfaces.shape, -1.0, dtype=torch.float32, device="cuda")
        d_out = torch.full(surfaces.shape, float("nan"), dtype=torch.float32, device="cuda")
        d_nfev = torch.full(surfaces.shape, -1, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        esl.time_surfaces_device(d_in.data_ptr(), np.float32, 4, d_init.data_ptr())
        opt.time_surfaces_device(d_in.data_ptr(), np.float32, 4, d_init.data_ptr(), d_out.data_ptr(), d_nfev.data_ptr())
        init, out, nfev = d_init.cpu().numpy(), d_out.cpu().numpy(), d_nfev.cpu().numpy().view(np.uint16)
        host = [e[0] for e in esl.depths_from_time_surfaces(surfaces)]
    rr = R.Rig(t_opt["cam_K"], t_opt["cam_D"], t_opt["proj_K"], t_opt["proj_D"], t_opt["Rt"], t_opt["proj_surface"], t_opt["p1_03"])
    for i in range(4):
        assert np.array_equal(init[i].view(np.uint32), host[i].view(np.uint32))
        w_depth, w_nfev, w_st = R.depth_optim(rr, surfaces[i], init[i])
        assert np.array_equal(nfev[i], w_nfev) and np.array_equal(out[i].view(np.uint32), w_depth.view(np.uint32))
        assert (w_st["n_optimised"] > 50) == (i in (0, 3)) and not np.isnan(out[i]).any()


@gpu
def test_other_windows_limits_and_tolerances(small):
    from x_maps_amd.esl_optim import EslOptim
    rig, want = small
    s, d0 = rig["surface"], rig["depth_init"]
    plain = want["float64", 0]
    # window_size 5: a border of 5, patches of 5 x 5; window_size 1: a border of 1, the pixel alone
    for ws in (5, 1, 7):
        w = R.depth_optim(K.ref_rig(rig, window_size=ws), s, d0)
        with EslOptim(K.tables(rig, window_size=ws)) as opt:
            depth, nfev, st = run(opt, s, d0)
        same(depth[0], nfev[0], st[0], w)
        assert st[0]["n_optimised"] == np.count_nonzero(d0[ws:-ws, ws:-ws] > 0) > 0 and not np.array_equal(w[0], plain[0])
    # max_iter 5: every pixel leaves through the limit
    w = R.depth_optim(K.ref_rig(rig), s, d0, max_iter=5)
    with EslOptim(K.tables(rig, max_iter=5)) as opt:
        depth, nfev, st = run(opt, s, d0)
    same(depth[0], nfev[0], st[0], w)
    assert st[0]["n_hit_limit"] == st[0]["n_optimised"] == plain[2]["n_optimised"] and set(np.unique(nfev)) == {0, 5}
    # max_iter 1: scipy evaluates twice before it looks at the limit
    w = R.depth_optim(K.ref_rig(rig), s, d0, max_iter=1)
    with EslOptim(K.tables(rig, max_iter=1)) as opt:
        depth, nfev, st = run(opt, s, d0)
    same(depth[0], nfev[0], st[0], w)
    assert set(np.unique(nfev)) == {0, 2}
    # xatol 0.25: parabolic steps within tol2 of a bound, moved to tol1 (the case golden G13 cannot hold)
    w = R.depth_optim(K.ref_rig(rig), s, d0, xatol=0.25, want_trace=True)
    assert any(step == "parabolic_tol1" for tr in w[3].values() for step, _ in tr)
    with EslOptim(K.tables(rig, xatol=0.25)) as opt:
        depth, nfev, st = run(opt, s, d0)
    same(depth[0], nfev[0], st[0], w[:3])
    assert st[0]["n_evals"] < plain[2]["n_evals"]
    # a negative P1[0, 3] inverts every bound, an infinite depth_init makes them NaN: written 0 and counted
    d_inf = d0.copy()
    d_inf[7, 9] = np.inf
    for p1_03, d in ((-rig["p1_03"], d0), (rig["p1_03"], d_inf)):
        w = R.depth_optim(K.ref_rig(rig, p1_03=p1_03), s, d)
        with EslOptim(K.tables(rig, p1_03=p1_03)) as opt:
            depth, nfev, st = run(opt, s, d)
        same(depth[0], nfev[0], st[0], w)
    assert st[0]["n_bad_bounds"] == 1 and depth[0][7, 9] == 0 and st[0]["n_optimised"] == plain[2]["n_optimised"] - int(d0[7, 9] > 0)
    w = R.depth_optim(K.ref_rig(rig, p1_03=-rig["p1_03"]), s, d0)
    assert w[2]["n_bad_bounds"] == plain[2]["n_optimised"] and w[2]["n_optimised"] == 0


@gpu
@pytest.mark.parametrize("cam_w,cam_h", [(63, 7), (64, 8), (65, 9)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shapes_astride_the_wave_and_the_tile(cam_w, cam_h, dtype):
    from x_maps_amd.esl_optim import EslOptim
    rig = K.make_rig(cam_w, cam_h, 40, 64, 50 + cam_h)
    s = rig["surface"].astype(dtype)
    w = R.depth_optim(K.ref_rig(rig), s, rig["depth_init"])
    assert w[2]["n_optimised"] > 20 * (cam_h - 6) and (w[1][:, 57:] > 0).any() and (w[1][3] > 0).any() and (w[1][cam_h - 4] > 0).any()
    with EslOptim(K.tables(rig)) as opt:
        depth, nfev, st = run(opt, s, rig["depth_init"])
    same(depth[0], nfev[0], st[0], w)


@gpu
def test_group_beyond_a_grid_dimension():
    """65 538 surfaces of the smallest camera: three launches of at most 65 535; the surfaces cycle through four variants"""
    from x_maps_amd.esl_optim import EslOptim
    rig = K.make_rig(7, 7, 40, 64, 77, lit00=True)
    variants = K.group(rig, np.float32, 5)[[0, 1, 3, 4]]
    d0s = np.zeros((4, 7, 7), np.float32)
    d0s[:, 3, 3] = (60.0, 57.0, 52.5, 66.0)
    d0s[:, 0, 0] = d0s[:, 2, 3] = 55.0  # (inside the border: ignored)
    wants = [R.depth_optim(K.ref_rig(rig), v, d) for v, d in zip(variants, d0s)]
    assert [w[2]["n_optimised"] for w in wants] == [1, 0, 1, 1] and len({float(w[0][3, 3]) for w in wants}) == 4
    n = 65538
    surfaces = np.ascontiguousarray(np.tile(variants, (n // 4 + 1, 1, 1))[:n])
    with EslOptim(K.tables(rig)) as opt:
        depth, nfev, st = run(opt, surfaces, np.tile(d0s, (n // 4 + 1, 1, 1))[:n])
    assert not np.isnan(depth).any()
    for k in range(4):
        assert (depth[k::4].view(np.uint32) == wants[k][0].view(np.uint32)).all() and (nfev[k::4] == wants[k][1]).all()
    assert [st[i] for i in (0, 1, 65534, 65535, 65536, 65537)] == [wants[i % 4][2] for i in (0, 1, 65534, 65535, 65536, 65537)]
    assert sum(s["n_evals"] for s in st) == sum(int(wants[i % 4][2]["n_evals"]) for i in range(n))


@gpu
def test_invalid_configurations_are_refused(small):
    from x_maps_amd import _native as N
    from x_maps_amd.esl_optim import EslOptim
    rig, _ = small
    for kw in (dict(window_size=2), dict(window_size=9), dict(window_size=-1), dict(max_iter=-1), dict(max_iter=65536), dict(xatol=-1e-5),
               dict(xatol=np.inf), dict(p1_03=0.0), dict(p1_03=np.nan), dict(p1_03=np.inf), dict(cam_w=6), dict(cam_h=6),
               dict(window_size=7, cam_h=14), dict(Rt=np.full(12, np.nan))):
        with pytest.raises(ValueError):
            EslOptim(K.tables(rig, **kw))
    with pytest.raises(ValueError):
        EslOptim(K.tables(rig, proj_surface=rig["proj"][:-1]))
    with pytest.raises(ValueError):
        EslOptim(K.tables(rig, cam_D=np.zeros(4)))
    with EslOptim(K.tables(rig, window_size=7, cam_w=15, cam_h=15)):  # (2 * 7 + 1: the smallest camera of the largest window)
        pass
    lib = N.load_library()
    t = K.tables(rig)
    arr = lambda key, n: (C.c_double * n)(*np.asarray(t[key], np.float64).ravel())
    cfg = N.xm_esl_optim_config(C.sizeof(N.xm_esl_optim_config), rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 0, 0, 0, 0.0,
                                rig["p1_03"], arr("cam_K", 9), arr("cam_D", 5), arr("proj_K", 9), arr("proj_D", 5), arr("Rt", 12),
                                rig["proj"].ctypes.data)
    h = C.c_void_p()
    for field, bad in (("struct_size", 8), ("cam_width", 0), ("proj_height", -3), ("proj_surface", None), ("window_size", 4)):
        keep = getattr(cfg, field)
        setattr(cfg, field, bad)
        assert lib.xm_esl_optim_create(0, C.byref(cfg), C.byref(h)) == N.XM_ERR_INVALID and not h.value and N.last_error()
        setattr(cfg, field, keep)
    assert lib.xm_esl_optim_create(0, None, C.byref(h)) == N.XM_ERR_INVALID
    assert lib.xm_esl_optim_create(0, C.byref(cfg), C.byref(h)) == N.XM_OK and h.value
    s = np.ascontiguousarray(rig["surface"].astype(np.float32))
    depth = np.empty(s.shape, np.float32)
    args = (s.ctypes.data, N.XM_T_FLOAT32, 1, N.XM_MEM_HOST, rig["depth_init"].ctypes.data, depth.ctypes.data, None, None)
    for pos, bad in ((1, N.XM_T_INT64), (2, 0), (2, -1), (3, 7), (0, None), (4, None), (5, None)):
        a = list(args)
        a[pos] = bad
        assert lib.xm_esl_optim_time_surfaces(h, *a) == N.XM_ERR_INVALID
    assert lib.xm_esl_optim_time_surfaces(None, *args) == N.XM_ERR_INVALID
    assert lib.xm_esl_optim_time_surfaces(h, *args) == N.XM_OK  # (the object is still good; nfev_out and stats_out are optional)
    lib.xm_esl_optim_destroy(h)
    lib.xm_esl_optim_destroy(None)


@gpu
def test_on_arrival_tool_writes_depth_optim_and_the_table_still_has_no_ground_truth(small, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_esl_on_arrival as T
    finally:
        sys.path.pop(0)
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    from x_maps_amd.esl_optim import build_esl_optim_tables
    from x_maps_amd.eval_table import esl_init_table_row
    rig, _ = small
    cp = CamProjCalibrationParams(rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 3 * rig["proj_w"], 3 * rig["proj_h"], rig["cam_K"],
                                  rig["cam_D"], rig["proj_K"], rig["proj_D"], rig["R"], rig["T"].reshape(3, 1))
    t_init, t_opt = build_esl_init_tables(cp), build_esl_optim_tables(cp)
    surfaces = K.group(rig, np.float64, 5)
    os.makedirs(tmp_path / "scans_np")
    for i, s in enumerate(surfaces):
        np.save(tmp_path / "scans_np" / f"scans{i:03d}.npy", s)
    rep_init, rep = T.esl_optim_from_scans(str(tmp_path), None, 0, 0, init_tables=t_init, optim_tables=t_opt, group=2)
    assert rep["scans_found"] == 5 and rep["scans_processed"] == 4 and rep["scans_empty"] == 1 and rep_init["scans_processed"] == 4
    assert "depth_optim_filtered" in rep["still_needed"] and "bilateral" in rep["still_needed"] and "TV" in rep["still_needed"]
    names = [f"scans{i:03d}.npy" for i in (0, 2, 3, 4)]
    assert sorted(os.listdir(tmp_path / "esl" / "depth_optim")) == names == sorted(os.listdir(tmp_path / "esl" / "depth_init"))
    rr = R.Rig(t_opt["cam_K"], t_opt["cam_D"], t_opt["proj_K"], t_opt["proj_D"], t_opt["Rt"], t_opt["proj_surface"], t_opt["p1_03"])
    with EslInit(t_init) as esl:
        inits = [e[0] for e in esl.depths_from_time_surfaces(surfaces)]
    n_opt = n_ev = 0
    for name in names:
        i = int(name[5:8])
        assert np.array_equal(np.load(tmp_path / "esl" / "depth_init" / name), inits[i])
        w_depth, _, w_st = R.depth_optim(rr, surfaces[i], inits[i])
        got = np.load(tmp_path / "esl" / "depth_optim" / name)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), w_depth.view(np.uint32))
        n_opt, n_ev = n_opt + w_st["n_optimised"], n_ev + w_st["n_evals"]
    assert rep["n_optimised"] == n_opt > 100 and rep["n_evals"] == n_ev and rep["n_hit_limit"] == 0
    row = esl_init_table_row(str(tmp_path))
    assert "no ground truth" in row["error"] and "bilateral" in row["error"] and row["esl_init_files"] == 4


def test_shapes_sit_astride_the_kernels_tiles():
    """CPU: the constants the shapes above were chosen against are the kernel's"""
    geo = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()
    src = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_esloptim.hpp")).read()
    host = open(os.path.join(ROOT, "x_maps_amd", "csrc", "host", "xm_api_esloptim.hpp")).read()
    assert re.search(r"constexpr int BLOCK = 256;", geo)
    assert re.search(r"constexpr int ESLO_FW = 64, ESLO_FR = BLOCK / 64;", src) and re.search(r"constexpr int ESLO_MAX_WS = 7;", src)
    assert re.search(r"constexpr size_t ESLO_GRID_CAP = 65535;", host)
