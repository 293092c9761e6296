"""-m gpu: the two filters behind ESL's depth optimisation on the device (xm_esl_filter_*, csrc/xmaps_eslfilter.hpp) against the CPU
restatement tests/esl_filter_ref.py.  Stage 1 (float32, one fixed operation order) is compared bit for bit.  Stage 2's trip counts
and integer statistics are compared exactly; its values are bounded: the device sums every norm in tile order, NumPy's BLAS in
another, so |gpu - ref| <= max(1000 x D, 1e-12) where D is the CPU difference between the restatement with np.linalg.norm and with
exactly rounded (math.fsum) norms on that very input -- computed here, never taken from the device.  Outputs are pre-filled with NaN
/ 0xFF, so an unwritten element shows.

Shapes (H x W): 20 x 24 is below one TV tile of 1024 pixels, 24 x 20 its transpose (the differences' stride is H: the reference's
swapped dims); 48 x 40 is two tiles, the second ragged, and 96 x 80 seven and a half, with stride-H neighbours across tile edges;
9 x 33 is one more than the bilateral tile of 32 x 8 in either direction.  Groups mix a zero map (lsqr returns x = 0; 1 outer
iteration), a constant map (2), a ramp that ends through tol, and full-length scenes, so stopped surfaces sit beside running ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import esl_filter_cases as K
import esl_filter_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref(img, no_bilateral=False, **kw):
    """the restatement on one map, computed once: (filtered, bilateral, info, bound, the CPU difference)"""
    key = (img.shape, img.tobytes(), no_bilateral, tuple(sorted(kw.items())))
    if key not in _REF:
        out, bil, info = R.esl_filter(img, no_bilateral=no_bilateral, **kw)
        out_fsum, _, info_fsum = R.esl_filter(img, no_bilateral=no_bilateral, norm=R.norm_fsum, **kw)
        assert np.array_equal(info["trips"], info_fsum["trips"])
        d = float(np.abs(out - out_fsum).max())
        _REF[key] = (out, bil, info, max(1000.0 * d, 1e-12), d)
    return _REF[key]


def run(flt, maps, want_bil=True):
    """xm_esl_filter_maps on host memory with pre-filled outputs -> (filtered, bilateral, trips, [stats])"""
    from x_maps_amd import _native as N
    grp = np.ascontiguousarray(maps if maps.ndim == 3 else maps[None], np.float32)
    n = len(grp)
    out = np.full(grp.shape, np.nan, np.float64)
    bil = np.full(grp.shape, np.nan, np.float32) if want_bil else None
    trips = np.full((n, flt.n_calls), 0xFF, np.uint8)
    st = (N.xm_esl_filter_stats * n)()
    N.check(flt._lib.xm_esl_filter_maps(flt._h, grp.ctypes.data, n, N.XM_MEM_HOST, out.ctypes.data, bil.ctypes.data if want_bil else None,
                                        trips.ctypes.data, C.cast(st, C.c_void_p)))
    return out, bil, trips, list(st)


def check_map(name, img, out, bil, trips, st, no_bilateral=False):
    w_out, w_bil, info, bound, d = ref(img, no_bilateral)
    diff = float(np.abs(out - w_out).max())
    print(f"{name}: max |gpu - ref| = {diff:.3e}, CPU numpy-vs-fsum = {d:.3e}, bound = {bound:.3e}, outer {st.n_outer}, lsqr {st.n_lsqr}, "
          f"itn {st.sum_itn}, istop {list(st.istop_count)}, final norm {st.final_norm:.6e} (ref {info['final_norm']:.6e})")
    assert not np.isnan(out).any()  # (every pixel was written)
    if not no_bilateral:
        assert np.array_equal(bil.view(np.uint32), w_bil.view(np.uint32))
    assert np.array_equal(trips, info["trips"])
    assert (st.n_outer, st.n_lsqr, st.sum_itn) == (info["n_outer"], info["n_lsqr"], info["sum_itn"])
    assert list(st.istop_count) == list(info["istop_count"])
    assert st.lo == float(img.min()) and st.hi == float(img.max())
    assert diff <= bound
    # | ||a|| - ||b|| | <= ||a - b||, and x and xold each lie within the bound of the restatement's
    assert abs(st.final_norm - info["final_norm"]) <= 2.0 * np.sqrt(img.size) * bound + 1e-12 * info["final_norm"]
    return diff


@gpu
@pytest.mark.parametrize("H,W,n", [(20, 24, 1), (20, 24, 5), (24, 20, 3), (48, 40, 5), (96, 80, 3), (9, 33, 1)])
def test_groups_against_the_restatement(H, W, n):
    from x_maps_amd.esl_filter import EslFilter
    maps = K.group(H, W, n)
    with EslFilter(W, H) as flt:
        out, bil, trips, st = run(flt, maps)
        assert flt.last_launches() == 3 + 200 * 14 + 1
    for i in range(n):
        check_map(f"{H}x{W} map {i} of {n}", maps[i], out[i], bil[i], trips[i], st[i])
    if n >= 3:
        assert st[1].n_outer == 1 and st[1].istop_count[0] == 10 and not out[1].any()  # the zero map
        assert st[2].n_outer == 2 and (trips[2][20:] == 0xFF).all()                    # the constant map
        assert np.array_equal(bil[2], maps[2])                                         # ... which stage 1 copies
    if n >= 5:
        assert 2 < st[3].n_outer < 20 and st[0].n_outer > st[3].n_outer                 # the ramp ends through tol


@gpu
def test_each_stage_alone():
    from x_maps_amd.esl_filter import EslFilter, NO_BILATERAL, NO_TV
    maps = K.group(48, 40, 5)
    with EslFilter(40, 48, flags=NO_TV) as flt:
        out, bil, trips, st = run(flt, maps)
    for i in range(5):
        w_bil = R.bilateral(maps[i])
        assert np.array_equal(bil[i].view(np.uint32), w_bil.view(np.uint32)) and np.array_equal(out[i], w_bil.astype(np.float64))
        assert (trips[i] == 0xFF).all() and st[i].n_outer == 0 and st[i].lo == float(maps[i].min()) and st[i].hi == float(maps[i].max())
    with EslFilter(40, 48, flags=NO_BILATERAL) as flt:
        out, _, trips, st = run(flt, maps[:2], want_bil=False)
    for i in range(2):
        check_map(f"TV alone, map {i}", maps[i], out[i], None, trips[i], st[i], no_bilateral=True)


@gpu
def test_bilateral_edges_bit_for_bit():
    """the border on maps smaller than the halo, the idx + 1 reach at |v - v0| = len, and a map of two values"""
    from x_maps_amd.esl_filter import EslFilter, NO_TV
    rng = np.random.default_rng(160)
    for H, W in ((1, 1), (1, 7), (2, 3), (3, 2), (8, 32), (9, 33), (17, 65)):
        m = (50.0 + 20.0 * rng.random((H, W))).astype(np.float32)
        if m.size > 1:
            m.flat[0], m.flat[1] = 20.0, 120.0  # the extrema side by side: a = 4096 exactly
        with EslFilter(W, H, flags=NO_TV) as flt:
            _, bil, _, _ = run(flt, m)
        assert np.array_equal(bil[0].view(np.uint32), R.bilateral(m).view(np.uint32)), (H, W)


@gpu
def test_a_map_alone_equals_itself_inside_a_group():
    from x_maps_amd.esl_filter import EslFilter
    maps = K.group(48, 40, 5)
    with EslFilter(40, 48) as flt:
        out, bil, trips, st = run(flt, maps)
        for i in (0, 3):
            o1, b1, t1, s1 = run(flt, maps[i])
            assert np.array_equal(o1[0].view(np.uint64), out[i].view(np.uint64)) and np.array_equal(b1[0].view(np.uint32), bil[i].view(np.uint32))
            assert np.array_equal(t1[0], trips[i]) and bytes(s1[0]) == bytes(st[i])
        o2, _, t2, _ = run(flt, maps[::-1].copy())  # other neighbours, another place in the group
        assert np.array_equal(o2[::-1].view(np.uint64), out.view(np.uint64)) and np.array_equal(t2[::-1], trips)


@gpu
def test_other_parameters_and_nan_input():
    from x_maps_amd.esl_filter import EslFilter
    img = K.scene(20, 24, 170)
    with EslFilter(24, 20, niter_outer=3, niter_inner=2, iter_lim=3, mu=0.3, lambda0=0.2, tol=1e-3, damp=1e-3) as flt:
        out, bil, trips, st = run(flt, img)
        assert flt.last_launches() == 3 + 6 * 10 + 1
    w, _, info, bound, _ = ref(img, mu=0.3, lambdas=(0.2, 0.1), niter_outer=3, niter_inner=2, iter_lim=3, tol=1e-3, damp=1e-3)
    assert np.array_equal(trips[0], info["trips"]) and st[0].n_outer == info["n_outer"] and np.abs(out[0] - w).max() <= bound
    bad = img.copy()
    bad[3, 4], bad[10, 10] = np.nan, np.inf  # out of contract: the call returns, and nothing is asserted about the values
    with EslFilter(24, 20) as flt:
        run(flt, bad)
        out2, _, _, _ = run(flt, img)  # (the object is still good)
    assert not np.isnan(out2).any()


@gpu
def test_c_abi_errors():
    from x_maps_amd import _native as N
    lib = N.load_library()
    cfg = N.xm_esl_filter_config(C.sizeof(N.xm_esl_filter_config), 24, 20)
    h = C.c_void_p()
    for field, value in (("struct_size", 8), ("width", 0), ("height", -1), ("flags", 3), ("flags", 4), ("d", 4), ("niter_outer", 256),
                         ("iter_lim", 255), ("mu", -1.0), ("tol", float("nan"))):
        old = getattr(cfg, field)
        setattr(cfg, field, value)
        assert lib.xm_esl_filter_create(0, C.byref(cfg), C.byref(h)) == N.XM_ERR_INVALID and not h.value and N.last_error(), field
        setattr(cfg, field, old)
    assert lib.xm_esl_filter_create(0, C.byref(cfg), C.byref(h)) == N.XM_OK and h.value
    img = K.scene(20, 24, 171)
    out = np.empty(img.shape, np.float64)
    assert lib.xm_esl_filter_maps(h, img.ctypes.data, 0, N.XM_MEM_HOST, out.ctypes.data, None, None, None) == N.XM_ERR_INVALID
    assert lib.xm_esl_filter_maps(h, img.ctypes.data, 65536, N.XM_MEM_HOST, out.ctypes.data, None, None, None) == N.XM_ERR_TOO_MANY
    assert lib.xm_esl_filter_maps(h, img.ctypes.data, 1, 7, out.ctypes.data, None, None, None) == N.XM_ERR_INVALID
    assert lib.xm_esl_filter_maps(h, None, 1, N.XM_MEM_HOST, out.ctypes.data, None, None, None) == N.XM_ERR_INVALID
    assert lib.xm_esl_filter_maps(None, img.ctypes.data, 1, N.XM_MEM_HOST, out.ctypes.data, None, None, None) == N.XM_ERR_INVALID
    assert lib.xm_esl_filter_maps(h, img.ctypes.data, 1, N.XM_MEM_HOST, out.ctypes.data, None, None, None) == N.XM_OK  # (all optional)
    assert np.abs(out - ref(img)[0]).max() <= ref(img)[3]
    lib.xm_esl_filter_destroy(h)
    lib.xm_esl_filter_destroy(None)


def _g13_chain(golden_dir):
    import esl_optim_cases as KO
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.esl_init import build_esl_init_tables
    from x_maps_amd.esl_optim import build_esl_optim_tables
    rig = KO.load_g13(golden_dir)["a"]
    cp = CamProjCalibrationParams(rig["cam_w"], rig["cam_h"], rig["proj_w"], rig["proj_h"], 3 * rig["proj_w"], 3 * rig["proj_h"], rig["cam_K"],
                                  rig["cam_D"], rig["proj_K"], rig["proj_D"], rig["R"], rig["T"].reshape(3, 1))
    return rig, KO, build_esl_init_tables(cp), build_esl_optim_tables(cp)


@gpu
def test_chained_on_the_device_behind_esl_optim(golden_dir):
    """XM_MEM_DEVICE: depth_optim is the buffer xm_esl_optim_time_surfaces has just filled (a G13 rig)"""
    import torch
    from x_maps_amd.esl_filter import EslFilter
    from x_maps_amd.esl_optim import EslOptim
    rig, KO, _, _ = _g13_chain(golden_dir)
    surfaces = KO.group(rig, np.float64, 3)
    d0 = np.ascontiguousarray(np.broadcast_to(rig["depth_init"], surfaces.shape), dtype=np.float32)
    with EslOptim(KO.tables(rig)) as opt, EslFilter(rig["cam_w"], rig["cam_h"]) as flt:
        d_in, d_init = torch.from_numpy(surfaces).cuda(), torch.from_numpy(d0).cuda()
        d_optim = torch.full(surfaces.shape, float("nan"), dtype=torch.float32, device="cuda")
        d_out = torch.full(surfaces.shape, float("nan"), dtype=torch.float64, device="cuda")
        d_bil = torch.full(surfaces.shape, float("nan"), dtype=torch.float32, device="cuda")
        d_trips = torch.full((3, flt.n_calls), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt.time_surfaces_device(d_in.data_ptr(), np.float64, 3, d_init.data_ptr(), d_optim.data_ptr())
        flt.maps_device(d_optim.data_ptr(), 3, d_out.data_ptr(), d_bil.data_ptr(), d_trips.data_ptr())
        optim, out, bil, trips = d_optim.cpu().numpy(), d_out.cpu().numpy(), d_bil.cpu().numpy(), d_trips.cpu().numpy()
        host = flt.filter_maps(optim, want_bilateral=True, want_trips=True)
    assert np.array_equal(optim[0].view(np.uint32), rig["depth_optim"].view(np.uint32))  # (G13's own output went in)
    for i in range(3):
        w_out, w_bil, info, bound, _ = ref(optim[i])
        assert np.array_equal(bil[i].view(np.uint32), w_bil.view(np.uint32)) and np.array_equal(trips[i], info["trips"])
        assert np.abs(out[i] - w_out).max() <= bound
        assert np.array_equal(out[i].view(np.uint64), host[i][0].view(np.uint64)) and np.array_equal(trips[i], host[i][2])


@gpu
def test_on_arrival_tool_writes_the_ground_truth_and_the_table_rows_compute(golden_dir, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_esl_on_arrival as T
    finally:
        sys.path.pop(0)
    from x_maps_amd.eval_table import esl_init_table_row, x_maps_table_row
    rig, KO, t_init, t_opt = _g13_chain(golden_dir)
    surfaces = KO.group(rig, np.float64, 5)[[0, 1, 3, 4]]  # (its own, an all-zero one -- skipped -- and two reseeded ones)
    os.makedirs(tmp_path / "scans_np")
    os.makedirs(tmp_path / "x_maps" / "depth_init")
    for i, s in enumerate(surfaces):
        np.save(tmp_path / "scans_np" / f"scans{i:03d}.npy", s)
    before = x_maps_table_row(str(tmp_path), min_depth=1, max_depth=500)
    assert "no ground truth" in before["error"]
    rep_init, rep, rep_f = T.esl_optim_from_scans(str(tmp_path), None, 0, 0, init_tables=t_init, optim_tables=t_opt, group=2, esl_filter=True)
    names = [f"scans{i:03d}.npy" for i in (0, 2, 3)]
    assert sorted(os.listdir(tmp_path / "esl" / "depth_optim_filtered")) == names == sorted(os.listdir(tmp_path / "esl" / "depth_optim"))
    assert rep_f["scans_processed"] == 3 and rep_f["scans_empty"] == 1 and rep_f["mean_outer_iterations"] >= 1
    for name in names:
        optim, got = np.load(tmp_path / "esl" / "depth_optim" / name), np.load(tmp_path / "esl" / "depth_optim_filtered" / name)
        w_out, _, _, bound, _ = ref(optim)
        assert got.dtype == np.float64 and got.shape == optim.shape and np.abs(got - w_out).max() <= bound
        np.save(tmp_path / "x_maps" / "depth_init" / name, np.load(tmp_path / "esl" / "depth_init" / name))  # an estimate to score
    for row in (x_maps_table_row(str(tmp_path), min_depth=1, max_depth=500), esl_init_table_row(str(tmp_path), min_depth=1, max_depth=500)):
        assert "error" not in row and row["scans"] == 3 and np.isfinite(row["fill_rate"]) and "table_cell" in row, row


def test_shapes_sit_astride_the_kernels_tiles():
    """CPU: the constants the shapes above were chosen against are the kernels'"""
    geo = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()
    assert re.search(r"constexpr int BLOCK = 256;", geo)
    assert re.search(r"constexpr int ESLF_BW = 32, ESLF_BH = BLOCK / ESLF_BW, ESLF_HALO = 2, ESLF_MAX_TAPS = 25, ESLF_BINS = 4096;", geo)
    assert re.search(r"constexpr int ESLF_RED_CHUNK = BLOCK \* 8, ESLF_TILE = BLOCK \* 4;", geo)
