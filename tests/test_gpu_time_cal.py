"""GPU: the projector time-map calibration (csrc/xmaps_timecal.hpp, xm_timecal_* of include/xmaps.h,
x_maps_amd/time_map_calibration.py) against the NumPy oracle of tests/time_cal_cases.py, bit for bit, on the cases
tests/test_time_cal_cases_cpu.py shows to reach every loop bound.  The arithmetic is this build's definition.

The corner verdict "not strictly convex" cannot be reached by detected corners (test_time_cal_cases_cpu.py shows why: whenever
detection fails the verdict, two corners coincide); it is held here where a caller can reach it, through corners of their own."""
import ctypes as C

import numpy as np
import pytest

import time_cal_cases as T
from x_maps_amd import _native as N
from x_maps_amd import time_map_calibration as TMC

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _check_solution(cal, st, got_map, got_present, want):
    assert (st.n_valid, st.n_core) == (want["n_valid"], want["n_core"])
    assert (None if st.corners is None else list(st.corners)) == want["corners"]
    assert _same(got_present, want["present"])
    assert _same(got_map[want["present"]], want["value"][want["present"]].astype(np.float32))  # the map before the fill
    assert _same(got_map, want["time_map"])
    assert (st.n_missing, st.n_unfilled) == (want["n_missing"], want["n_unfilled"])


# ---- accumulate -> mean -> corners -> warp -> fill -----------------------------------------------------------------------
@pytest.mark.parametrize("name,sizes,min_count", [("n1", None, 1), ("n3", None, 2), ("n9", "one", 5), ("n9", "4+5", 5), ("n9", "nine", 5),
                                                  ("n9_f32", "4+5", 5), ("small", None, 2), ("skipped", None, 2), ("persp", None, 1)])
def test_chain_is_the_oracles(name, sizes, min_count):
    s = T.surfaces(name)
    want = T.solved(name, min_count, T.PROJ)
    o = T.accumulated(name)
    with TMC.TimeMapCalibrator((s.shape[2], s.shape[1])) as cal:
        for rounds in range(2):  # reset, then the same adds: the same bits
            k = 0
            for n in T.GROUPINGS[sizes] if sizes else (len(s),):
                cal.add_surfaces(s[k:k + n])
                k += n
            assert (cal.stats.n_added, cal.stats.n_skipped) == (o.n_added, o.n_skipped)
            share = min_count / o.n_used
            assert T.min_count_for(share, o.n_used) == min_count
            mean, valid, st = cal.mean(share, want_arrays=True)
            assert st.min_count == min_count
            assert _same(mean, want["mean"]) and _same(valid, want["valid"])  # (sum and cnt, through them)
            h = T.proj_to_cam(T.PROJ, want["corners"])
            got_map, got_present = cal.warp(h, T.PROJ, want_present=True)
            _check_solution(cal, cal.stats, got_map, got_present, want)
            solved_map, _ = cal.solve(T.PROJ)  # the product's own host solve
            assert _same(solved_map, want["time_map"]) and _same(cal.stats.h, want["h"])
            cal.reset()
            assert cal.stats.n_added == 0


def test_min_count_edges():
    o = T.accumulated("n9")
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        cal.add_surfaces(T.surfaces("n9"))
        for mc in (4, 5, 9):
            mean, valid, st = cal.mean(mc / 9.0, want_arrays=True, need_corners=False)
            wm, wv = o.mean(mc)
            assert (st.n_valid, st.n_core) == T.find_corners(wv, check=False)[:2] and (st.corner_error is None) == (mc < 9)
            assert _same(mean, wm) and _same(valid, wv)
            assert valid[o.cnt == mc].all() and not valid[o.cnt == mc - 1].any()


@pytest.mark.parametrize("size", T.PROJ_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("corners,min_count", [(None, 5), (T.QUAD_WIDE, T.WIDE_MIN_COUNT)], ids=["detected", "wide"])
def test_projector_sizes_and_missing_runs(size, corners, min_count):
    want = T.solved("n9", min_count, size, corners)
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        cal.add_surfaces(T.surfaces("n9"))
        cal.mean(min_count / 9.0, need_corners=corners is None)  # (at the wide case's min_count the mask has holes and no core pixel)
        got_map, got_present = cal.warp(want["h"], size, want_present=True)
        _check_solution(cal, cal.stats, got_map, got_present, want)
        solved_map, st = cal.solve(size, corners=corners)
        assert _same(solved_map, want["time_map"])


@pytest.mark.parametrize("order", range(8))
def test_corner_orders(order):
    want = T.solved("persp", 1, T.PROJ, None, order)
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        cal.add_surfaces(T.surfaces("persp"))
        cal.mean(0.5)
        got, _ = cal.solve(T.PROJ, corner_order=order)
        assert _same(got, want["time_map"])


# ---- the device-memory entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n9", "n9_f32"])
def test_device_pointers(name):
    import torch
    s = T.surfaces(name)
    want = T.solved(name, 5, (300, 5), T.QUAD_WIDE)
    lib = N.load_library()
    W, H = 300, 5
    tc = C.c_void_p()
    N.check(lib.xm_timecal_create(0, T.CAM[0], T.CAM[1], C.byref(tc)))
    try:
        d_in = torch.from_numpy(np.array(s)).cuda()
        dt = N.XM_T_FLOAT32 if s.dtype == np.float32 else N.XM_T_FLOAT64
        N.check(lib.xm_timecal_add_surfaces(tc, C.c_void_p(d_in[:4].data_ptr()), dt, 4, N.XM_MEM_DEVICE))
        N.check(lib.xm_timecal_add_surfaces(tc, C.c_void_p(d_in[4:].data_ptr()), dt, 5, N.XM_MEM_DEVICE))
        d_mean = torch.empty((T.CAM[1], T.CAM[0]), dtype=torch.float64, device="cuda")
        d_valid = torch.empty((T.CAM[1], T.CAM[0]), dtype=torch.uint8, device="cuda")
        st = N.xm_timecal_stats()
        torch.cuda.synchronize()
        N.check(lib.xm_timecal_mean(tc, 5, C.c_void_p(d_mean.data_ptr()), C.c_void_p(d_valid.data_ptr()), N.XM_MEM_DEVICE, C.byref(st)))
        assert _same(d_mean.cpu().numpy(), want["mean"]) and _same(d_valid.cpu().numpy().astype(bool), want["valid"])
        assert (st.n_added, st.n_skipped, st.n_valid, st.n_core) == (9, 0, want["n_valid"], want["n_core"])
        assert [(st.corners[k][0], st.corners[k][1]) for k in range(4)] == want["corners"]
        d_map = torch.empty((H, W), dtype=torch.float32, device="cuda")
        d_present = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h = (C.c_double * 9)(*want["h"])
        N.check(lib.xm_timecal_warp(tc, h, W, H, C.c_void_p(d_map.data_ptr()), C.c_void_p(d_present.data_ptr()), N.XM_MEM_DEVICE,
                                    C.byref(st)))
        assert _same(d_map.cpu().numpy(), want["time_map"]) and _same(d_present.cpu().numpy().astype(bool), want["present"])
        assert (st.n_missing, st.n_unfilled) == (want["n_missing"], want["n_unfilled"])
        # present_out is optional
        N.check(lib.xm_timecal_warp(tc, h, W, H, C.c_void_p(d_map.data_ptr()), None, N.XM_MEM_DEVICE, None))
        assert _same(d_map.cpu().numpy(), want["time_map"])
    finally:
        lib.xm_timecal_destroy(tc)


# ---- corners on hand-built masks --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rectangle", "diamond"])
def test_corner_ties(name):
    valid, _ = T.corner_masks()[name]
    n_valid, n_core, corners = T.find_corners(valid)
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        st = cal.set_mean(np.where(valid, 0.5, 0.0), valid)
        assert (st.n_valid, st.n_core, list(st.corners)) == (n_valid, n_core, corners)


@pytest.mark.parametrize("name,word", [("two_wide", "no core pixel"), ("blob3", "coincide")])
def test_corner_errors(name, word):
    valid, _ = T.corner_masks()[name]
    lib = N.load_library()
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        m = np.ascontiguousarray(np.where(valid, 0.5, 0.0))
        v = np.ascontiguousarray(valid.astype(np.uint8))
        st = N.xm_timecal_stats()
        rc = lib.xm_timecal_set_mean(cal._tc, C.c_void_p(m.ctypes.data), C.c_void_p(v.ctypes.data), N.XM_MEM_HOST, C.byref(st))
        assert rc == N.XM_ERR_INVALID and word in N.last_error()
        assert st.n_valid == int(valid.sum()) and st.n_core == int(T.core_mask(valid).sum())
        with pytest.raises(ValueError, match=word):
            cal.set_mean(m, valid)
        # the same through the accumulators: surfaces that are seen on the mask only
        cal.reset()
        s = np.where(valid, 1.0 + np.arange(valid.size, dtype=np.float64).reshape(valid.shape), 0.0)
        cal.add_surfaces(s[None])
        rc = lib.xm_timecal_mean(cal._tc, 1, None, None, N.XM_MEM_HOST, C.byref(st))
        assert rc == N.XM_ERR_INVALID and word in N.last_error() and st.n_valid == int(valid.sum())
        # the state stays: corners of the caller's own go on
        got, _ = cal.solve(T.PROJ, corners=((15, 3), (26, 3), (26, 42), (15, 42)))
        assert got.shape == (T.PROJ[1], T.PROJ[0])


def test_non_convex_corners_are_refused():
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        cal.add_surfaces(T.surfaces("persp"))
        cal.mean(0.5)
        with pytest.raises(ValueError, match="strictly convex"):
            cal.solve(T.PROJ, corners=T.NON_CONVEX)
        with pytest.raises(ValueError, match="coincide"):
            cal.solve(T.PROJ, corners=((1, 1), (1, 1), (9, 9), (1, 9)))


def test_argument_errors():
    lib = N.load_library()
    tc = C.c_void_p()
    assert lib.xm_timecal_create(0, 0, 5, C.byref(tc)) == N.XM_ERR_INVALID
    with TMC.TimeMapCalibrator(T.CAM_SMALL) as cal:
        h = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
        out = np.empty((4, 5), np.float32)
        assert lib.xm_timecal_warp(cal._tc, h, 5, 4, C.c_void_p(out.ctypes.data), None, N.XM_MEM_HOST, None) == N.XM_ERR_INVALID
        assert "no mean" in N.last_error()
        assert lib.xm_timecal_mean(cal._tc, 0, None, None, N.XM_MEM_HOST, None) == N.XM_ERR_INVALID
        assert lib.xm_timecal_add_surfaces(cal._tc, C.c_void_p(out.ctypes.data), N.XM_T_INT64, 1, N.XM_MEM_HOST) == N.XM_ERR_INVALID
        with pytest.raises(ValueError):
            cal.add_surfaces(np.zeros((2, 3, 3), np.float32))


# ---- the warp as a stage: an oracle-made mean and an arbitrary h ------------------------------------------------------------
def test_warp_on_an_oracle_mean_with_an_arbitrary_h():
    base = T.solved("n9", 5, T.PROJ)
    value, present = T.warp(base["mean"], base["valid"], T.ARBITRARY_H, T.PROJ)
    want_map, n_missing, n_unfilled = T.fill(value, present)
    with TMC.TimeMapCalibrator(T.CAM) as cal:
        cal.set_mean(base["mean"], base["valid"])
        got, got_present = cal.warp(T.ARBITRARY_H, T.PROJ, want_present=True)
        assert _same(got_present, present) and _same(got, want_map)
        assert (cal.stats.n_missing, cal.stats.n_unfilled) == (n_missing, n_unfilled)


@pytest.mark.parametrize("name", list(T.WARP_PROBES))
def test_warp_positions(name):
    mean, valid = T.warp_probe()
    h = T.WARP_PROBES[name]
    value, present = T.warp(mean, valid, h, T.WARP_PROBE_SIZE)
    want_map, n_missing, n_unfilled = T.fill(value, present)
    with TMC.TimeMapCalibrator(T.CAM_SMALL) as cal:
        cal.set_mean(mean, valid)
        got, got_present = cal.warp(h, T.WARP_PROBE_SIZE, want_present=True)
        assert _same(got_present, present)
        assert _same(got[present], value[present].astype(np.float32)) and _same(got, want_map)
        assert (cal.stats.n_missing, cal.stats.n_unfilled) == (n_missing, n_unfilled)


# ---- the fill on hand-built rows --------------------------------------------------------------------------------------------
def test_fill_rows():
    """the rows of T.fill_rows() as a warp's result: a 300 x 6 camera image under the identity, valid = present"""
    names, value, present = T.fill_rows()
    H, W = value.shape
    want_map, n_missing, n_unfilled = T.fill(value, present)
    ident = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    v2, p2 = T.warp(value, present, ident, (W, H))
    assert np.array_equal(p2, present) and _same(v2, value)  # on pixel centres the warp hands the rows through
    with TMC.TimeMapCalibrator((W, H)) as cal:
        try:
            cal.set_mean(value, present)
        except ValueError:
            pass  # (whatever the corners of this mask are: the state stays)
        got, got_present = cal.warp(ident, (W, H), want_present=True)
        assert _same(got_present, present) and _same(got, want_map)
        assert (cal.stats.n_missing, cal.stats.n_unfilled) == (n_missing, n_unfilled) and n_unfilled == 1
