"""CPU: O.process_time_surface -- the oracle of the time-surface entry (xm_process_time_surfaces) -- against golden G7 (the
reference's own functions on its evaluation caller), its defined results for surfaces without events, the value edges of the
normalisation, and the geometry of the cameras that tests/test_gpu_time_surfaces_oracle.py runs it on."""
import os
import re

import numpy as np
import pytest

import time_surface_cases as K
import xmaps_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g7(golden_dir):
    return np.load(os.path.join(golden_dir, "g7_eval_caller.npz"))


def _g7_tables(g):
    return {"cam_mapx_i16": g["mapx"], "cam_mapy_i16": g["mapy"], "proj_x_map": g["xmap"], "p03": float(g["p03"]),
            "cam_mapx_f32": g["mapx_f32"], "cam_mapy_f32": g["mapy_f32"], "Q": g["Q"]}


def test_golden_g7(g7):
    surf = g7["raw_time_surface"]
    r = O.process_time_surface(_g7_tables(g7), surf)
    assert np.array_equal(r["event_x"], g7["event_x"]) and np.array_equal(r["event_t"], g7["event_t"])
    mask = r["mask"]
    assert np.array_equal(r["xr_f32"], g7["xr_f32"][mask]) and np.array_equal(r["yr_f32"], g7["yr_f32"][mask])
    assert r["xr_f32"].dtype == np.float32 and np.array_equal(r["x"], g7["event_x"][mask])
    depth = r["depth"]
    assert depth.dtype == np.float32 and depth.shape == g7["depth"].shape
    assert np.array_equal(depth == 0, g7["depth"] == 0)
    np.testing.assert_allclose(depth, g7["depth"], rtol=1e-4, atol=0)
    cloud, ref = O.construct_point_cloud(g7["Q"], r["xr_f32"], r["yr_f32"], r["disp"].astype(np.float32)), g7["cloud"]
    assert cloud.shape == ref.shape == (1268, 3)
    fin = np.isfinite(ref)
    assert not fin.all() and np.array_equal(np.isfinite(cloud), fin)  # (rows of disparity 0)
    np.testing.assert_allclose(cloud[fin], ref[fin], rtol=1e-5, atol=1e-6)
    nz = surf[surf != 0]
    assert r["stats"] == {"n_nonzero": nz.size, "n_events": 2007, "n_inliers": 1268, "n_index_errors": 0, "lo": nz.min(),
                          "hi": nz.max(), "t_min": g7["event_t"].min(), "t_max": 1.0}
    # a float32 file is widened before it is normalised
    r32 = O.process_time_surface(_g7_tables(g7), surf.astype(np.float32))
    r64 = O.process_time_surface(_g7_tables(g7), surf.astype(np.float32).astype(np.float64))
    assert np.array_equal(r32["event_t"], r64["event_t"]) and np.array_equal(r32["depth"], r64["depth"]) and r32["stats"] == r64["stats"]


def test_rows_are_the_depth_maps_pixels_in_raster_order(g7):
    tb = _g7_tables(g7)
    r = O.process_time_surface(tb, g7["raw_time_surface"])
    x, y, disp = r["x"], r["y"], r["disp"]
    assert len(x) == len(y) == len(disp) == len(r["xr_f32"]) == r["stats"]["n_inliers"] == int(r["mask"].sum())
    order = y * 64 + x
    assert (np.diff(order) > 0).all()  # raster order, one row per pixel
    frame = np.zeros((48, 64), np.float32)
    frame[y, x] = disp
    assert np.array_equal(r["depth"], O.disparity_to_depth_rectified(frame, tb["p03"]))
    assert np.array_equal(r["xr_f32"], tb["cam_mapx_f32"][y, x]) and np.array_equal(r["yr_f32"], tb["cam_mapy_f32"][y, x])


def _hand_tables():
    """a 6 x 4 camera whose every pixel is an inlier at every time column"""
    ys, xs = np.mgrid[0:4, 0:6]
    return {"cam_mapx_i16": (xs + 1).astype(np.int16), "cam_mapy_i16": (ys + 1).astype(np.int16),
            "proj_x_map": (O.X_OFFSET + 10 + np.arange(8)[None, :] + np.zeros((7, 1))).astype(np.int16), "p03": 30.0}


def test_surfaces_without_events_have_defined_results():
    tb = _hand_tables()
    one = np.zeros((4, 6))
    one[1, 2] = one[3, 5] = 7.5  # one distinct non-zero value, twice
    for surf, nnz, v in ((np.zeros((4, 6)), 0, 0.0), (np.zeros((4, 6), np.float32), 0, 0.0), (one, 2, 7.5)):
        r = O.process_time_surface(tb, surf)
        assert r["depth"].shape == (4, 6) and r["depth"].dtype == np.float32 and not r["depth"].any()
        assert len(r["x"]) == len(r["y"]) == len(r["disp"]) == 0 and r["xr_f32"] is None
        assert r["stats"] == {"n_nonzero": nnz, "n_events": 0, "n_inliers": 0, "n_index_errors": 0, "lo": v, "hi": v,
                              "t_min": 0.0, "t_max": 0.0}
    with pytest.raises(ValueError):
        O.process_time_surface(tb, np.zeros((6, 4)))


def test_negative_lo_makes_zeros_events():
    tb = _hand_tables()
    surf = np.zeros((4, 6))
    surf[0, 0], surf[1, 1], surf[2, 2] = -2.0, 2.0, 1.0
    r = O.process_time_surface(tb, surf)
    st = r["stats"]
    assert (st["n_nonzero"], st["n_events"], st["lo"], st["hi"]) == (3, 23, -2.0, 2.0)  # every pixel but lo's
    assert st["t_min"] == 0.5 and st["t_max"] == 1.0 and st["n_inliers"] == 23
    assert (r["depth"] != 0).sum() == 23 and r["depth"][0, 0] == 0
    # a zero has t = 0.5: column rint(0 / 0.5 * 7) = 0; (2, 2) has t = 0.75: column rint(0.5 * 7) = 4 (half to even)
    assert (r["y"][0], r["x"][0], r["disp"][0]) == (0, 1, 10 + 0 - 2) and r["disp"][list(zip(r["y"], r["x"])).index((2, 2))] == 10 + 4 - 3


def test_two_values_give_one_time_stamp():
    tb = _hand_tables()
    surf = np.zeros((4, 6), np.float32)
    surf[0, 1] = surf[2, 3] = surf[3, 5] = 2.0
    surf[1, 1] = 1.0
    r = O.process_time_surface(tb, surf)
    st = r["stats"]
    assert (st["n_nonzero"], st["n_events"], st["n_inliers"]) == (4, 3, 3) and st["t_min"] == st["t_max"] == 1.0
    assert np.array_equal(r["event_t"], [1.0, 1.0, 1.0])
    assert list(zip(r["y"], r["x"])) == [(0, 1), (2, 3), (3, 5)]
    assert np.array_equal(r["disp"], 10 + 0 - np.array([2, 4, 6]))  # t_min == t_max: every event in column 0


def test_negative_zero_is_no_event():
    tb = _hand_tables()
    surf = np.zeros((4, 6))
    surf[0, 0], surf[0, 1], surf[3, 5] = 1.0, 3.0, 2.0
    ref = O.process_time_surface(tb, surf)
    surf[1, 1] = surf[3, 4] = -0.0
    assert np.signbit(surf).sum() == 2
    r = O.process_time_surface(tb, surf)
    assert r["stats"] == ref["stats"] and r["stats"]["n_nonzero"] == 3 and r["stats"]["n_events"] == 2
    assert np.array_equal(r["depth"], ref["depth"]) and r["depth"][1, 1] == 0 and r["depth"][3, 4] == 0
    # ... but with lo < 0 it is an event like any other zero
    surf[0, 0] = -1.0
    r = O.process_time_surface(tb, surf)
    assert r["stats"]["n_events"] == 23 and r["depth"][1, 1] == np.float32(30.0 / (10 + 0 - 2))
    assert r["event_t"][list(zip(r["event_y"], r["event_x"])).index((1, 1))] == 0.25


def test_differential_cameras_cross_the_loop_bounds():
    """the constants time_surface_cases.geometry() restates, and what each camera of the GPU tests is for"""
    src = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_surface.hpp")).read()
    kern = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()  # (BLOCK: shared with the host's plan)

    def const(name, text=src):
        return int(re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*" + name + r"\s*=\s*(\d+)", text).group(1))
    block = const("BLOCK", kern)
    assert block * const("SURF_RED_ITEMS") == K.RED_CHUNK and (const("SURF_TW"), const("SURF_TR")) == (K.TILE_W, K.TILE_ROWS)
    assert block // 64 == K.WAVES_PER_BLOCK and const("SURF_SCAN_BLOCK") == K.SCAN_BLOCK
    geo = {name: K.geometry(*wh) for name, wh in K.CAMERAS.items()}
    assert geo == {"tall": (66, 2, 129, 4098, 5, 1032), "wide": (34, 33, 3, 1089, 2, 396), "on_bound": (32, 1, 64, 1024, 1, 256),
                   "past_bound": (33, 1, 65, 1025, 2, 260)}
    nb_red, _, _, n_seg, ipt, n_wo = geo["tall"]
    assert nb_red > 64 and n_seg > K.SCAN_BLOCK and n_wo > K.SCAN_BLOCK  # the second trip of all three loops
    assert (n_seg - 1) // ipt == 819 and n_seg % ipt != 0  # thread 819 has a partial run, the threads behind it none
    assert 65 % K.TILE_W == 1 and 2049 % K.TILE_ROWS == 1  # a 1-pixel last tile column, a 1-row last tile
    _, tiles_x, _, n_seg, ipt, _ = geo["wide"]
    assert tiles_x % 2 == 1 and ipt == 2 and (n_seg - 1) // ipt == 544 and n_seg % ipt != 0
    assert 64 * 1024 % K.RED_CHUNK == 0 and 64 % K.TILE_W == 0 and 1024 % K.TILE_ROWS == 0  # on_bound: no padding anywhere
