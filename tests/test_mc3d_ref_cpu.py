"""CPU: the NumPy restatement of MC3D (tests/mc3d_ref.py) against the reference's own outputs (golden G12, written by
tests/golden/make_golden_mc3d.py from python/eval/mc3d_baseline.py), array for array; x_maps_amd.mc3d.mc3d_int_maps against the
truncation, poison and saturation cases; the median against eval_table.median_blur3; build_mc3d_tables for shapes, finiteness
inside the frame and p1_03 (its maps' values are unpinned against cv2)."""
import os

import numpy as np
import pytest

import mc3d_cases as K
import mc3d_ref as R


@pytest.fixture(scope="module")
def rigs(golden_dir):
    return K.load_rigs(golden_dir, R.int_maps)


@pytest.mark.parametrize("name", K.RIGS)
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_search_equals_the_reference(rigs, name, dtype):
    rig = rigs[name]
    surf, want = rig[f"surf_{dtype}"], rig[f"disp_{dtype}"]
    assert surf.dtype == (np.float32 if dtype == "f32" else np.float64) and want.dtype == np.uint16
    assert (rig["cam_w"] % 64 or rig["cam_h"] % 4) and rig["proj_w"] != rig["proj_h"]
    depth, disp, st = R.mc3d(surf, rig["cam_map"], rig["proj_map"], K.P1_03[0], blur=False)
    assert np.array_equal(disp, want)
    assert st["n_matched"] == np.count_nonzero(want) > 50 and st["n_disp_overflow"] == 0
    assert st["n_positive"] == (surf > 0).sum() > st["n_in_rect"] > st["n_out_of_range"] >= 3 and st["n_poisoned"] > 0
    assert st["n_nonzero"] > st["n_positive"]  # (negative pixels)


@pytest.mark.parametrize("name", K.RIGS)
def test_float64_surface_names_other_projector_pixels(rigs, name):
    """the fixture's float64 surface is the float32 one widened, but for three pixels whose float32 rounding crosses an id"""
    rig = rigs[name]
    s32, s64 = rig["surf_f32"], rig["surf_f64"]
    diff = np.argwhere(s32.astype(np.float64) != s64)
    assert len(diff) == 3
    wh = rig["proj_w"] * rig["proj_h"]
    for i, j in diff:
        assert np.float32(s64[i, j]) == s32[i, j] and int(np.float32(wh) * s32[i, j]) == int(wh * s64[i, j]) + 1


@pytest.mark.parametrize("name", K.RIGS)
@pytest.mark.parametrize("sign", [0, 1])
def test_depth_equals_the_reference(rigs, name, sign):
    rig = rigs[name]
    want = rig["depth_pos" if sign == 0 else "depth_neg"]
    assert want.dtype == np.float64  # (NumPy 2: float64 scalar / float32 array)
    depth = R.depth_from_disparity(rig["disp_f32"], K.P1_03[sign])
    assert depth.dtype == np.float32 and np.array_equal(depth, want.astype(np.float32))
    assert np.all(np.isfinite(depth)) and np.all((depth == 0) == (rig["disp_f32"] == 0))


def test_hand_built_pixels_of_rig_a(rigs):
    """what the generator asserts, spelt out for the pixels a reader can check against rig_a() by eye"""
    t, d = rigs["a"]["tags"], rigs["a"]["disp_f32"]
    assert d[t["tie_minus_first"]] == 7                       # yc - 3 in front of yc + 3: the first
    assert d[t["cost_50"]] == 4 and d[t["cost_51"]] == 0      # the acceptance bound
    assert d[t["nan_inside"]] == 0 and d[t["nan_outside"]] == 5 and d[t["nan_x_inside"]] == 0
    assert d[t["disp_1"]] == 1 and d[t["disp_0"]] == 0 and d[t["disp_neg"]] == 0  # only the winner is examined
    assert d[t["trunc_not_floor"]] == 11 and d[t["trunc_negative"]] == 15         # int(), not floor
    assert d[t["xc_0"]] == 0 and d[t["xc_1"]] == 399 and d[t["xc_299"]] == 101 and d[t["xc_300"]] == 0  # 0 < xc < 3 * H
    assert d[t["yc_0"]] == 0 and d[t["yc_1"]] == 390 and d[t["yc_14"]] == 390 and d[t["yc_15"]] == 0    # 0 < yc < 3 * W
    assert d[t["v_one"]] == 0 and d[t["v_above_one"]] == 0 and d[t["v_inf"]] == 0 and d[t["v_last"]] == 390
    assert d[t["cam_nan"]] == 0 and d[t["cam_inf"]] == 0 and d[t["v_negative"]] == 0
    assert d[t["win_clip_0"]] == d[t["win_clip_H"]] == d[t["win_full"]] == 390


def test_int_maps():
    from x_maps_amd.mc3d import POISON, mc3d_int_maps
    x = np.array([[-0.5, -0.999, -1.0, -1.5, 0.0, 0.999, 2.9, -2.9]], np.float32)
    y = np.array([[np.nan, np.inf, -np.inf, 1e12, -1e12, 2.0 ** 30, -(2.0 ** 30) - 1024, 7.5]], np.float32)
    m = mc3d_int_maps(x, y)
    assert m.dtype == np.int32 and m.shape == (1, 8, 2) and POISON == R.POISON == np.iinfo(np.int32).min
    assert m[0, :, 0].tolist() == [0, 0, -1, -1, 0, 0, 2, -2]
    assert m[0, :, 1].tolist() == [POISON, POISON, POISON, 2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30, 7]
    assert np.array_equal(m, R.int_maps(x, y))


@pytest.mark.parametrize("name", K.RIGS)
def test_int_maps_on_the_fixture(rigs, name):
    from x_maps_amd.mc3d import POISON, mc3d_int_maps
    rig = rigs[name]
    for key in ("cam_map", "proj_map"):
        got = mc3d_int_maps(*rig[key + "_f"])
        assert np.array_equal(got, rig[key]) and (got == POISON).any()
    py = rig["proj_map_f"][1]
    assert ((py > -1) & (py < 0)).any() and not (rig["proj_map"][..., 1][(py > -1) & (py < 0)] != 0).any()


def test_median_restatement():
    from x_maps_amd.eval_table import median_blur3
    rng = np.random.default_rng(4)
    img = rng.random((7, 9)).astype(np.float32)
    img[rng.random((7, 9)) < 0.4] = 0
    got = R.median_blur3(img)
    assert got.dtype == np.float32 and np.array_equal(got, median_blur3(img))
    assert got[0, 0] == np.sort(np.array([img[0, 0]] * 4 + [img[0, 1]] * 2 + [img[1, 0]] * 2 + [img[1, 1]]))[4]  # replicated corner
    d = R.median_blur3(img.astype(np.float64) + 1e-12)
    assert d.dtype == np.float64 and not np.array_equal(d, d.astype(np.float32))  # float64 stays float64


def test_dense_surfaces_keep_their_ring_lit(rigs):
    for rig in (rigs[n] for n in K.RIGS):
        for dt in (np.float32, np.float64):
            s = K.dense_surface(rig, dt, 1)
            v = R.median_blur3(s)
            h, w = s.shape
            assert all(v[i, j] > 0 for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)))
            assert (v[0] > 0).any() and (v[-1] > 0).any() and (v[:, 0] > 0).any() and (v[:, -1] > 0).any()
            assert ((v > 0) != (s > 0)).any() and (s >= 1).any() and (s < 0).any()


def test_table_builder_on_the_esl_calibration(golden_dir):
    """build_mc3d_tables on the calibration numbers of golden G6 (640 x 480 camera, 1080 x 1920 projector): shapes, dtypes, no
    poisoned entry (both maps are finite over their frames), the reference's limits and window, p1_03 = P1[0, 3] = the rectified
    focal length times the baseline, P0[0, 3] = 0.  The maps' values are unpinned against cv2.undistortPoints."""
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.mc3d import POISON, build_mc3d_tables
    g6 = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    cp = CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g6["camera_K"], g6["camera_D"], g6["projector_K"],
                                  g6["projector_D"], g6["R"], g6["T"])
    t = build_mc3d_tables(cp)
    assert t["cam_map"].shape == (480, 640, 2) and t["proj_map"].shape == (1920, 1080, 2)
    assert t["cam_map"].dtype == t["proj_map"].dtype == np.int32
    assert not (t["cam_map"] == POISON).any() and not (t["proj_map"] == POISON).any()
    assert all(np.isfinite(m).all() for m in t["cam_map_f32"] + t["proj_map_f32"])
    assert (t["nc"], t["max_row_diff"], t["rect_x_limit"], t["rect_y_limit"]) == (128, 50, 5760, 3240)
    assert t["p1_03"] == t["P1"][0, 3] != 0 and t["P0"][0, 3] == 0
    assert abs(abs(t["p1_03"]) - t["P1"][0, 0] * np.linalg.norm(g6["T"])) <= 1e-9 * abs(t["p1_03"])
    # rectified rows agree between the two devices: a camera pixel's row lies inside the projector map's range of rows
    cy, py = t["cam_map"][..., 1], t["proj_map"][..., 1]
    assert py.min() < np.median(cy) < py.max()
