"""CPU: the NumPy restatement of ESL-init (tests/esl_init_ref.py) against the reference's own outputs (golden G11, written by
tests/golden/make_golden_esl_init.py from python/eval/compute_depth_esl.py), array for array; the fused definition (only the
rectified pixels the back map references are searched) against the staged composition on random maps; and the host-side pieces of
x_maps_amd.esl_init that need no GPU."""
import os

import numpy as np
import pytest

import esl_init_cases as K
import esl_init_ref as R


@pytest.fixture(scope="module")
def g11(golden_dir):
    return dict(np.load(os.path.join(golden_dir, K.G11)))


@pytest.mark.parametrize("tag,shape", [("a", (12, 1100)), ("b", (3, 2300))])
def test_disparity_init_equals_the_reference(g11, tag, shape):
    cam, proj, want = g11[f"{tag}_cam_rect"], g11[f"{tag}_proj_rect"], g11[f"{tag}_disparity"]
    assert cam.shape == shape and cam.dtype == np.float64 and proj.dtype == np.float32 and want.dtype == np.uint16
    got = R.disparity_init(cam, proj)
    assert np.array_equal(got, want)
    assert want.max() == 899 or tag == "b"
    assert np.count_nonzero(want) > 100


def test_hand_built_rows_of_the_fixture(g11):
    """what the generator asserts, spelt out for the rows a reader can check by eye"""
    d = g11["a_disparity"]
    assert not d[1].any()                       # no candidate
    assert d[2, 100] == 0 and d[2, 200] == 100  # one candidate -> 0; two -> the nearer (0.4 at column 300)
    assert d[3, 10] == 5 and d[3, 20] == 899    # exact match at the window's first column; winner at its last
    assert d[4, 50] == 5                        # closer values at c + 4 and c + 900 do not win
    assert d[5, 100] == 20                      # e + delta in front of e - delta: the first
    assert d[6, 200] == 10                      # cost 0 twice: the first
    assert d[7, 300] == 10 and d[7, 301] == 0 and d[7, 302] == 0  # all costs +inf: the first; values <= 0 skipped
    assert not d[0, 1095:].any() and np.all(g11["a_cam_rect"][0, 1095:] > 0)  # empty windows


def test_projector_time_surface(g11):
    want = g11["proj_7x11"]
    assert np.array_equal(R.get_projector_time_surface(7, 11), want)
    from x_maps_amd.esl_init import get_projector_time_surface
    got = get_projector_time_surface(7, 11)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    big = get_projector_time_surface(108, 192)  # (the vectorised form against the loop beyond the fixture's size)
    assert np.array_equal(big, R.get_projector_time_surface(108, 192))


@pytest.mark.parametrize("sign", ["pos", "neg"])
def test_remap_back_and_depth(g11, sign):
    disp_cam = R.remap_nearest_i16(g11["a_disparity"], g11["back_map"])
    assert np.array_equal(disp_cam.astype(np.float32), g11["disp_cam"])
    depth = R.depth_from_disparity(disp_cam, float(g11[f"p1_03_{sign}"]))
    want = g11[f"depth_{sign}"]
    assert want.dtype == np.float64  # (NumPy 2: float64 scalar / float32 array)
    assert depth.dtype == np.float32 and np.array_equal(depth, want.astype(np.float32))
    assert np.all(np.isfinite(depth)) and np.all((depth == 0) == (disp_cam == 0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fused_definition_equals_the_staged_composition(dtype):
    rig = K.make_rig()
    r2c, c2r = rig["rect_to_cam"], rig["cam_to_rect"]
    # the rig holds what it is for: entries outside both frames, a shared rectified pixel
    assert (r2c[..., 0] < 0).any() and (r2c[..., 0] >= rig["rect_w"]).any() and (r2c[..., 1] >= rig["rect_h"]).any()
    assert (c2r[..., 0] < 0).any() and (c2r[..., 0] >= rig["cam_w"]).any() and (c2r[..., 1] >= rig["cam_h"]).any()
    assert np.array_equal(r2c[2, 0], r2c[0, 0])
    surfaces = K.make_surfaces(rig, 5, dtype)
    for i, s in enumerate(surfaces):
        for p in (812.25, -812.25):
            d1, c1, st1, _ = R.depth_init_staged(s, c2r, r2c, rig["proj_rect"], p)
            d2, c2, st2 = R.depth_init_fused(s, c2r, r2c, rig["proj_rect"], p)
            assert np.array_equal(d1, d2) and np.array_equal(c1, c2) and st1 == st2, i
        if i in (1, 2):
            assert st2["n_searched"] == 0 and not d2.any() and (st2["n_nonzero"] == 0) == (i == 1)
        else:
            assert st2["n_matched"] > 20 and st2["n_searched"] > st2["n_matched"]
            assert c2[0, 0] == c2[2, 0]


def test_table_builder_on_the_esl_calibration(g11, golden_dir):
    """build_esl_init_tables on the calibration numbers of golden G6 (a 640 x 480 camera, a 1920 x 1080 projector; the rectified
    frame at the projector's size to keep this quick): shapes, dtypes, the sign convention (p1_03 is the pair's non-zero P[0, 3])
    and the geometry's self-consistency -- the forward map undoes the back map to within their two roundings.  The maps' rounding
    itself is unpinned against cv2."""
    from x_maps_amd.calibration import CamProjCalibrationParams
    from x_maps_amd.esl_init import build_esl_init_tables
    g6 = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    cw, ch, rw, rh = 640, 480, 1920, 1080
    cp = CamProjCalibrationParams(cw, ch, rw, rh, rw, rh, g6["camera_K"], g6["camera_D"], g6["projector_K"], g6["projector_D"],
                                  g6["R"], g6["T"])
    t = build_esl_init_tables(cp)
    assert t["cam_to_rect_map"].shape == (rh, rw, 2) and t["rect_to_cam_map"].shape == (ch, cw, 2)
    assert t["cam_to_rect_map"].dtype == t["rect_to_cam_map"].dtype == np.int16
    assert t["proj_rect"].shape == (rh, rw) and t["proj_rect"].dtype == np.float32 and np.count_nonzero(t["proj_rect"]) > rw * rh // 4
    assert t["p1_03"] == t["P1"][0, 3] != 0 and t["P0"][0, 3] == 0 and (t["min_disp"], t["max_disp"]) == (5, 900)
    rx, ry = t["rect_to_cam_map"][..., 0].astype(int), t["rect_to_cam_map"][..., 1].astype(int)
    ok = (rx >= 0) & (rx < rw) & (ry >= 0) & (ry < rh)
    assert ok.mean() > 0.5
    back = t["cam_to_rect_map"][ry[ok], rx[ok]].astype(int)
    y, x = np.nonzero(ok)
    # half a rectified pixel of rounding in the back map is at most half a camera pixel here (the rectified frame is the finer
    # one: focal length P0[0, 0] >= the camera's), plus the forward map's own half pixel: strictly less than 1.5, so at most 1
    assert t["P0"][0, 0] >= max(g6["camera_K"][0, 0], g6["camera_K"][1, 1])
    assert np.abs(back[:, 0] - x).max() <= 1 and np.abs(back[:, 1] - y).max() <= 1
