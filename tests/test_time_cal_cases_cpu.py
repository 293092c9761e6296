"""CPU: the NumPy oracle of the projector time-map calibration (tests/time_cal_cases.py) is pinned here -- exact where the
arithmetic is exact, hand-computed where it is a rule -- and every case is shown to reach the loop bound it is named for, so that a
missing edge fails here and cannot pass silently on the GPU (tests/test_gpu_time_cal.py)."""
import math

import numpy as np
import pytest

import time_cal_cases as T


def _truth_affine():
    """the linear time map in the normalisation of the affine case's own surface: [H][W]"""
    s = T.surfaces("affine")[0]
    lo, hi, _ = T.surface_extrema(s)
    W, H = T.PROJ
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return ((1.0 + (u * H + v) / (W * H) * 1000.0) - lo) / (hi - lo)


def test_interior_warp_is_exact_on_an_affine_map():
    r = T.solved("affine", 1, T.PROJ, T.QUAD_AFFINE)
    n, _, _ = T.taps_valid(r["valid"], r["h"], T.PROJ)
    full = n == 4
    assert full.sum() > 1000
    err = np.abs(r["value"] - _truth_affine())[full].max()
    print("interior error", err)
    # bilinear interpolation is exact on affine functions: what remains is a handful of float64 roundings on values of order 1
    assert err <= 1e-12


def test_partial_tap_pixels_stay_within_one_camera_pixel_of_gradient():
    r = T.solved("affine", 1, T.PROJ, T.QUAD_AFFINE)
    n, _, _ = T.taps_valid(r["valid"], r["h"], T.PROJ)
    part = (n > 0) & (n < 4)
    assert part.sum() > 50 and np.array_equal(r["present"], n > 0)
    m, v = r["mean"], r["valid"]
    gx = np.abs(m[:, 1:] - m[:, :-1])[v[:, 1:] & v[:, :-1]].max()
    gy = np.abs(m[1:] - m[:-1])[v[1:] & v[:-1]].max()
    err = np.abs(r["value"] - _truth_affine())[part].max()
    print("partial-tap error", err, "bound", gx + gy)
    # every valid tap lies within one pixel of the position along each axis, and the value is a convex combination of the taps
    assert err < gx + gy


def test_detected_corners_are_pinned():
    assert T.solved("affine", 1, T.PROJ)["corners"] == [(10, 8), (57, 10), (58, 39), (11, 37)]
    assert T.solved("persp", 1, T.PROJ)["corners"] == [(10, 9), (56, 12), (60, 41), (8, 35)]
    assert T.solved("n9", 5, T.PROJ)["corners"] == [(10, 9), (56, 14), (60, 41), (11, 35)]


def test_corner_ties_go_to_the_smallest_raster_index():
    masks = T.corner_masks()
    valid, want = masks["rectangle"]
    n_valid, n_core, got = T.find_corners(valid)
    assert tuple(got) == want and n_valid == 41 * 33 and n_core == 39 * 31
    valid, _ = masks["diamond"]
    core = T.core_mask(valid)
    ys, xs = np.nonzero(core)
    s = xs + ys
    tied = np.nonzero(s == s.min())[0]
    assert len(tied) >= 2  # two core pixels share the minimal x + y
    _, _, got = T.find_corners(valid)
    assert got[0] == (int(xs[tied[0]]), int(ys[tied[0]])) and ys[tied[0]] == ys[tied].min()
    d = xs - ys
    assert (d == d.max()).sum() >= 2 and (s == s.max()).sum() >= 2 and (d == d.min()).sum() >= 2  # ... and so do the other three
    assert got == [(27, 5), (31, 5), (52, 26), (12, 20)]


def test_corner_errors():
    masks = T.corner_masks()
    with pytest.raises(T.CornerError, match="no core pixel"):
        T.find_corners(masks["two_wide"][0])
    assert masks["two_wide"][0].sum() == 2 * 36
    with pytest.raises(T.CornerError, match="coincide"):
        T.find_corners(masks["blob3"][0])
    assert T.core_mask(masks["blob3"][0]).sum() == 1
    with pytest.raises(T.CornerError, match="strictly convex"):
        T.corner_verdict(T.NON_CONVEX)
    with pytest.raises(T.CornerError, match="strictly convex"):
        T.corner_verdict(((0, 0), (5, 5), (10, 10), (0, 10)))  # three points on a line
    T.corner_verdict(T.QUAD_PERSP)
    T.corner_verdict(T.QUAD_PERSP[::-1])  # the other orientation is as convex


def test_detection_never_yields_distinct_corners_that_are_not_convex():
    """The four corners are extreme points of the core set along the two diagonals, in cyclic order, and a tie goes to the end of
    the tied run that IS the neighbouring corner: whenever the verdict fails on detected corners, it is for coinciding ones.  So the
    convexity verdict is reachable only by corners a caller brings (corners=); here over every 3 x 4 core set and random ones."""
    rng = np.random.default_rng(0)
    sets = [np.array([(k >> i) & 1 for i in range(12)], bool).reshape(3, 4) for k in range(1, 1 << 12)]
    sets += [rng.random((7, 9)) < p for p in (0.15, 0.4, 0.7) for _ in range(300)]
    n_ok = n_coincide = 0
    for core in sets:
        ys, xs = np.nonzero(core)
        if not len(xs):
            continue
        picks = (np.argmin(xs + ys), np.argmax(xs - ys), np.argmax(xs + ys), np.argmin(xs - ys))
        corners = [(int(xs[i]), int(ys[i])) for i in picks]
        try:
            T.corner_verdict(corners)
            n_ok += 1
        except T.CornerError as e:
            assert "coincide" in str(e), (core, corners)
            n_coincide += 1
    assert n_ok > 100 and n_coincide > 100


def test_fill_rows_by_hand():
    names, value, present = T.fill_rows()
    out, n_missing, n_unfilled = T.fill(value, present)
    W = value.shape[1]
    row = dict(zip(names, range(len(names))))
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    r = row["start"]
    assert np.array_equal(out[r, :7], f32([value[r, 7]] * 7)) and np.array_equal(out[r, 7:], f32(value[r, 7:]))
    r = row["end"]
    assert np.array_equal(out[r, W - 9:], f32([value[r, W - 10]] * 9)) and np.array_equal(out[r, :W - 9], f32(value[r, :W - 9]))
    r = row["boundary"]
    ml, mr = value[r, 249], value[r, 263]
    want = [ml + (mr - ml) * (float(u - 249) / 14.0) for u in range(250, 263)]
    assert np.array_equal(out[r, 250:263], f32(want)) and np.array_equal(out[r, :250], f32(value[r, :250]))
    r = row["alternating"]
    want = [value[r, u - 1] + (value[r, u + 1] - value[r, u - 1]) * 0.5 for u in range(1, W - 1, 2)]
    assert np.array_equal(out[r, 1:W - 1:2], f32(want)) and out[r, W - 1] == f32(value[r, W - 2])
    assert np.array_equal(out[row["full"]], f32(value[row["full"]]))
    assert not out[row["empty"]].any() and n_unfilled == 1
    assert n_missing == 7 + 9 + 13 + W // 2 + W


def test_grouping_does_not_change_a_bit():
    for name in ("n9", "n9_f32"):
        a = T.accumulated(name, T.GROUPINGS["one"])
        for g in ("4+5", "nine"):
            b = T.accumulated(name, T.GROUPINGS[g])
            assert a.sum.tobytes() == b.sum.tobytes() and np.array_equal(a.cnt, b.cnt)
    assert T.surfaces("n9_f32").dtype == np.float32 and T.surfaces("n9").dtype == np.float64


def test_homography_maps_the_corners():
    for order in range(8):
        h = T.proj_to_cam(T.PROJ, T.QUAD_PERSP, order).reshape(3, 3)
        W, H = T.PROJ
        for k, (u, v) in enumerate(((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))):
            p = h @ (u, v, 1.0)
            assert np.allclose(p[:2] / p[2], T.QUAD_PERSP[T.SYMMETRIES[order][k]], atol=1e-9)
    assert len({s for s in T.SYMMETRIES}) == 8


def test_cases_reach_what_they_are_named_for():
    chunks = lambda size: math.ceil(size[0] * size[1] / T.RED_CHUNK)
    assert chunks(T.CAM) == 2 and chunks(T.CAM_SMALL) == 1
    assert [len(T.surfaces(n)) for n in ("n1", "n3", "n9")] == [1, 3, 9]
    assert T.surfaces("small").shape[1:] == T.CAM_SMALL[::-1]
    # skipped surfaces: an all-zero one and a single-valued one, in the middle of the group
    o = T.accumulated("skipped")
    assert (o.n_added, o.n_skipped) == (5, 2)
    s = T.surfaces("skipped")
    assert not s[1].any() and len(np.unique(s[3][s[3] != 0])) == 1 and T.surface_extrema(s[0])[2] > 0 and T.surface_extrema(s[4])[2] > 0
    # min_count edges
    o = T.accumulated("n9")
    assert T.min_count_for(0.5, o.n_used) == 5 and (o.cnt == 4).any() and (o.cnt == 5).any()
    mean, valid = o.mean(5)
    assert not valid[o.cnt == 4].any() and valid[o.cnt == 5].all() and not mean[~valid].any()
    # fill trips and missing runs at both ends of a row
    assert [math.ceil(w / T.BLOCK) for w, _ in T.PROJ_SIZES] == [1, 2, 3] and T.PROJ_SIZES[0][0] < 64
    for size in T.PROJ_SIZES:
        r = T.solved("n9", T.WIDE_MIN_COUNT, size, T.QUAD_WIDE)
        p = r["present"]
        assert (~p[:, 0] & ~p[:, -1] & p.any(1)).any() and r["n_unfilled"] >= 1 and r["n_missing"] > 0
        inner = [(np.diff(np.nonzero(row)[0]) > 1).any() for row in p if row.any()]
        assert any(inner)  # a missing run between two present pixels
        assert T.solved("n9", 5, size)["n_missing"] == 0  # detected corners lie inside the valid area
    names, value, present = T.fill_rows()
    assert value.shape[1] == 300 and not present[2, 250:263].any() and present[2, 249] and present[2, 263]
    # warp positions
    mean, valid = T.warp_probe()
    res = {k: T.warp(mean, valid, h, T.WARP_PROBE_SIZE) for k, h in T.WARP_PROBES.items()}
    val, pres = res["centre"]
    assert np.array_equal(val[pres], mean[4:8, 5:10][pres]) and not pres[1, 2] and pres.sum() == 19  # exactly the pixel under it
    val, pres = res["last"]
    assert pres.all() and val[3, 4] == mean[27, 39]
    val, pres = res["outside"]
    assert pres[:3, :3].all() and not pres[3].any() and not pres[:, 3:].any()
    assert val[0, 2] == (0.5 * 0.5 * mean[25, 39] + 0.5 * 0.5 * mean[26, 39]) / (0.5 * 0.5 + 0.5 * 0.5)
    val, pres = res["before"]
    assert not pres[:, 0].any() and pres[:, 1:].all()
    assert val[0, 1] == (0.5 * 0.5 * mean[0, 0]) / (0.5 * 0.5)
    for k in ("d_zero", "nan"):
        val, pres = res[k]
        assert not pres[:, :3].any() and pres[:, 3:].all() and not val[~pres].any()
    n, _, _ = T.taps_valid(valid, T.WARP_PROBES["half"], T.WARP_PROBE_SIZE)
    assert n.min() == 3 and n.max() == 4
    n, _, _ = T.taps_valid(T.solved("n9", 5, T.PROJ)["valid"], T.ARBITRARY_H, T.PROJ)
    assert set(np.unique(n)) == {0, 1, 2, 3, 4}


def test_the_products_host_side_agrees_with_the_oracle():
    """x_maps_amd.time_map_calibration's host code -- the homography solve, the corner orders, the check of a caller's corners --
    against the oracle's, and the ctypes struct against the header's layout (2 x u64, 2 x u32, 8 x i32, 2 x u32)"""
    import ctypes
    from x_maps_amd import _native as N
    from x_maps_amd import time_map_calibration as TMC
    assert TMC.CORNER_ORDERS == T.SYMMETRIES
    W, H = T.PROJ
    src = ((0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1))
    for quad in (T.QUAD_AFFINE, T.QUAD_PERSP, T.QUAD_WIDE):
        for order in range(8):
            got = TMC.homography(src, [quad[k] for k in TMC.CORNER_ORDERS[order]])
            assert got.tobytes() == T.proj_to_cam(T.PROJ, quad, order).tobytes()
    TMC.check_corners(T.QUAD_PERSP)
    with pytest.raises(ValueError, match="strictly convex"):
        TMC.check_corners(T.NON_CONVEX)
    with pytest.raises(ValueError, match="coincide"):
        TMC.check_corners(((1, 1), (5, 1), (5, 1), (1, 5)))
    assert ctypes.sizeof(N.xm_timecal_stats) == 64 and N.xm_timecal_stats.corners.offset == 24 and N.xm_timecal_stats.n_missing.offset == 56
