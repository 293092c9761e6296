"""-m gpu: the evaluation metrics on the device (xm_eval_stats, csrc/xmaps_eval.hpp) against tests/eval_ref.py at every trip
count of k_eval_stats' grid-stride loop -- one block per BLOCK * 8 pixels, so up to 8 trips per thread, and more under the grid's
cap of 2048 blocks, which takes 2048 * 2048 pixels to reach --, on partial waves and blocks, and at every value edge.

Inputs of the shape tests: ground truth and errors are multiples of 1/8, so every float32 difference and square is exact and
every float64 sum too, in any order; the ground truth lies in [0, 90), which puts the margin (about 0.45) well away from a
multiple of 1/8.  Before the GPU is touched each case asserts that no pixel's error is within 1e-3 * margin of the margin: the
two margins (exact here, a float64 sum in some order there) agree to 1e-9, so no count can depend on which one is used.

Then: n_valid and n_gt_zero are equal; fillrate and the three percentages are quotients of the same integers and EQUAL as doubles;
margin and rmse agree to rtol 1e-9 (a float64 sum of N <= 2^22.01 non-negative terms in any order is within N * 2^-53 = 4.7e-10
of the exact sum; 1.2e-10 for the shapes up to 2^20).  (The unmarked test at the end checks the shapes against the kernel's
constants on the CPU.)"""
import math
import os
import re

import numpy as np
import pytest

import eval_ref as E

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCK, ITEMS, CAP = 256, 8, 2048  # threads per block, pixels per thread the grid is sized for, the grid's cap (checked at the end)
STRIDED = (513, 1025)  # 525 825 pixels, more than CAP * BLOCK: 257 blocks, 8 trips, the last 65 281 threads wide
CAPPED = (2049, 2049)  # 4 198 401 pixels: 2051 blocks asked for, 2048 given; 9 trips, the last 4097 threads wide
SHAPES = [STRIDED, (1, 1), (1, 63), (1, 64), (1, 65), (7, 37), (256, 2048), (257, 2048), CAPPED]


def _launch(shape):
    """(blocks, trips of thread 0, threads with work in the last trip) of k_eval_stats on a map of that shape"""
    n = shape[0] * shape[1]
    grid = min(-(-n // (BLOCK * ITEMS)), CAP)
    return grid, -(-n // (grid * BLOCK)), n - (n - 1) // (grid * BLOCK) * (grid * BLOCK)


MIN_D, MAX_D = 20.0, 120.0


def _maps(shape, seed):
    """(est, gt): gt in [0, 90) and errors in multiples of 1/8, a fifth of the ground truth missing, estimates missing, beyond
    max_depth and below min_depth as in golden G8"""
    rng = np.random.default_rng(seed)
    gt = (rng.integers(1, 720, shape) / 8).astype(np.float32)
    gt[rng.random(shape) < 0.2] = 0
    err = rng.integers(-120, 121, shape) / 8  # up to 15: all three thresholds are crossed
    err[rng.random(shape) < 0.3] = 0
    est = (gt + err).astype(np.float32)
    est[rng.random(shape) < 0.2] = 0
    est[rng.random(shape) < 0.02] = 150
    est[rng.random(shape) < 0.02] = 5
    return est, gt


def _assert_clear_of_the_margin(ref, est, gt):
    """a condition on the INPUTS: no pixel so close to the margin that the last bits of the margin decide its side"""
    m = ref["margin"]
    if math.isnan(m):
        return
    a = E.abs_error(est, gt).astype(np.float64)
    a = a[np.isfinite(a)]
    assert not (np.abs(a - m) < 1e-3 * m).any(), (m, a[np.abs(a - m) < 1e-3 * m])


def _check(est, gt, bounds=None):
    """bounds: (min_depth, max_depth) of load_and_filter, or None for the estimate as it is"""
    from x_maps_amd.eval_metrics import evaluation_stats
    filtered = E.load_and_filter(est, gt, *bounds) if bounds else est
    ref = E.evaluation_stats(filtered, gt)
    _assert_clear_of_the_margin(ref, filtered, gt)
    r = evaluation_stats(est, gt, **({"min_depth": bounds[0], "max_depth": bounds[1]} if bounds else {}))
    got = {f: getattr(r, f) for f in E.FLOATS}
    print(est.shape, bounds, got, r.n_valid, r.n_gt_zero, {k: ref[k] for k in E.FLOATS + E.COUNTS})
    assert (r.n_valid, r.n_gt_zero) == (ref["n_valid"], ref["n_gt_zero"])
    for f in ("fillrate", "perc_1", "perc_5", "perc_10"):
        assert np.array_equal(got[f], ref[f], equal_nan=True), (f, got[f], ref[f])  # equal as doubles (NaN and +-inf as NumPy's)
    for f in ("margin", "rmse"):
        if math.isfinite(ref[f]):
            np.testing.assert_allclose(got[f], ref[f], rtol=1e-9, atol=0, err_msg=f)
        else:
            assert np.array_equal(got[f], ref[f], equal_nan=True), (f, got[f], ref[f])
    return ref


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes_equal_the_reference(shape):
    est, gt = _maps(shape, seed=shape[0] * 10007 + shape[1])
    if shape == (1, 1):
        est[0, 0], gt[0, 0] = 44.0, 43.0  # one pixel with ground truth and an error that counts once
    if shape in (STRIDED, CAPPED):  # what only the last trip reads must matter: pixels of every kind in it
        tail_e, tail_g = est.ravel()[-_launch(shape)[2]:], gt.ravel()[-_launch(shape)[2]:]
        with_gt = tail_g > 0
        assert 4000 < len(tail_g) < 70000 and (tail_g == 0).sum() > 100 and (with_gt & (tail_e > 0)).sum() > 100
        assert (np.abs(tail_g - tail_e)[with_gt] > 10).sum() > 100 and (np.abs(tail_g - tail_e)[with_gt] < 0.25).sum() > 100
    for bounds in (None, (MIN_D, MAX_D)):
        ref = _check(est, gt, bounds)
        if est.size > 1:
            assert 0 < ref["n_gt_zero"] < est.size and ref["n10"] > 0 and ref["n_valid"] > 0
        if est.size > 100:
            assert 0 < ref["n10"] < ref["n5"] < ref["n1"] < est.size and ref["n_close"] > ref["n_gt_zero"] and ref["rmse"] > 0


EDGE_MIN, EDGE_MAX = 0.25, 120.0  # (the edge map's estimates of 0.5 must pass the filter)


def _edge_map():
    """64 x 64, by hand: a quiet background (error 1/8, a third of it without ground truth) and one pixel per edge.
    -> est, gt, {name: flat index}"""
    f32 = np.float32

    def up(v):
        return np.nextafter(f32(v), f32(np.inf))
    gt = np.full((64, 64), 50.0, f32)
    est = np.full((64, 64), 50.125, f32)
    gt[:, ::3] = 0
    est[::4, :] = 0
    px = {}
    at = iter(range(65, 4096, 67))  # scattered over the rows and the waves

    def put(name, e, g):
        i = next(at)
        est.ravel()[i], gt.ravel()[i] = e, g
        px[name] = i
    for v in (1, 5, 10):
        put(f"err_{v}", f32(50 + v), f32(50))  # exactly v: not counted
        put(f"err_{v}_neg", f32(50 - v), f32(50))
        put(f"err_{v}_up", f32(0.5), up(v) + f32(0.5))  # gt - est is one float32 step above v: counted
        assert up(v) + f32(0.5) - f32(0.5) == up(v) and up(v) > v
    put("est_max", f32(EDGE_MAX), f32(100))  # zeroed by the filter
    put("est_max_in", np.nextafter(f32(EDGE_MAX), f32(0)), f32(100))  # kept
    put("est_min", f32(EDGE_MIN), f32(30))  # zeroed
    put("est_min_in", up(EDGE_MIN), f32(30))  # kept
    put("gt_neg_zero", f32(33), f32(-0.0))  # treated as zero
    put("gt_neg", f32(25), f32(-3))  # not zero, not in the margin's mean, counted in the percentages (error 28)
    put("gt_neg_close", f32(-3), f32(-3))
    put("nan_over_gt", f32(np.nan), f32(50))
    put("nan_over_hole", f32(np.nan), f32(0))
    put("inf_over_gt", f32(np.inf), f32(50))
    put("inf_over_hole", f32(np.inf), f32(0))
    assert np.signbit(gt).sum() == 3 and len(set(px.values())) == len(px) == 20
    return est, gt, px


@gpu
@pytest.mark.parametrize("variant", ["plain", "filtered", "plain_finite"])
def test_value_edges_equal_the_reference(variant):
    est, gt, px = _edge_map()
    if variant == "plain_finite":  # without the infinite estimate over ground truth, so that the unfiltered RMSE is a number
        est.ravel()[px["inf_over_gt"]] = 50.125
    bounds = (EDGE_MIN, EDGE_MAX) if variant == "filtered" else None
    # what the map is for, from the reference alone
    e = (E.load_and_filter(est, gt, *bounds) if bounds else est).ravel()
    a = E.abs_error(e.reshape(64, 64), gt).ravel()
    ref = E.evaluation_stats(e.reshape(64, 64), gt)
    for v, n in ((1, "n1"), (5, "n5"), (10, "n10")):
        assert a[px[f"err_{v}"]] == v and a[px[f"err_{v}_neg"]] == v and a[px[f"err_{v}_up"]] == np.nextafter(np.float32(v), np.float32(99))
        with np.errstate(invalid="ignore"):
            assert ref[n] == (a > v).sum() == (a >= v).sum() - 2  # strict: the two pixels exactly on the level do not count
    assert a[px["gt_neg_zero"]] == 0 and a[px["nan_over_hole"]] == 0 and a[px["inf_over_hole"]] == 0 and a[px["gt_neg"]] == 28
    assert np.isnan(a[px["nan_over_gt"]]) and a[px["gt_neg_close"]] == (3 if bounds else 0)  # (a negative estimate is <= min_depth)
    assert gt.ravel()[px["gt_neg_zero"]] == 0 and ref["n_gt_zero"] == (gt == 0).sum() > 1000  # -0.0 is a hole ...
    assert ref["n_gt_pos"] == 4096 - ref["n_gt_zero"] - 2  # ... and -3 is neither a hole nor in the margin's mean
    assert math.isfinite(ref["margin"]) and (ref["rmse"] == math.inf) == (variant == "plain") and not math.isnan(ref["rmse"])
    if bounds:  # on the bounds: zeroed; one float32 step inside: kept
        assert e[px["est_max"]] == 0 and e[px["est_min"]] == 0 and e[px["inf_over_gt"]] == 0 and e[px["err_1_up"]] == 0.5
        assert 119.99 < e[px["est_max_in"]] < EDGE_MAX and EDGE_MIN < e[px["est_min_in"]] < 0.2501
        assert np.isnan(e[px["nan_over_gt"]]) and e[px["nan_over_hole"]] == 0 and e[px["gt_neg_zero"]] == 0 and e[px["gt_neg"]] == 25
    else:
        assert a[px["inf_over_gt"]] == (0.125 if variant == "plain_finite" else np.inf)
    _check(est, gt, bounds)


@gpu
@pytest.mark.parametrize("filt", [False, True])
def test_no_positive_ground_truth_and_a_perfect_estimate(filt):
    bounds = (MIN_D, MAX_D) if filt else None
    est, _ = _maps((64, 64), seed=3)
    for gt in (np.zeros((64, 64), np.float32), np.where(np.arange(4096).reshape(64, 64) % 5 == 0, -2.5, 0).astype(np.float32)):
        ref = _check(est, gt, bounds)  # NaN margin; fillrate -inf (no pixel with ground truth) or negative
        assert math.isnan(ref["margin"]) and ref["n_close"] == 0 and ref["rmse"] == 0 and ref["fillrate"] < 0
    assert E.evaluation_stats(est, np.zeros((64, 64), np.float32))["fillrate"] == -math.inf
    _, gt = _maps((64, 64), seed=4)
    ref = _check(gt.copy(), gt, bounds)  # est == gt everywhere
    assert ref["rmse"] == 0 and ref["n_gt_pos"] > 0
    if filt:  # ... but for the estimates the filter takes, at or below min_depth: their whole depth is the error
        assert ref["n_valid"] < ref["n_gt_pos"] and ref["n10"] == ref["n_gt_pos"] - ref["n_valid"] - int(((gt > 0) & (gt <= 10)).sum())
    else:
        assert ref["fillrate"] == 1.0 and ref["n1"] == 0 and ref["n_valid"] == ref["n_gt_pos"]


def test_shapes_cross_the_loop_bounds():
    """CPU: the constants of k_eval_stats' launch, read from the sources, and what each shape is for"""
    host = open(os.path.join(ROOT, "x_maps_amd", "csrc", "host", "xm_api_misc.hpp")).read()
    common = open(os.path.join(ROOT, "x_maps_amd", "csrc", "xmaps_geometry.hpp")).read()  # (BLOCK: shared with the host's plan)
    block = int(re.search(r"constexpr\s+int\s+(?:\w+\s*=\s*\d+\s*,\s*)*BLOCK\s*=\s*(\d+)", common).group(1))
    body = host[host.index("int xm_eval_stats("):]
    per_block = re.search(r"grid\s*=\s*grid_for\(n,\s*BLOCK\s*\*\s*(\d+)\)", body)
    cap = re.search(r"if\s*\(grid\s*>\s*(\d+)\)\s*grid\s*=\s*(\d+);", body)
    assert per_block and cap and cap.group(1) == cap.group(2)
    assert (block, int(per_block.group(1)), int(cap.group(1))) == (BLOCK, ITEMS, CAP)
    assert STRIDED[0] * STRIDED[1] > CAP * BLOCK  # more pixels than the capped grid has threads ...
    assert _launch(STRIDED) == (257, 8, 65281)  # ... a grid this map does not get: 257 blocks, 8 trips, the last partly filled
    assert _launch(CAPPED) == (CAP, 9, 4097) and CAPPED[0] * CAPPED[1] > CAP * BLOCK * ITEMS  # the cap, and one trip more than ITEMS
    assert _launch((256, 2048)) == (256, 8, 256 * BLOCK) and _launch((257, 2048)) == (257, 8, 257 * BLOCK)  # full trips only
    assert _launch((1, 1))[:2] == _launch((1, 63))[:2] == _launch((1, 64))[:2] == _launch((1, 65))[:2] == (1, 1)  # partial waves
    assert _launch((7, 37)) == (1, 2, 3) and BLOCK % 64 == 0  # a second trip of three lanes
    assert all(sh in SHAPES for sh in (STRIDED, CAPPED, (1, 1), (1, 63), (1, 64), (1, 65), (7, 37), (256, 2048), (257, 2048)))
