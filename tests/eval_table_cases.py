"""Inputs and the NumPy yardstick of the evaluation table's device scorer (xm_eval_table_*, x_maps_amd.eval_table.EvalTable), shared
by tests/golden/make_golden_eval_table.py (golden G15), tests/test_eval_table_golden_cpu.py and tests/test_gpu_eval_table.py.

The inputs are a seeded recipe, not files: G15's arrays compress to about 6 MB, so the fixture stores their SHA-256 and the recipe
lives here.  make_case builds a smooth scene whose depths are multiples of 1/8 between 37 and 77, ground-truth scans of it with
holes and a strip of columns no scan covers, and per method estimates of it with errors in multiples of 1/8 up to +-15, a third of
them exact, a fifth missing, some at 150 (beyond max_depth) and some at 5 (below min_depth), plus per method a systematic error
on stripes of columns, the same in every scan, so that a "1 sec" row keeps errors beyond 10.  Multiples of 1/8: every float32
difference and square of a per-scan row is exact and so is every float64 sum, in any order (tests/test_gpu_eval_edges.py derives
this); the margin, about 0.57, lies between the error levels 0.5 and 0.625.

table() is the yardstick: combine_mc3d, load_and_filter and evaluation_stats restated on arrays with the pieces the repository
already pins -- eval_table.median_blur3, eval_ref.load_and_filter, eval_ref.evaluation_stats -- plus the two float64 sums of every
cell.  tests/test_eval_table_golden_cpu.py holds it (and eval_table.combine_depth_maps, its file form) to the reference's own
outputs in G15."""
import hashlib

import numpy as np

import eval_ref as E

MIN_D, MAX_D = 20, 120  # create_evaluation_table.py:95-96
G15_SHAPE, G15_SCANS, G15_SEED = (480, 640), 4, 15  # (combine_mc3d hard-codes 480 x 640)
G15_METHODS, G15_ONE_SEC = ("x_maps", "esl_init", "mc3d"), ("mc3d",)
G15_ROWS = G15_METHODS + ("mc3d_1s",)
SAMPLE_STEP = 97  # the golden keeps every 97th pixel of the two combined maps beside their hashes


def make_case(shape, n_scans, n_methods, seed):
    """-> gt float32 [n_scans][h][w], est float32 [n_methods][n_scans][h][w], info (where the hand-placed pixels are)"""
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    scene = np.round(8 * (57 + 20 * np.sin(xx / 90.0 + 0.3) * np.cos(yy / 70.0))) / 8
    gt = np.empty((n_scans, h, w), np.float32)
    est = np.empty((n_methods, n_scans, h, w), np.float32)
    # a method's systematic error, the same in every scan, on stripes six columns wide (a sixteenth of the columns): what survives
    # the mean and the median of a "1 sec" row
    bias = [np.where((xx // 6 + m) % 16 == 0, (rng.integers(-100, 101, w // 6 + 1) / 8)[xx // 6], 0.0) for m in range(n_methods)]
    for s in range(n_scans):
        full = scene + rng.integers(-2, 3, shape) / 8
        g = full.copy()
        g[rng.random(shape) < 0.15] = 0
        gt[s] = g
        for m in range(n_methods):
            err = rng.integers(-120, 121, shape) / 8
            err[rng.random(shape) < 0.3] = 0
            e = full + err + bias[m]
            e[rng.random(shape) < 0.2] = 0
            e[rng.random(shape) < 0.02] = 150
            e[rng.random(shape) < 0.02] = 5
            est[m, s] = e
    info = {}
    if w >= 16:  # a strip of columns without ground truth in any scan
        c0, c1 = w * 7 // 8 - max(w // 32, 3), w * 7 // 8
        gt[:, :, c0:c1] = 0
        info["strip"] = (c0, c1)
        if h >= 5:
            lone, hole = (h // 2, (c0 + c1) // 2), (h // 3, w // 3)
            gt[:, lone[0], lone[1]] = scene[lone]  # covered by every scan, alone in the strip: the median takes it away
            gt[:, hole[0], hole[1]] = 0  # covered by none, alone among covered pixels: the median fills it
            gt[:, hole[0] - 1:hole[0] + 2, hole[1] - 1] = scene[hole[0] - 1:hole[0] + 2, hole[1] - 1]
            gt[:, hole[0] - 1:hole[0] + 2, hole[1] + 1] = scene[hole[0] - 1:hole[0] + 2, hole[1] + 1]
            info["lone"], info["hole"] = lone, hole
    if h * w >= 64:  # depths exactly on the bounds, in the ground truth and in the estimates: both are zeroed
        flat = rng.choice(h * w, 8, replace=False)
        for k, i in enumerate(flat):
            y, x = divmod(int(i), w)
            v = (MIN_D, MAX_D)[k % 2]
            if k < 4:
                gt[k % n_scans, y, x] = v
            else:
                est[k % n_methods, k % n_scans, y, x] = v
        info["on_bounds"] = [divmod(int(i), w) for i in flat]
    return gt, est, info


def g15_inputs():
    """-> gt [4][480][640], {method: [4][480][640]}, info"""
    gt, est, info = make_case(G15_SHAPE, G15_SCANS, len(G15_METHODS), G15_SEED)
    return gt, {name: est[m] for m, name in enumerate(G15_METHODS)}, info


def inputs_sha256(gt, est):
    """of the bytes of the ground truth and of every method's stack, in the methods' order"""
    d = hashlib.sha256(np.ascontiguousarray(gt, np.float32).tobytes())
    for e in (est.values() if isinstance(est, dict) else est):
        d.update(np.ascontiguousarray(e, np.float32).tobytes())
    return d.hexdigest()


def map_sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def combine_arrays(maps, min_d=MIN_D, max_d=MAX_D):
    """eval_table.combine_depth_maps (esl_utilities.py:153-175) on arrays -> (combined, avg_depth, the mean before the median)"""
    from x_maps_amd.eval_table import median_blur3
    acc = np.zeros(maps[0].shape, np.float32)
    count = np.zeros(maps[0].shape, np.float32)
    with np.errstate(invalid="ignore"):
        for m in maps:
            d = np.array(m, np.float32, copy=True)
            d[d >= max_d] = 0
            d[d <= min_d] = 0
            acc += d
            count += d > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = acc / count
    mean[count == 0] = 0
    comb = median_blur3(mean)
    avg = float(comb[comb > 0].astype(np.float64).sum() / max(int((comb > 0).sum()), 1))
    return comb, avg, mean


def cell(est, g):
    """eval_ref.evaluation_stats plus the two float64 sums the device reports (np.sum in float64: exact for multiples of 1/8)"""
    r = E.evaluation_stats(est, g)
    with np.errstate(all="ignore"):
        d = g - est
        r["sum_gt"] = float(g[g > 0].astype(np.float64).sum())
        r["sum_sq"] = float((d * d)[(g > 0) & (est > 0)].astype(np.float64).sum())
    return r


def table(gt, est, one_sec=(), min_d=MIN_D, max_d=MAX_D):
    """gt [S][h][w]; est: a list (or dict's values) of [S][h][w]; one_sec: indices of the methods with a 1-sec row.
    -> {"mask", "avg_depth", "mean", "one_sec_maps": {m: map}, "cells": [rows][S] of cell(), "filtered": [rows][S] of (e, g)}
    rows: the methods, then the 1-sec rows by ascending m"""
    est = list(est.values()) if isinstance(est, dict) else list(est)
    mask, avg, mean = combine_arrays(gt, min_d, max_d)
    g = [E.load_and_filter(x, mask, min_d, max_d) for x in gt]
    maps = {m: combine_arrays(est[m], min_d, max_d)[0] for m in sorted(one_sec)}
    pairs = [[(E.load_and_filter(e[s], mask, min_d, max_d), g[s]) for s in range(len(gt))] for e in est]
    pairs += [[(maps[m], g[s]) for s in range(len(gt))] for m in sorted(one_sec)]
    return {"mask": mask, "avg_depth": avg, "mean": mean, "one_sec_maps": maps, "filtered": pairs,
            "cells": [[cell(e, gg) for e, gg in row] for row in pairs]}


def assert_clear_of_the_margin(tab):
    """a condition on the INPUTS (tests/test_gpu_eval_edges.py): no pixel's error within 1e-3 * margin of the margin"""
    for row, cells in zip(tab["filtered"], tab["cells"]):
        for (e, g), c in zip(row, cells):
            m = c["margin"]
            if np.isnan(m):
                continue
            a = E.abs_error(e, g).astype(np.float64)
            a = a[np.isfinite(a)]
            near = np.abs(a - m) < 1e-3 * m
            assert not near.any(), (m, a[near][:5])


# ---- golden G15 (tests/golden/make_golden_eval_table.py): what both the yardstick and the device are held to ----

def check_cells_against_golden(g15, get):
    """get(r, s) -> dict with eval_ref's FLOATS and COUNTS"""
    assert tuple(g15["rows"]) == G15_ROWS and tuple(g15["floats"]) == E.FLOATS
    assert tuple(g15["counts_names"]) == E.COUNTS
    for r in range(len(G15_ROWS)):
        for s in range(G15_SCANS):
            got, want, cnt = get(r, s), dict(zip(g15["floats"], g15["results"][r, s])), dict(zip(g15["counts_names"], g15["counts"][r, s]))
            for k in E.COUNTS:
                assert int(got[k]) == int(cnt[k]), (r, s, k, got[k], cnt[k])
            for k in ("fillrate", "perc_1", "perc_5", "perc_10"):
                assert float(got[k]) == float(want[k]), (r, s, k, got[k], want[k])
            for k in ("margin", "rmse"):
                np.testing.assert_allclose(float(got[k]), float(want[k]), rtol=1e-6, atol=0, err_msg=f"{r} {s} {k}")


def check_maps_against_golden(g15, mask, one_sec):
    assert map_sha256(mask) == str(g15["mask_sha256"]) and map_sha256(one_sec) == str(g15["one_sec_sha256"])
    assert np.array_equal(mask.ravel()[::SAMPLE_STEP], g15["mask_sample"])
    assert np.array_equal(one_sec.ravel()[::SAMPLE_STEP], g15["one_sec_sample"])
