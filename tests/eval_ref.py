"""Plain high-precision restatement of the reference's evaluation metrics (python/eval/create_evaluation_table.py:14-63: class
evaluation_stats, load_and_filter) -- the yardstick of xm_eval_stats (tests/test_gpu_eval_edges.py), itself pinned against the
reference's own outputs (golden G8) and the oracle (tests/test_eval_ref_cpu.py).

What the reference does element-wise on float32 maps is done in float32 here too, with NumPy: the comparisons of
load_and_filter, gt - est, its absolute value and its square.  What the reference sums -- in float32, pairwise -- is summed
exactly here: math.fsum over float64; the margin and the RMSE come from those sums.  The integer counts are returned next to the
six numbers of the reference, so that a caller can compare quotients of integers as integers.

sums="float32" swaps the two exact sums, and nothing else, for the reference's own (np.sum of the float32 selection, the margin
and the mean square formed from it with the reference's expressions): the form in which all six numbers can be held to the
reference's digit for digit, which pins every element-wise step and every mask that the exact form shares with it."""
import math

import numpy as np

COUNTS = ("n_gt_pos", "n_gt_zero", "n_close", "n_valid", "n1", "n5", "n10")
FLOATS = ("fillrate", "rmse", "perc_1", "perc_5", "perc_10", "margin")


def load_and_filter(result, gt, min_depth, max_depth):
    """:57-62 on a float32 map (the file is the caller's business); the bounds compare as float32, as NumPy compares a float32
    array with a Python number"""
    result = np.array(result, dtype=np.float32, copy=True)
    gt = np.asarray(gt, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        result[result >= np.float32(max_depth)] = 0
        result[result <= np.float32(min_depth)] = 0
    result[gt == 0] = 0
    return result


def abs_error(estimate, groundtruth):
    """|gt - est| in float32, zeroed where gt == 0 (:22-23, :37-38)"""
    gt, est = np.asarray(groundtruth, dtype=np.float32), np.asarray(estimate, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(gt - est)
    a[gt == 0] = 0
    return a


def _div(a, b):
    """a / b as NumPy divides: 0 / 0 = NaN, x / 0 = +-inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def evaluation_stats(estimate, groundtruth, sums="exact"):
    """-> dict of the six floats of class evaluation_stats (FLOATS) and the seven counts they are made of (COUNTS)"""
    assert sums in ("exact", "float32")
    gt, est = np.asarray(groundtruth, dtype=np.float32), np.asarray(estimate, dtype=np.float32)
    assert gt.ndim == 2 and gt.shape == est.shape
    px = gt.size
    gt_pos = gt > 0
    n_gt_pos, n_gt_zero = int(gt_pos.sum()), int((gt == 0).sum())
    with np.errstate(all="ignore"):
        if sums == "exact":
            margin = np.float64(_div(0.01 * math.fsum(gt[gt_pos].astype(np.float64).tolist()), n_gt_pos))  # :18
        else:
            margin = 0.01 * np.sum(gt[gt_pos]) / np.sum(gt_pos)  # :18 as it stands: a float32 sum
        a = abs_error(est, gt)
        n_close = int(((a.astype(np.float64) if sums == "exact" else a) < margin).sum())
        d = gt - est
        sq = d * d  # pow(float32 array, 2): a float32 product
        valid = gt_pos & (est > 0)
        n1, n5, n10 = (int((a > np.float32(v)).sum()) for v in (1, 5, 10))
        n_valid = int(valid.sum())
        if n_valid == 0:
            rmse = 0.0
        elif sums == "exact":
            rmse = math.sqrt(math.fsum(sq[valid].astype(np.float64).tolist()) / n_valid)  # :28-34
        else:
            rmse = float(np.sqrt(np.sum(sq[valid]) / np.sum(valid)))
    return {"fillrate": _div(n_close - n_gt_zero, px - n_gt_zero),  # :24-26
            "rmse": rmse, "perc_1": _div(100 * n1, px), "perc_5": _div(100 * n5, px), "perc_10": _div(100 * n10, px),  # :40-42
            "margin": float(margin), "n_gt_pos": n_gt_pos, "n_gt_zero": n_gt_zero, "n_close": n_close, "n_valid": n_valid,
            "n1": n1, "n5": n5, "n10": n10}
