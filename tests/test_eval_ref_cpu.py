"""CPU: the high-precision restatement of the evaluation metrics (tests/eval_ref.py) against the outputs of the reference's own
class (golden G8) and against the oracle (O.evaluation_stats, the reference's arithmetic: float32 pairwise sums), with the
tolerances tests/test_oracle_golden.py uses for G8 (array_equal for load_and_filter, rtol 1e-12 / atol 0 for the six numbers, ==
for the empty estimate).  With the reference's own float32 sums (sums="float32") all six numbers meet them; with exact sums, the
form the GPU tests use, the counts are the same integers, their quotients meet them, and margin and RMSE lie within the
float32 sums' error.  Then the counts on a map small enough to count by hand, in both forms."""
import math
import os

import numpy as np
import pytest

import eval_ref as E
import xmaps_oracle as O


@pytest.fixture(scope="module")
def g8(golden_dir):
    return np.load(os.path.join(golden_dir, "g8_eval_metrics.npz"))


def _cases(g):
    lo, hi = float(g["min_depth"]), float(g["max_depth"])
    for k in "abc":
        gt = g[f"{k}_gt"]
        est = E.load_and_filter(g[f"{k}_est_raw"], gt, lo, hi)
        yield k, est, gt, dict(zip(E.FLOATS, g[f"{k}_res"])), O.evaluation_stats(O.load_and_filter(g[f"{k}_est_raw"], gt, lo, hi), gt)


def test_with_the_references_sums_all_six_numbers_match_g8_and_the_oracle(g8):
    """load_and_filter and, with sums="float32", every number of the class: the element-wise steps and the masks are the reference's"""
    for k, est, gt, want, orc in _cases(g8):
        assert est.dtype == np.float32 and np.array_equal(est, g8[f"{k}_est"])
        r = E.evaluation_stats(est, gt, sums="float32")
        for f in E.FLOATS:
            print(k, f, r[f], want[f], orc[f])
            np.testing.assert_allclose(r[f], want[f], rtol=1e-12, atol=0)
            np.testing.assert_allclose(r[f], orc[f], rtol=1e-12, atol=0)
    r = E.evaluation_stats(np.zeros_like(g8["a_gt"]), g8["a_gt"], sums="float32")
    assert r["rmse"] == 0 and r["n_valid"] == 0 and r["fillrate"] == g8["empty_res"][0]
    np.testing.assert_allclose([r[f] for f in E.FLOATS], g8["empty_res"], rtol=1e-12, atol=0)


def test_with_exact_sums_the_quotients_of_counts_match_g8_and_the_oracle(g8):
    """the form the GPU tests use: only the two sums differ, so the counts are the same integers and their quotients the same doubles"""
    for k, est, gt, want, orc in _cases(g8):
        r, r32 = E.evaluation_stats(est, gt), E.evaluation_stats(est, gt, sums="float32")
        assert {c: r[c] for c in E.COUNTS} == {c: r32[c] for c in E.COUNTS}
        for f in ("fillrate", "perc_1", "perc_5", "perc_10"):
            assert r[f] == r32[f]
            np.testing.assert_allclose(r[f], want[f], rtol=1e-12, atol=0)
            np.testing.assert_allclose(r[f], orc[f], rtol=1e-12, atol=0)
        # the counts the quotients are made of
        assert r["n_gt_pos"] + r["n_gt_zero"] == gt.size and r["n_gt_zero"] == int((gt == 0).sum())
        assert r["n10"] <= r["n5"] <= r["n1"] <= gt.size and 0 < r["n_valid"] <= r["n_gt_pos"] and r["n_close"] >= r["n_gt_zero"]
        assert r["perc_1"] == 100 * r["n1"] / gt.size and r["fillrate"] == (r["n_close"] - r["n_gt_zero"]) / (gt.size - r["n_gt_zero"])
    r = E.evaluation_stats(np.zeros_like(g8["a_gt"]), g8["a_gt"])
    assert r["rmse"] == 0 and r["n_valid"] == 0 and r["fillrate"] == g8["empty_res"][0]
    assert [r["perc_1"], r["perc_5"], r["perc_10"]] == g8["empty_res"][2:5].tolist()


def test_exact_margin_and_rmse_are_within_the_float32_sums_error_of_the_references(g8):
    """An exact sum cannot have the reference's digits: its margin and RMSE come from float32 sums (measured, (exact - G8) / G8:
    margin 2.7e-8, 3.2e-8, 6.3e-8 and RMSE 1.1e-8, 6.5e-9, 2.9e-8 for a, b, c).  What they can differ by: a pairwise float32 sum
    of N non-negative terms in blocks of 128 is within (127 + log2(N / 128) + 1) roundings of 2^-24 of the exact sum in the
    worst case (N <= 19 200 here: 136 roundings), the result is rounded to float32 once more, and the square root halves a
    relative error."""
    for k, est, gt, want, orc in _cases(g8):
        r = E.evaluation_stats(est, gt)
        bound = (127 + math.ceil(math.log2(gt.size / 128)) + 2) * 2.0 ** -24
        for f in ("margin", "rmse"):
            print(k, f, r[f], want[f], (r[f] - want[f]) / want[f], bound)
            assert 0 < abs(r[f] - want[f]) <= bound * want[f] and abs(r[f] - orc[f]) <= bound * orc[f], (k, f)


def test_counts_on_a_map_counted_by_hand():
    gt = np.array([[10, 10, 0, 20], [-0.0, 40, -5, 20]], np.float32)  # gt > 0: 10 10 20 40 20 -> margin 0.2
    est = np.array([[10.125, 11.5, 7, 0], [3, 29, 1, 20.25]], np.float32)
    r = E.evaluation_stats(est, gt)
    r32 = E.evaluation_stats(est, gt, sums="float32")
    assert all(r[c] == r32[c] for c in E.COUNTS) and r["rmse"] == r32["rmse"]  # (sums a float32 holds exactly)
    assert (r["n_gt_pos"], r["n_gt_zero"], r["n_valid"]) == (5, 2, 4) and r["margin"] == 0.01 * 100.0 / 5
    # |gt - est|, zeroed where gt == 0:  0.125 1.5 0 20 / 0 11 6 0.25
    assert (r["n_close"], r["n1"], r["n5"], r["n10"]) == (3, 4, 3, 2)
    assert r["fillrate"] == (3 - 2) / (8 - 2) and r["perc_5"] == 100 * 3 / 8
    assert r["rmse"] == math.sqrt((0.125 ** 2 + 1.5 ** 2 + 11 ** 2 + 0.25 ** 2) / 4)
    f = E.load_and_filter(est, gt, 3, 11.5)  # est <= 3 and est >= 11.5 go, and everything over gt == 0
    assert np.array_equal(f, np.array([[10.125, 0, 0, 0], [0, 0, 0, 0]], np.float32))
    # no ground truth at all: NaN margin, nothing is close, 0 / 0 and x / 0 as NumPy gives them
    r = E.evaluation_stats(est, np.zeros_like(gt))
    o = O.evaluation_stats(est, np.zeros_like(gt))
    assert math.isnan(r["margin"]) and r["n_close"] == 0 and r["fillrate"] == -math.inf and r["rmse"] == 0
    assert np.array_equal([r[k] for k in E.FLOATS], [o[k] for k in E.FLOATS], equal_nan=True)
