"""CPU: the NumPy yardstick of the evaluation table -- x_maps_amd.eval_table.combine_depth_maps / load_and_filter on files,
tests/eval_table_cases.py's table() on arrays, tests/eval_ref.py's evaluation_stats -- against golden G15, which the reference's
own combine_mc3d, load_and_filter and evaluation_stats produced (tests/golden/make_golden_eval_table.py; cv2.medianBlur was the
exact median of nine there: unpinned).  Maps bit for bit (by hash and by sample); counts equal; the quotients of counts equal as
doubles; margin, RMSE and avg_depth to rtol 1e-6, the repository's G8 tolerance (the reference sums in float32, the yardstick
exactly: they agree to about 1e-7).  tests/test_gpu_eval_table.py holds the device to the same golden and, at small shapes, to this
yardstick."""
import os

import numpy as np
import pytest

import eval_ref as E
import eval_table_cases as K


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_eval_table.npz"))


@pytest.fixture(scope="module")
def inputs():
    return K.g15_inputs()


def test_the_recipe_still_makes_the_goldens_inputs(g15, inputs):
    gt, est, _ = inputs
    assert K.inputs_sha256(gt, est) == str(g15["inputs_sha256"])
    assert (int(g15["min_depth"]), int(g15["max_depth"])) == (K.MIN_D, K.MAX_D)


def test_the_array_yardstick_equals_the_reference(g15, inputs):
    gt, est, _ = inputs
    assert K.inputs_sha256(gt, est) == str(g15["inputs_sha256"])
    tab = K.table(gt, est, one_sec=(K.G15_METHODS.index("mc3d"),))
    K.check_maps_against_golden(g15, tab["mask"], tab["one_sec_maps"][2])
    np.testing.assert_allclose(tab["avg_depth"], float(g15["avg_depth"]), rtol=1e-6, atol=0)
    K.check_cells_against_golden(g15, lambda r, s: tab["cells"][r][s])
    K.assert_clear_of_the_margin(tab)


def test_the_file_recipe_equals_the_reference(g15, inputs, tmp_path):
    """eval_table.combine_depth_maps and load_and_filter, the functions the per-pair path is made of"""
    from x_maps_amd import eval_table as T
    gt, est, _ = inputs
    assert K.inputs_sha256(gt, est) == str(g15["inputs_sha256"])

    def files(name, stack):
        os.makedirs(tmp_path / name)
        names = [str(tmp_path / name / f"scans{i:03d}.npy") for i in range(len(stack))]
        for f, a in zip(names, stack):
            np.save(f, a)
        return names
    gt_files = files("gt", gt)
    est_files = {name: files(name, e) for name, e in est.items()}
    mask, thresh, avg = T.combine_depth_maps(gt_files, K.MIN_D, K.MAX_D)
    one_sec, _, _ = T.combine_depth_maps(est_files["mc3d"], K.MIN_D, K.MAX_D)
    K.check_maps_against_golden(g15, mask, one_sec)
    np.testing.assert_allclose(avg, float(g15["avg_depth"]), rtol=1e-6, atol=0)
    np.testing.assert_allclose(thresh, float(g15["thresh"]), rtol=1e-6, atol=0)
    comb, avg2, _ = K.combine_arrays(gt)
    assert np.array_equal(comb, mask)
    np.testing.assert_allclose(avg2, avg, rtol=1e-6, atol=0)
    g = [T.load_and_filter(f, mask, K.MIN_D, K.MAX_D) for f in gt_files]

    def get(r, s):
        name = K.G15_ROWS[r]
        e = one_sec if name == "mc3d_1s" else T.load_and_filter(est_files[name][s], mask, K.MIN_D, K.MAX_D)
        return E.evaluation_stats(e, g[s])
    K.check_cells_against_golden(g15, get)
