#!/usr/bin/env python3
"""Generate tests/golden/g15_eval_table.npz by RUNNING THE REFERENCE'S OWN FUNCTIONS: esl_utilities.utils.combine_mc3d
(python/eval/esl_utilities.py:153-175) and create_evaluation_table.load_and_filter / evaluation_stats
(python/eval/create_evaluation_table.py:14-62), in the order of that script's per-sequence loop (:121-163).

Run only in the build container (needs /root/reference, which does not exist on the GPU box):
    python tests/golden/make_golden_eval_table.py
esl_utilities imports cv2 at its top, which is not installed offline; it is replaced by an in-process stub before the import (as
make_golden_mc3d.py does).  UNPINNED: the stub's cv2.medianBlur is the exact median of nine with replicated borders
(x_maps_amd.eval_table.median_blur3) -- no cv2 run stands behind it, as everywhere in this repository.  Nothing from
/root/reference is copied: the .npz holds hashes of the inputs and the outputs the reference produced for them -- data, not source.

combine_mc3d hard-codes 480 x 640, so that is the size: 4 scans, 3 methods and the MC3D 1-sec row.  The inputs come from the
seeded recipe in tests/eval_table_cases.py (they would compress to about 6 MB); the .npz stores their SHA-256, every cell's six
floats and seven counts, avg_depth, and the SHA-256 and every 97th pixel of both combined maps.  The script ASSERTS the case
conditions the fixture exists for -- see check_cases()."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_EVAL = "/root/reference/python/eval"
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_ref as E  # noqa: E402
import eval_table_cases as K  # noqa: E402

FLOATS = ("fillrate", "rmse", "perc_1", "perc_5", "perc_10", "margin")


def import_reference():
    from x_maps_amd.eval_table import median_blur3

    def median_blur(img, ksize):
        assert ksize == 3 and img.dtype == np.float32
        return median_blur3(img)
    cv2 = types.ModuleType("cv2")
    cv2.medianBlur = median_blur
    sys.modules["cv2"] = cv2
    for name in ("yaml", "matplotlib", "matplotlib.pyplot"):  # (imported at the top, used by neither function)
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            if name == "matplotlib":
                sys.modules[name].pyplot = None
    sys.path.insert(0, REF_EVAL)
    import create_evaluation_table
    from esl_utilities import utils
    return create_evaluation_table, utils


def counts(stats):
    """the seven integers behind the reference's six numbers, by its own expressions (:18, :22-25, :30, :37-42)"""
    gt, est = stats.groundtruth, stats.estimate
    diff = np.abs(gt - est)
    diff[gt == 0] = 0
    return [int(np.sum(gt > 0)), int(np.sum(gt == 0)), int(np.sum(diff < stats.margin)), int(np.sum((gt > 0) & (est > 0))),
            int(np.sum(diff > 1)), int(np.sum(diff > 5)), int(np.sum(diff > 10))]


def check_cases(gt, est, info, mask, mean, cells, filtered):
    """every case the fixture exists for, found in the inputs and the reference's outputs"""
    h, w = mask.shape
    for row, cs in zip(filtered, cells):
        for (e, g), c in zip(row, cs):
            a = E.abs_error(e, g).astype(np.float64)
            near = np.abs(a - c["margin"]) < 1e-3 * c["margin"]  # _assert_clear_of_the_margin of test_gpu_eval_edges.py
            assert not near.any(), (c["margin"], a[near][:5])
            assert 0 < c["n10"] < c["n5"] < c["n1"] < h * w and c["n_valid"] > 0 and 0 < c["n_gt_zero"] < h * w, c
    # pixels exactly at min_depth and max_depth, in the ground truth and in the estimates
    assert (gt == K.MIN_D).any() and (gt == K.MAX_D).any()
    assert any((e == K.MIN_D).any() for e in est.values()) and any((e == K.MAX_D).any() for e in est.values())
    # mask-zero pixels with non-zero 3 x 3 neighbours and the reverse; a pixel the median takes away and one it fills
    p = np.pad(mask, 1, mode="edge")
    nb = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 0)
    assert ((mask == 0) & (nb != 0).any(0)).any() and ((mask != 0) & (nb == 0).any(0)).any()
    assert mean[info["lone"]] > 0 and mask[info["lone"]] == 0 and mean[info["hole"]] == 0 and mask[info["hole"]] > 0
    c0, c1 = info["strip"]
    assert (mask[:, c0 + 1:c1 - 1] == 0).all() and (mask > 0).mean() > 0.8


def main():
    assert os.path.isdir(REF_EVAL), "needs /root/reference (build container only)"
    ref, utils = import_reference()
    gt, est, info = K.g15_inputs()
    S = len(gt)
    with tempfile.TemporaryDirectory() as tmp:
        def files(name, stack):
            os.makedirs(os.path.join(tmp, name))
            names = [os.path.join(tmp, name, f"scans{i:03d}.npy") for i in range(len(stack))]
            for f, a in zip(names, stack):
                np.save(f, a)
            return names
        gt_files = files("gt", gt)
        est_files = {name: files(name, e) for name, e in est.items()}
        # create_evaluation_table.py:128-129
        one_sec, _, _ = utils.combine_mc3d(est_files["mc3d"], S, K.MIN_D, K.MAX_D)
        mask, thresh, avg_depth = utils.combine_mc3d(gt_files, S, K.MIN_D, K.MAX_D)
        assert mask.dtype == np.float32 and one_sec.dtype == np.float32 and np.isfinite(mask).all() and np.isfinite(one_sec).all()
        results = np.zeros((len(K.G15_ROWS), S, 6), np.float64)
        cnts = np.zeros((len(K.G15_ROWS), S, 7), np.int64)
        cells = [[None] * S for _ in K.G15_ROWS]
        filtered = [[None] * S for _ in K.G15_ROWS]
        for s in range(S):  # :143-158
            g = ref.load_and_filter(gt_files[s], mask, K.MIN_D, K.MAX_D)
            for r, name in enumerate(K.G15_ROWS):
                e = one_sec if name == "mc3d_1s" else ref.load_and_filter(est_files[name][s], mask, K.MIN_D, K.MAX_D)
                st = ref.evaluation_stats(e, g)
                results[r, s] = [getattr(st, f) for f in FLOATS]
                cnts[r, s] = counts(st)
                cells[r][s] = dict(zip(E.COUNTS, cnts[r, s].tolist()), margin=float(st.margin))
                filtered[r][s] = (e, g)
    # the mean before the median, for the case conditions only (the reference does not return it)
    _, _, mean = K.combine_arrays(gt, K.MIN_D, K.MAX_D)
    check_cases(gt, est, info, mask, mean, cells, filtered)
    out = {"inputs_sha256": np.array(K.inputs_sha256(gt, est)), "rows": np.array(K.G15_ROWS), "floats": np.array(FLOATS),
           "counts_names": np.array(E.COUNTS), "results": results, "counts": cnts, "avg_depth": np.float64(avg_depth),
           "thresh": np.float64(thresh), "min_depth": np.int32(K.MIN_D), "max_depth": np.int32(K.MAX_D),
           "mask_sha256": np.array(K.map_sha256(mask)), "mask_sample": mask.ravel()[::K.SAMPLE_STEP].copy(),
           "one_sec_sha256": np.array(K.map_sha256(one_sec)), "one_sec_sample": one_sec.ravel()[::K.SAMPLE_STEP].copy(),
           "median": np.array("UNPINNED: cv2.medianBlur(., 3) was a stub, the exact median of nine with replicated borders")}
    path = os.path.join(HERE, "g15_eval_table.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes; avg_depth", float(avg_depth), "fill rates", results[:, :, 0].mean(1), "rmse", results[:, :, 1].mean(1))
    assert size < 300 * 1024


if __name__ == "__main__":
    main()
