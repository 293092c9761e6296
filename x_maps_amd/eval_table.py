"""The X-maps, "ESL (init)", "MC3D" and "MC3D (1 sec)" rows of the reference's Table 1, from files on disk
(python/eval/create_evaluation_table.py:57-62,84-180 and the ground-truth combination it borrows from python/eval/esl_utilities.py:153-175), for one sequence directory laid out as the
reference's evaluation leaves it:

    <seq>/scans_np/*.npy                   camera time surfaces (input of compute_depth_x_maps.py)
    <seq>/x_maps/depth_init/scansNNN.npy   X-maps depth per scan        (written by x_maps_amd / tools/run_esl_on_arrival.py)
    <seq>/esl/depth_init/scansNNN.npy      ESL-init depth per scan      (x_maps_amd.esl_init / tools/run_esl_on_arrival.py --esl-init)
    <seq>/mc3d/depth/scansNNN.npy          MC3D depth per scan          (x_maps_amd.mc3d / tools/run_esl_on_arrival.py --mc3d)
    <seq>/esl/depth_optim/scansNNN.npy     ESL's optimised depth before its filters (x_maps_amd.esl_optim /
                                           tools/run_esl_on_arrival.py --esl-optim)
    <seq>/esl/depth_optim_filtered/*.npy   the same behind cv2.bilateralFilter and the pylops TV denoiser = the table's ground
                                           truth (compute_depth_esl.py:243-247; x_maps_amd.esl_filter /
                                           tools/run_esl_on_arrival.py --esl-filter; when the directory is absent the row cannot
                                           be computed and the caller says so)

The metrics themselves run on the GPU (x_maps_amd.eval_metrics, pinned by golden G8); what is restated here is the file-level
recipe: the per-pixel mean of the filtered ground-truth scans, median-filtered 3 x 3 (cv2.medianBlur: unpinned against a cv2
run -- OpenCV is not in this image -- replicate border, exact median of nine), as the mask every map is filtered with."""
from __future__ import annotations

import glob
import os

import numpy as np

from .eval_metrics import evaluation_stats


def median_blur3(img: np.ndarray) -> np.ndarray:
    """cv2.medianBlur(img, 3) for a float32 image: median of the 3 x 3 neighbourhood, borders replicated"""
    p = np.pad(np.asarray(img, np.float32), 1, mode="edge")
    h, w = img.shape
    stack = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], 0)
    return np.partition(stack, 4, axis=0)[4]


def combine_depth_maps(depth_files, min_d, max_d):
    """esl_utilities.py:153-175 (combine_mc3d): mean over the scans of the depths inside (min_d, max_d), median-filtered;
    -> (combined, 1 % of the mean depth, mean depth)"""
    acc = count = None
    for f in depth_files:
        try:
            d = np.load(f).astype(np.float32)
        except Exception:  # (the reference skips unreadable files too)
            continue
        if acc is None:
            acc, count = np.zeros(d.shape, np.float32), np.zeros(d.shape, np.float32)
        d[d >= max_d] = 0
        d[d <= min_d] = 0
        acc += d
        count += d > 0
    if acc is None:
        raise ValueError("no readable depth map")
    with np.errstate(invalid="ignore", divide="ignore"):
        comb = acc / count
    comb[count == 0] = 0
    comb = median_blur3(comb)
    avg = float(comb[comb > 0].sum() / max(int((comb > 0).sum()), 1))
    return comb, 0.01 * avg, avg


def load_and_filter(filename, gt, min_depth, max_depth):
    """create_evaluation_table.py:57-62"""
    r = np.load(filename).astype(np.float32)
    r[r >= max_depth] = 0
    r[r <= min_depth] = 0
    r[gt == 0] = 0
    return r


def depth_table_row(seq_dir: str, est_subdir, files_key: str, min_depth: float = 20, max_depth: float = 120, device: int = 0) -> dict:
    """One row of the table: mean fill rate / RMSE of <seq>/<est_subdir>/*.npy against <seq>/esl/depth_optim_filtered, scan by
    scan (create_evaluation_table.py:121-180 runs the same lines for every method).  est_subdir: path components below <seq>;
    files_key: the name under which an error result reports how many estimate files were found."""
    gt_files = sorted(glob.glob(os.path.join(seq_dir, "esl", "depth_optim_filtered", "*.npy")))
    est_files = sorted(glob.glob(os.path.join(seq_dir, *est_subdir, "*.npy")))
    if not gt_files:
        return {"error": f"no ground truth under {os.path.join(seq_dir, 'esl', 'depth_optim_filtered')} (the reference's "
                         f"compute_depth_esl.py writes it: esl/depth_optim, which x_maps_amd.esl_optim computes, behind the bilateral "
                         f"and TV filters: x_maps_amd.esl_filter, tools/run_esl_on_arrival.py --esl-filter)", files_key: len(est_files)}
    if len(gt_files) != len(est_files):
        return {"error": "frames are missing", "gt_files": len(gt_files), files_key: len(est_files)}
    gt_combined, _, avg_depth = combine_depth_maps(gt_files, min_depth, max_depth)
    rows = []
    for g, x in zip(gt_files, est_files):
        gt = load_and_filter(g, gt_combined, min_depth, max_depth)
        est = load_and_filter(x, gt_combined, min_depth, max_depth)
        s = evaluation_stats(est, gt, device=device)
        rows.append((s.fillrate, s.rmse))
    fr, rmse = np.mean(np.array(rows, np.float64), axis=0)
    return {"scans": len(rows), "mean_depth": round(avg_depth, 3), "fill_rate": float(fr), "rmse": float(rmse),
            "table_cell": f"{round(float(fr), 2)} & {round(float(rmse), 2)}"}


def x_maps_table_row(seq_dir: str, min_depth: float = 20, max_depth: float = 120, device: int = 0) -> dict:
    """Mean fill rate / RMSE of <seq>/x_maps/depth_init against <seq>/esl/depth_optim_filtered, scan by scan
    (create_evaluation_table.py:121-160; its defaults are min 20 / max 120, eval/x-map-eval.sh:72 passes -max_depth 500)."""
    return depth_table_row(seq_dir, ("x_maps", "depth_init"), "x_maps_files", min_depth, max_depth, device)


def esl_init_table_row(seq_dir: str, min_depth: float = 20, max_depth: float = 120, device: int = 0) -> dict:
    """The "ESL (init)" row (create_evaluation_table.py:143-180): <seq>/esl/depth_init -- what x_maps_amd.esl_init /
    tools/run_esl_on_arrival.py --esl-init write -- against the same ground truth."""
    return depth_table_row(seq_dir, ("esl", "depth_init"), "esl_init_files", min_depth, max_depth, device)


def mc3d_table_rows(seq_dir: str, min_depth: float = 20, max_depth: float = 120, device: int = 0) -> dict:
    """The "MC3D" and "MC3D (1 sec)" rows (create_evaluation_table.py:126-161) -> {"mc3d": row, "mc3d_1s": row}.  "mc3d":
    <seq>/mc3d/depth -- what x_maps_amd.mc3d / tools/run_esl_on_arrival.py --mc3d write -- scan by scan, as every other method.
    "mc3d_1s": combine_depth_maps of ALL those files (:128), which is NOT passed through load_and_filter, scored against every
    filtered ground-truth scan (:151)."""
    row = depth_table_row(seq_dir, ("mc3d", "depth"), "mc3d_files", min_depth, max_depth, device)
    if "error" in row:
        return {"mc3d": row, "mc3d_1s": dict(row)}
    gt_files = sorted(glob.glob(os.path.join(seq_dir, "esl", "depth_optim_filtered", "*.npy")))
    est_files = sorted(glob.glob(os.path.join(seq_dir, "mc3d", "depth", "*.npy")))
    combined, _, _ = combine_depth_maps(est_files, min_depth, max_depth)
    gt_combined, _, avg_depth = combine_depth_maps(gt_files, min_depth, max_depth)
    rows = []
    for g in gt_files:
        s = evaluation_stats(combined, load_and_filter(g, gt_combined, min_depth, max_depth), device=device)
        rows.append((s.fillrate, s.rmse))
    fr, rmse = np.mean(np.array(rows, np.float64), axis=0)
    return {"mc3d": row,
            "mc3d_1s": {"scans": len(rows), "mean_depth": round(avg_depth, 3), "fill_rate": float(fr), "rmse": float(rmse),
                        "table_cell": f"{round(float(fr), 2)} & {round(float(rmse), 2)}"}}
