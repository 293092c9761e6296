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
run -- OpenCV is not in this image -- replicate border, exact median of nine), as the mask every map is filtered with.

EvalTable / sequence_table (at the end) are the same table from ONE device call: combine, median, filters and the metrics of every
(method, scan) cell and of the "1 sec" rows on the GPU (xm_eval_table_*), with sums folded in a fixed order.  The functions above
them stay as the per-pair path and as the NumPy yardstick the tests hold that call to."""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np

from . import _native as N
from ._group import GroupObject, map_group, ptr as _ptr, stats_dtype
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


# ---- the same table from ONE device call (xm_eval_table_*; kernels in csrc/xmaps_evaltable.hpp, the contract in include/xmaps.h) ----

RESULT_DTYPE = stats_dtype(N.xm_eval_result)
SUMS_DTYPE = stats_dtype(N.xm_eval_sums)
MAX_METHODS = 8


class EvalTableScore:
    """What EvalTable.score returns.  rows: the row names (the methods as given, then "<name>_1s" for every 1-sec row, in the
    methods' order); results / sums: structured arrays [rows][scans] of xm_eval_result / xm_eval_sums; mask: the combined
    ground truth (None from score_device); avg_depth: its mean depth."""
    __slots__ = ("rows", "results", "sums", "mask", "avg_depth")

    def __init__(self, rows, results, sums, mask, avg_depth):
        self.rows, self.results, self.sums, self.mask, self.avg_depth = rows, results, sums, mask, avg_depth

    def row(self, name):
        """the [scans] results of one row"""
        return self.results[self.rows.index(name)]

    def mean_fill_rate_and_rmse(self, name):
        """create_evaluation_table.py:160-163: np.mean(np.array(rows), axis=0) over the scans"""
        r = self.row(name)
        fr, rmse = np.mean(np.array(list(zip(r["fillrate"], r["rmse"])), np.float64), axis=0)
        return float(fr), float(rmse)


class EvalTable(GroupObject):
    """with EvalTable(height, width, min_depth, max_depth) as t: score = t.score(gt_maps, {"x_maps": maps, "mc3d": maps}, one_sec=("mc3d",))

    combine_depth_maps, load_and_filter and evaluation_stats of every (method, scan) pair -- and of the "1 sec" rows, whose
    estimate is a method's combined map -- in one device call; no NumPy arithmetic, the same bits every run."""
    _destroy = "xm_eval_table_destroy"

    def __init__(self, height: int, width: int, min_depth: float = 20, max_depth: float = 120, device: int = 0):
        self.height, self.width = int(height), int(width)
        cfg = N.xm_eval_table_config(C.sizeof(N.xm_eval_table_config), self.height, self.width, float(min_depth), float(max_depth), 0)
        self._create("xm_eval_table_create", device, cfg)

    def combine(self, maps, want_mean: bool = False):
        """combine_depth_maps on the device -> (combined, avg_depth[, the mean before the median])"""
        grp = map_group(maps, self.height, self.width, np.float32)
        comb = np.empty((self.height, self.width), np.float32)
        mean = np.empty((self.height, self.width), np.float32) if want_mean else None
        avg = C.c_double()
        N.check(self._lib.xm_eval_table_combine(self._h, _ptr(grp), grp.shape[0], N.XM_MEM_HOST, _ptr(comb), _ptr(mean), C.byref(avg)))
        return (comb, avg.value, mean) if want_mean else (comb, avg.value)

    @staticmethod
    def _rows(names, one_sec):
        names = list(names)
        unknown = [n for n in one_sec if n not in names]
        if unknown:
            raise ValueError(f"one_sec names no method: {unknown}")
        bits = sum(1 << i for i, n in enumerate(names) if n in one_sec)
        return names + [f"{n}_1s" for n in names if n in one_sec], bits

    def _call(self, gt_ptr, est_ptrs, n_scans, bits, n_rows, mem, mask_ptr):
        results = np.zeros((n_rows, n_scans), RESULT_DTYPE)
        sums = np.zeros((n_rows, n_scans), SUMS_DTYPE)
        avg = C.c_double()
        est = (C.c_void_p * len(est_ptrs))(*est_ptrs)
        N.check(self._lib.xm_eval_table_score(self._h, gt_ptr, est, len(est_ptrs), bits, int(n_scans), mem, _ptr(results), _ptr(sums),
                                              mask_ptr, C.byref(avg)))
        return results, sums, avg.value

    def score(self, gt, methods: dict, one_sec=()) -> EvalTableScore:
        """gt: the ground-truth scans (a list of [height][width] maps or one 3-D array); methods: {name: the estimates, scan by scan};
        one_sec: the names of the methods that also get a "1 sec" row"""
        g = map_group(gt, self.height, self.width, np.float32, "ground-truth maps")
        stacks = [map_group(m, self.height, self.width, np.float32, f"{name} maps") for name, m in methods.items()]
        for name, s in zip(methods, stacks):
            if s.shape[0] != g.shape[0]:
                raise ValueError(f"{name}: {s.shape[0]} maps for {g.shape[0]} ground-truth scans")
        rows, bits = self._rows(methods, tuple(one_sec))
        mask = np.empty((self.height, self.width), np.float32)
        results, sums, avg = self._call(_ptr(g), [s.ctypes.data for s in stacks], g.shape[0], bits, len(rows), N.XM_MEM_HOST, _ptr(mask))
        return EvalTableScore(rows, results, sums, mask, avg)

    def score_device(self, gt_ptr, est_ptrs: dict, n_scans: int, one_sec=(), mask_ptr=None) -> EvalTableScore:
        """the same on device memory of this object's device (raw pointers to [n_scans][height][width] float32; synchronous)"""
        rows, bits = self._rows(est_ptrs, tuple(one_sec))
        results, sums, avg = self._call(gt_ptr, [int(p) for p in est_ptrs.values()], n_scans, bits, len(rows), N.XM_MEM_DEVICE, mask_ptr)
        return EvalTableScore(rows, results, sums, None, avg)


SEQUENCE_METHODS = (("x_maps", ("x_maps", "depth_init"), "x_maps_files"), ("esl_init", ("esl", "depth_init"), "esl_init_files"),
                    ("mc3d", ("mc3d", "depth"), "mc3d_files"))


def sequence_table(seq_dir: str, min_depth: float = 20, max_depth: float = 120, device: int = 0) -> dict:
    """x_maps_table_row, esl_init_table_row and mc3d_table_rows of one sequence directory from ONE device call: every file of the
    four directories is read once, nothing is combined or filtered in NumPy.  -> {"x_maps": row, "esl_init": row, "mc3d": row,
    "mc3d_1s": row}, the rows shaped like depth_table_row's (a method whose files are missing gets that function's error row)."""
    gt_files = sorted(glob.glob(os.path.join(seq_dir, "esl", "depth_optim_filtered", "*.npy")))
    out, stacks = {}, {}
    for name, sub, files_key in SEQUENCE_METHODS:
        est_files = sorted(glob.glob(os.path.join(seq_dir, *sub, "*.npy")))
        if not gt_files:
            out[name] = {"error": f"no ground truth under {os.path.join(seq_dir, 'esl', 'depth_optim_filtered')} (the reference's "
                                  f"compute_depth_esl.py writes it: esl/depth_optim, which x_maps_amd.esl_optim computes, behind the bilateral "
                                  f"and TV filters: x_maps_amd.esl_filter, tools/run_esl_on_arrival.py --esl-filter)", files_key: len(est_files)}
        elif len(gt_files) != len(est_files):
            out[name] = {"error": "frames are missing", "gt_files": len(gt_files), files_key: len(est_files)}
        else:
            stacks[name] = [np.load(f).astype(np.float32, copy=False) for f in est_files]
    if stacks:
        gt = [np.load(f).astype(np.float32, copy=False) for f in gt_files]
        h, w = gt[0].shape
        with EvalTable(h, w, min_depth, max_depth, device=device) as table:
            score = table.score(gt, stacks, one_sec=("mc3d",) if "mc3d" in stacks else ())
        for name in score.rows:
            fr, rmse = score.mean_fill_rate_and_rmse(name)
            out[name] = {"scans": len(gt), "mean_depth": round(score.avg_depth, 3), "fill_rate": fr, "rmse": rmse,
                         "table_cell": f"{round(fr, 2)} & {round(rmse, 2)}"}
    if "mc3d_1s" not in out:
        out["mc3d_1s"] = dict(out["mc3d"])
    return {k: out[k] for k in ("x_maps", "esl_init", "mc3d", "mc3d_1s")}
