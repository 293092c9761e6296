#!/usr/bin/env python3
"""Time the evaluation table's scorer on a sequence the size of the reference's: 60 scans x 4 methods + one "1 sec" row, 480 x 640.

    python tools/eval_table_time.py [--md profiles/eval_table.md] [--repeats 10] [--scans 60]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/eval_table.md.  The maps are the
seeded recipe of tests/eval_table_cases.py (a smooth scene, holes, noisy estimates), not the ESL recordings, and the output says so;
the scorer's time does not depend on the values.

The parent process never opens the GPU: it runs the one step in a fresh child process under its own time limit (--step-timeout).
What the step times, after warm-up, as medians of --repeats runs that end in a device synchronise (host clock around synchronous
calls), file reading excluded everywhere:
  - xm_eval_table_score, one call, from device-resident stacks and from host stacks (the copies in included);
  - the per-pair path the one call replaces, over the same maps already in host memory: x_maps_amd.eval_table's recipe on arrays
    -- combine_depth_maps and load_and_filter in NumPy, one xm_eval_stats call per (scan, row) -- and, apart, those xm_eval_stats
    calls alone on maps filtered beforehand.
Every cell of the one call is compared with the per-pair path's before anything is timed.  Counted from the shapes, not measured:
the bytes the kernels stream."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import clock_state, timed  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # achievable streaming rate of an MI355X (8 TB/s peak)
H, W, METHODS, ONE_SEC = 480, 640, ("x_maps", "esl_init", "mc3d", "esl_optim"), ("mc3d",)
MIN_D, MAX_D = 20, 120


def host_timed(fn, repeats, warmup=1):
    fn_ms = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            fn_ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(fn_ms)), float(min(fn_ms)), float(max(fn_ms))


def step(n_scans, repeats, device):
    """one child process -> one JSON line"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    import eval_ref as E
    import eval_table_cases as K
    from x_maps_amd.eval_metrics import evaluation_stats
    from x_maps_amd.eval_table import EvalTable
    base_gt, base_est, _ = K.make_case((H, W), 6, len(METHODS), seed=60)  # six distinct scans, cycled
    pick = [i % 6 for i in range(n_scans)]
    gt = np.ascontiguousarray(base_gt[pick])
    est = {name: np.ascontiguousarray(base_est[m][pick]) for m, name in enumerate(METHODS)}
    rows = list(METHODS) + [f"{n}_1s" for n in ONE_SEC]

    def combine(maps):  # eval_table.combine_depth_maps on arrays
        return K.combine_arrays(maps, MIN_D, MAX_D)[0]

    def per_pair():
        """the recipe of depth_table_row / mc3d_table_rows, row by row: the mask is combined again for every row"""
        out = {}
        for name in rows:
            mask = combine(gt)
            one_sec = combine(est[name[:-3]]) if name.endswith("_1s") else None
            out[name] = [evaluation_stats(one_sec if one_sec is not None else E.load_and_filter(est[name][s], mask, MIN_D, MAX_D),
                                          E.load_and_filter(gt[s], mask, MIN_D, MAX_D), device=device) for s in range(n_scans)]
        return out

    with EvalTable(H, W, MIN_D, MAX_D, device=device) as t:
        score = t.score(gt, est, one_sec=ONE_SEC)
        want = per_pair()
        for r, name in enumerate(rows):  # the same table: counts equal, margin / RMSE to the last bits of a reordered sum
            for s in range(n_scans):
                got, w = score.results[r, s], want[name][s]
                assert (int(got["n_valid"]), int(got["n_gt_zero"])) == (w.n_valid, w.n_gt_zero), (name, s)
                assert got["fillrate"] == w.fillrate and got["perc_10"] == w.perc_10, (name, s, got, w)
                np.testing.assert_allclose([got["margin"], got["rmse"]], [w.margin, w.rmse], rtol=1e-9)
        d_gt = torch.from_numpy(gt).cuda(device)
        d_est = {n: torch.from_numpy(e).cuda(device) for n, e in est.items()}
        torch.cuda.synchronize()
        ptrs = {n: x.data_ptr() for n, x in d_est.items()}
        dev = timed(lambda: t.score_device(d_gt.data_ptr(), ptrs, n_scans, one_sec=ONE_SEC), repeats)
        again = t.score_device(d_gt.data_ptr(), ptrs, n_scans, one_sec=ONE_SEC)
        assert again.results.tobytes() == score.results.tobytes() and again.sums.tobytes() == score.sums.tobytes()
        host = host_timed(lambda: t.score(gt, est, one_sec=ONE_SEC), max(3, repeats // 2))
        mask = score.mask
    pairs = [(combine(est[name[:-3]]) if name.endswith("_1s") else E.load_and_filter(est[name][s], mask, MIN_D, MAX_D),
              E.load_and_filter(gt[s], mask, MIN_D, MAX_D)) for name in rows for s in range(n_scans)]
    calls = host_timed(lambda: [evaluation_stats(e, g, device=device) for e, g in pairs], max(3, repeats // 2))
    recipe = host_timed(per_pair, 2, warmup=0)
    px, M, G = H * W, len(METHODS), 1 + len(ONE_SEC)
    streamed = (G * n_scans + n_scans + (1 + M) * n_scans) * px * 4  # combine + pass 1 + pass 2 (the 1-sec map and the mask stay in cache)
    res = {"scans": n_scans, "rows": rows, "cells": len(rows) * n_scans,
           "one_call_device_resident_ms": round(dev.host, 4), "one_call_device_resident_min_max_ms": [round(dev.host_min, 4), round(dev.host_max, 4)],
           "one_call_device_events_ms": round(dev.ev, 4),
           "one_call_from_host_stacks_ms": round(host[0], 3), "one_call_from_host_stacks_min_max_ms": [round(host[1], 3), round(host[2], 3)],
           "per_pair_eval_stats_calls_only_ms": round(calls[0], 3), "per_pair_eval_stats_calls_only_min_max_ms": [round(calls[1], 3), round(calls[2], 3)],
           "per_pair_recipe_with_numpy_ms": round(recipe[0], 1),
           "bytes_streamed": streamed, "bytes_uploaded_from_host": (1 + M) * n_scans * px * 4,
           "streamed_bytes_per_second": round(streamed / (dev.host * 1e-3), 0),
           "share_of_copy_ceiling": round(streamed / HBM_BYTES_PER_S / (dev.host * 1e-3), 4),
           "checked": "every cell against the per-pair path before timing; the one call's bytes identical between runs and memories"}
    print("EVAL_TABLE_STEP " + json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step-timeout", type=float, default=400.0, help="seconds the step may take")
    ap.add_argument("--step", action="store_true", help=argparse.SUPPRESS)  # (internal: the step in this process)
    a = ap.parse_args(argv)
    if a.step:
        return step(a.scans, a.repeats, a.device)
    res = {"geometry": [H, W], "maps": "the seeded recipe of tests/eval_table_cases.py; NOT the ESL recordings", "clock_state": clock_state(),
           "repeats": a.repeats, "command": "python tools/eval_table_time.py " + " ".join(argv if argv is not None else sys.argv[1:])}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--scans", str(a.scans), "--repeats", str(a.repeats), "--device", str(a.device)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("EVAL_TABLE_STEP ")]
        if r.returncode != 0 or not line:
            res["error"] = {"exit_status": r.returncode, "stderr_tail": r.stderr[-2000:]}
        else:
            res["step"] = json.loads(line[-1][len("EVAL_TABLE_STEP "):])
    except subprocess.TimeoutExpired:
        res["error"] = f"no result within {a.step_timeout} s"
    print(json.dumps(res, indent=1))
    if a.md and "step" in res:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    return res


def markdown(r) -> str:
    s = r["step"]
    return f"""# The evaluation table on the device: times for one sequence

Written by `{r['command']}` on an MI355X.  {s['scans']} scans of {r['geometry'][0]} x {r['geometry'][1]}, the rows {', '.join(s['rows'])}:
{s['cells']} cells.  **The maps are {r['maps']}**; the scorer's time does not depend on the values.  Medians of synchronous calls
after warm-up, host clock around a call that ends in a device synchronise; the step runs in a process of its own.  File reading
is excluded on both sides.  Clock state of the box, queried idle before the first launch: {r['clock_state']}.

| what | ms (min .. max) |
|---|---|
| `xm_eval_table_score`, one call, stacks resident on the device | {s['one_call_device_resident_ms']} ({s['one_call_device_resident_min_max_ms'][0]} .. {s['one_call_device_resident_min_max_ms'][1]}); {s['one_call_device_events_ms']} between device events |
| the same call from host stacks ({s['bytes_uploaded_from_host'] / 1e6:.0f} MB copied in from pageable memory) | {s['one_call_from_host_stacks_ms']} ({s['one_call_from_host_stacks_min_max_ms'][0]} .. {s['one_call_from_host_stacks_min_max_ms'][1]}) |
| the per-pair path's {s['cells']} `xm_eval_stats` calls alone, maps filtered beforehand, in host memory | {s['per_pair_eval_stats_calls_only_ms']} ({s['per_pair_eval_stats_calls_only_min_max_ms'][0]} .. {s['per_pair_eval_stats_calls_only_min_max_ms'][1]}) |
| the per-pair recipe as `depth_table_row` / `mc3d_table_rows` run it on arrays (NumPy combine per row, NumPy filters, the same calls) | {s['per_pair_recipe_with_numpy_ms']} |

The bar is structural: from device-resident stacks the one call is not slower than the per-pair path's calls
({s['one_call_device_resident_ms']} ms against {s['per_pair_eval_stats_calls_only_ms']} ms).  Each of those calls allocates, uploads two maps, runs two
launches and synchronises; the one call is a fixed schedule of six launches.

Bytes the kernels stream, counted from the shapes (combine reads every stack it combines once, pass 1 the ground truth, pass 2
the ground truth and every method; the mask and the 1-sec map stay in cache): {s['bytes_streamed'] / 1e6:.0f} MB, that is
{s['streamed_bytes_per_second'] / 1e12:.3f} TB/s over the device-resident call's time, {100 * s['share_of_copy_ceiling']:.1f} % of the 6.3 TB/s a streaming
copy reaches on this part (8 TB/s peak).  This is a whole-call figure -- launches, the fold, the copy of the sums back and the
synchronise included -- not a kernel's share of peak.
The stacks are read about 1.6 times per call and calls are repeated back to back, so part of every read is served by the
256 MiB Infinity Cache: the rate is no HBM rate either.  No kernel trace was taken.

{s['checked']}.
"""


if __name__ == "__main__":
    main()
