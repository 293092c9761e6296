#!/usr/bin/env python3
"""Time the two filters behind ESL's depth optimisation on the device at the evaluation's size (640 x 480 maps).

    python tools/esl_filter_time.py [--md profiles/esl_filter.md] [--repeats 10] [--groups 8 32]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/esl_filter.md.  The maps are the
SEEDED SCENES of tests/esl_filter_cases.py at 640 x 480 (a slanted plane with a step, noise and 15 % zeros, as depth_optim looks)
-- the ESL recordings are not available here, and the output says so.

What is timed, after warm-up, as the median of --repeats calls: xm_esl_filter_maps on device-resident buffers between two device
events, with the host clock around the same synchronous call beside it; the same with XM_ESL_FILTER_NO_TV for stage 1's share; then
the whole call from host memory.  Reported with the time: kernel launches per call, outer iterations and lsqr iterations per surface
from the device's statistics.  One 96 x 80 scene is compared with the CPU restatement (tests/esl_filter_ref.py) in every run, and the
difference is written beside the CPU's own numpy-vs-fsum difference.  There is no fallback: without a GPU the tool stops."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import clock_state, cycle, timed  # noqa: E402

N_DISTINCT = 8
W, H = 640, 480


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--groups", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    clocks = clock_state()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    import esl_filter_cases as K
    import esl_filter_ref as R
    from x_maps_amd.esl_filter import NO_TV, EslFilter

    base = [K.scene(H, W, 180 + k) for k in range(N_DISTINCT)]
    res = {"geometry": {"map": [W, H], "d": 5, "sigma": [3, 3], "mu": 0.5, "lambda": [0.1, 0.1], "niter": [20, 10], "iter_lim": 5},
           "maps": "seeded scenes of tests/esl_filter_cases.py; NOT the ESL recordings", "clock_state": clocks, "repeats": a.repeats,
           "groups": {}}
    dev = torch.device("cuda", a.device)
    with EslFilter(W, H, device=a.device) as flt, EslFilter(W, H, device=a.device, flags=NO_TV) as bil:
        for n in a.groups:
            grp = cycle(base, n)
            d_in = torch.from_numpy(grp).to(dev)
            d_out = torch.empty(grp.shape, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            out = flt.filter_maps(grp, want_trips=True)
            st = [o[3] for o in out]
            ev = timed(lambda: flt.maps_device(d_in.data_ptr(), n, d_out.data_ptr()), a.repeats, warmup=2)
            launches = flt.last_launches()
            assert np.array_equal(d_out.cpu().numpy().view(np.uint64), np.stack([o[0] for o in out]).view(np.uint64))
            ev1 = timed(lambda: bil.maps_device(d_in.data_ptr(), n, d_out.data_ptr()), a.repeats, warmup=2)
            host = timed(lambda: flt.filter_maps(grp), max(3, a.repeats // 3), warmup=1).host
            res["groups"][str(n)] = {
                "ms_per_call_device_resident": round(ev.ev, 3), "ms_per_surface_device_resident": round(ev.ev / n, 4),
                "min_max_ms_per_call": [round(ev.ev_min, 3), round(ev.ev_max, 3)], "ms_per_call_host_clock": round(ev.host, 3),
                "ms_per_surface_from_host_memory": round(host / n, 4), "launches_per_call": launches,
                "us_per_launch": round(ev.ev * 1e3 / launches, 2),
                "ms_per_call_stage_1_alone": round(ev1.ev, 4), "stage_1_launches": bil.last_launches(),
                "stage_1_share_percent": round(100.0 * ev1.ev / ev.ev, 2),
                "outer_iterations_per_surface": round(float(np.mean([s.n_outer for s in st])), 2),
                "lsqr_calls_per_surface": round(float(np.mean([s.n_lsqr for s in st])), 1),
                "lsqr_iterations_per_surface": round(float(np.mean([s.sum_itn for s in st])), 1),
                "istop_counts": [int(sum(s.istop_count[i] for s in st)) for i in range(8)]}
    # one small scene against the restatement
    img = K.scene(96, 80, 143)
    with EslFilter(80, 96, device=a.device) as flt:
        got, _, trips, _ = flt.filter_maps(img, want_trips=True)[0]
    c0 = time.perf_counter()
    want, _, info = R.esl_filter(img)
    t_ref = time.perf_counter() - c0
    want_fsum, _, info_fsum = R.esl_filter(img, norm=R.norm_fsum)
    assert np.array_equal(trips, info["trips"]) and np.array_equal(trips, info_fsum["trips"]), "trip counts differ from the restatement"
    res["restatement_96x80"] = {"max_abs_gpu_minus_numpy_norms": float(np.abs(got - want).max()),
                                "max_abs_numpy_minus_fsum_norms_cpu": float(np.abs(want - want_fsum).max()),
                                "trips_equal": True, "decision_margin": info["margin"],
                                "seconds_numpy_restatement_on_this_host": round(t_ref, 2)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    return res


def markdown(r) -> str:
    rows = [f"| {n} | {v['ms_per_surface_device_resident']} | {v['ms_per_call_device_resident']} ({v['min_max_ms_per_call'][0]} .. "
            f"{v['min_max_ms_per_call'][1]}) | {v['ms_per_call_host_clock']} | {v['ms_per_surface_from_host_memory']} | {v['launches_per_call']} | "
            f"{v['us_per_launch']} | {v['ms_per_call_stage_1_alone']} ({v['stage_1_share_percent']} %) | {v['outer_iterations_per_surface']} | "
            f"{v['lsqr_calls_per_surface']} | {v['lsqr_iterations_per_surface']} |" for n, v in r["groups"].items()]
    s = r["restatement_96x80"]
    return f"""# ESL ground truth on the device: bilateral filter and TV denoiser, times at the evaluation's size

Written by `tools/esl_filter_time.py` on an MI355X.  Maps of 640 x 480; d = 5, sigmaColor = sigmaSpace = 3; mu = 0.5, lambda =
0.1, 0.1, 20 x 10 iterations, iter_lim 5, damp 1e-4: the reference's values.  **The maps are seeded scenes**
(`tests/esl_filter_cases.py`: a slanted plane with a step, noise, 15 % zeros), not `depth_optim` maps of the ESL recordings.
Medians of {r['repeats']} calls after warm-up, between two device events around `xm_esl_filter_maps` on device-resident buffers
(every launch of both stages and the final synchronise), with the host clock around the same synchronous call beside it.  Clock
state of the box, queried idle before the first launch: {r['clock_state']}.

**Nothing was measured before this.**  The parent commit has neither filter on the device; the reference runs
`cv2.bilateralFilter` and pylops' `SplitBregman` (200 scipy `lsqr` calls per map from an interpreter loop), and this repository
holds no time of either on record.  So there is no time bar here: these are first numbers.

| group | ms / surface, device-resident | ms / call by events (min .. max) | ms / call by the host clock | ms / surface from host memory | launches / call | us / launch | stage 1 alone, ms / call (share) | outer iterations / surface | lsqr calls / surface | lsqr iterations / surface |
|---|---|---|---|---|---|---|---|---|---|---|
{chr(10).join(rows)}

The schedule is fixed: 3 launches for stage 1, `2 * iter_lim + 4` = 14 per inner call (right-hand side, first `v`, five pairs of
`u` / `v` steps, the closing step, shrinkage), one to finish -- whatever the group and however early a surface stops; a stopped
surface's blocks return on reading its control record.  A launch moves a few vectors of the group once (each step reads and writes
3 to 11 float64 per pixel: a `u` step reads six and writes five, a `v` step reads five and writes one).  At this size the call is
bound by that memory traffic, not by the launches: the mean time per launch above -- which includes the launches that a stopped
lsqr turns into immediate returns, about half of the iteration pairs -- grows with the group and corresponds to several TB/s.

One 96 x 80 scene against the CPU restatement (`tests/esl_filter_ref.py`) in the same run: every trip count equal; max |gpu -
restatement with NumPy norms| = {s['max_abs_gpu_minus_numpy_norms']:.3e}; the CPU's own difference between NumPy norms and exactly
rounded (`math.fsum`) norms on that map = {s['max_abs_numpy_minus_fsum_norms_cpu']:.3e}; least decision margin {s['decision_margin']:.3e}.  The
device's tile-order sums are a third summation order; the GPU tests bound the difference by 1000 x the CPU's, floor 1e-12.  The
NumPy restatement took {s['seconds_numpy_restatement_on_this_host']} s for that map on the host of the measurement (context only: test code).

Unpinned: `cv2.bilateralFilter`; pylops' loop, stacking, stencil, threshold and float32 operator dtype (DESIGN.md section 5).
Pinned: the reference's own `denoise_tv` -- its call, the dims swap, every parameter -- on the installed scipy's `lsqr` (golden G14).
"""


if __name__ == "__main__":
    main()
