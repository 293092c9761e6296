#!/usr/bin/env python3
"""Time ESL's depth optimisation on the device at the evaluation's size (640 x 480 camera, 1080 x 1920 projector, window 3).

    python tools/esl_optim_time.py [--md profiles/esl_optim.md] [--repeats 20] [--groups 8 32]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/esl_optim.md.  The surfaces are
RENDERED from x_maps_amd/rig.py's ESL-like stand-in (the reference's calibration numbers, a piecewise-planar scene) -- the ESL
recordings are not available here, and the output says so -- and their depth_init maps come from xm_esl_init_time_surfaces on the
device, as in the chained call of tools/run_esl_on_arrival.py --esl-optim.

What is timed, after warm-up, as the median of --repeats calls: xm_esl_optim_time_surfaces on device-resident buffers (the extrema
launch, the optimisation kernel, the statistics launch and the final synchronise), between two device events, with the host clock
around the same synchronous call beside it; then the same from host memory (plus the copies in and out).  Reported with the time:
optimised pixels, evaluations per optimised pixel and n_hit_limit from the device's statistics.  A sample of optimised pixels of the
first surface is compared with the scalar restatement (tests/esl_optim_ref.py) in every run.  There is no fallback: without a GPU
the tool stops."""
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

from _timing import clock_state, cycle, render_surfaces, timed  # noqa: E402

N_DISTINCT = 8
N_SAMPLE = 48


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--groups", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    clocks = clock_state()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    import esl_optim_ref as R
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    from x_maps_amd.esl_optim import EslOptim, build_esl_optim_tables

    g6 = np.load(os.path.join(ROOT, "tests", "golden", "g6_esl_calib.npz"))
    cp = C.CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g6["camera_K"], rig.NEBRA_CAMERA_D.copy(), g6["projector_K"],
                                    np.zeros(5), g6["R"], g6["T"])
    t0 = time.perf_counter()
    t_init, t_opt = build_esl_init_tables(cp), build_esl_optim_tables(cp)
    t_tables = time.perf_counter() - t0
    base = render_surfaces(cp, t_init, N_DISTINCT)
    px = cp.camera_width * cp.camera_height
    res = {"geometry": {"camera": [640, 480], "projector": [1080, 1920], "window_size": 3, "xatol": 1e-5, "max_iter": 500},
           "surfaces": "rendered from rig.py's ESL-like stand-in (float32 microsecond stamps); NOT the ESL recordings",
           "events_per_surface": int(np.count_nonzero(base[0])), "clock_state": clocks, "repeats": a.repeats,
           "table_build_seconds_host": round(t_tables, 2), "p1_03": t_opt["p1_03"], "groups": {}}
    dev = torch.device("cuda", a.device)
    with EslInit(t_init, device=a.device) as esl, EslOptim(t_opt, device=a.device) as opt:
        for n in a.groups:
            grp = cycle(base, n)
            d_in = torch.from_numpy(grp).to(dev)
            d_init = torch.empty(grp.shape, dtype=torch.float32, device=dev)
            d_out = torch.empty(grp.shape, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            esl.time_surfaces_device(d_in.data_ptr(), np.float32, n, d_init.data_ptr())
            init = d_init.cpu().numpy()
            out = opt.depths_from_time_surfaces(grp, init, want_nfev=True)
            st = [o[2] for o in out]
            n_opt, n_ev = sum(s.n_optimised for s in st), sum(s.n_evals for s in st)
            call = lambda: opt.time_surfaces_device(d_in.data_ptr(), np.float32, n, d_init.data_ptr(), d_out.data_ptr())
            ev = timed(call, a.repeats)
            host = timed(lambda: opt.depths_from_time_surfaces(grp, init), max(3, a.repeats // 4), warmup=1).host
            assert np.array_equal(d_out.cpu().numpy().view(np.uint32), np.stack([o[0] for o in out]).view(np.uint32))
            nfev0 = out[0][1]
            res["groups"][str(n)] = {
                "ms_per_call_device_resident": round(ev.ev, 4), "ms_per_surface_device_resident": round(ev.ev / n, 4),
                "min_max_ms_per_call": [round(ev.ev_min, 4), round(ev.ev_max, 4)], "ms_per_call_host_clock": round(ev.host, 4),
                "ms_per_surface_from_host_memory": round(host / n, 4),
                "depth_init_pixels_per_surface": int(np.count_nonzero(init > 0)) // n, "optimised_per_surface": n_opt // n,
                "evaluations_per_optimised_pixel": round(n_ev / max(n_opt, 1), 2), "max_evaluations_of_a_pixel": int(max(o[1].max() for o in out)),
                "n_hit_limit": sum(s.n_hit_limit for s in st), "n_bad_bounds": sum(s.n_bad_bounds for s in st),
                "evaluations_per_second": round(n_ev / (ev.ev * 1e-3), 0),
                "bytes_surfaces_depths_in_and_out": n * px * 4 * 4}
        # a sample of the first surface's optimised pixels against the scalar restatement
        cam, _ = R.normalise_and_fill(base[0])
        rr = R.Rig(t_opt["cam_K"], t_opt["cam_D"], t_opt["proj_K"], t_opt["proj_D"], t_opt["Rt"], t_opt["proj_surface"], t_opt["p1_03"])
        ys, xs = np.nonzero(nfev0)
        pick = np.linspace(0, len(ys) - 1, min(N_SAMPLE, len(ys))).astype(int) if len(ys) else []
        c0 = time.perf_counter()
        for k in pick:
            y, x = int(ys[k]), int(xs[k])
            d0 = init[0][y, x]
            diff = float(np.float64(d0 * d0) / np.float64(rr.p1_03))
            xf, nf, _, _ = R.minimize_bounded(R.make_cost(rr, cam, x, y), float(d0) - diff, float(d0) + diff)
            assert np.float32(xf) == out[0][0][y, x] and nf == nfev0[y, x], f"pixel ({x}, {y}) differs from the restatement"
        res["restatement_sample"] = {"pixels": len(pick), "seconds_scalar_python_on_this_host": round(time.perf_counter() - c0, 3)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    return res


def markdown(r) -> str:
    rows = [f"| {n} | {v['ms_per_surface_device_resident']} | {v['ms_per_call_device_resident']} ({v['min_max_ms_per_call'][0]} .. "
            f"{v['min_max_ms_per_call'][1]}) | {v['ms_per_call_host_clock']} | {v['ms_per_surface_from_host_memory']} | {v['optimised_per_surface']} | "
            f"{v['evaluations_per_optimised_pixel']} (max {v['max_evaluations_of_a_pixel']}) | {v['n_hit_limit']} | {v['n_bad_bounds']} | "
            f"{v['evaluations_per_second']:.3g} |" for n, v in r["groups"].items()]
    s = r["restatement_sample"]
    return f"""# ESL depth optimisation on the device: times at the evaluation's size

Written by `tools/esl_optim_time.py` on an MI355X.  Camera 640 x 480, projector 1080 x 1920, window 3, xatol 1e-5, at most 500
evaluations: the reference's values.  **The surfaces are rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in
({r['events_per_surface']} events per surface), not the ESL recordings, and their `depth_init` maps come from
`xm_esl_init_time_surfaces` on the device (P1[0,3] = {r['p1_03']:.2f}).  Medians of {r['repeats']} calls after warm-up, between two device
events around `xm_esl_optim_time_surfaces` on device-resident buffers (extrema launch, optimisation kernel, statistics launch and
the final synchronise), with the host clock around the same synchronous call beside it.  Clock state of the box, queried idle before
the first launch: {r['clock_state']}.

**Nothing was measured before this.**  The parent commit has no optimisation on the device; the reference's `depth_optimization`
is the "lengthy point-wise optimization" its README warns about (one scipy call per pixel from an interpreter loop), and this
repository holds no time of it on record.  So there is no time bar here: these are first numbers.

| group | ms / surface, device-resident | ms / call by events (min .. max) | ms / call by the host clock | ms / surface from host memory | optimised pixels / surface | evaluations / optimised pixel | n_hit_limit | n_bad_bounds | evaluations / s |
|---|---|---|---|---|---|---|---|---|---|
{chr(10).join(rows)}

The trip count of a pixel depends on its data (24 .. 32 evaluations on the small rigs of golden G13); a wave runs until its last
lane has converged, and lanes without a `depth_init` idle beside it.  Each evaluation is a few dozen float64 operations (four
divisions among them), nine gathered projector values and a nine-step `fma` chain; the projector surface (8.3 MB) stays in L2.
The compulsory traffic of a group -- surfaces and `depth_init` in, depth out -- is small beside that arithmetic, so no bandwidth
share is given.

{s['pixels']} optimised pixels of the first surface, spread over the image, equal the scalar restatement (`tests/esl_optim_ref.py`)
in depth and evaluation count; that interpreter restatement took {s['seconds_scalar_python_on_this_host']} s for them on the host of
the measurement (context only: it is test code, not the reference's scipy loop, which was not timed here).

Unpinned: `cv2.undistortPoints`, `cv2.Rodrigues`, `cv2.projectPoints` (DESIGN.md section 5).  The solver and the cost are pinned
against the reference's own `depth_optimization` on the installed scipy (golden G13).
"""


if __name__ == "__main__":
    main()
