#!/usr/bin/env python3
"""What the offline evaluation caller pays per scan: 60 time surfaces of 640 x 480 at ~50 % fill on the camera-view C-1M tables,
  (a) one scan at a time through compute_depth_from_time_surface(fused=True): the surface is normalised and turned into x / y / t
      columns on the host, then the engine's frame kernels run (depth only: that route has no cloud);
  (b) the time-surface entry in groups of 1 / 8 / 60, depth only and depth + cloud -- from host arrays (the copies included: what
      the caller pays) and from device-resident buffers (XM_MEM_DEVICE + xm_sync: the launches alone).
Wall-clock medians over --reps repetitions after a warm-up, every repetition ending in a synchronisation; one JSON line at the end.
One GPU process; --time-limit seconds (SIGALRM) ends a run that hangs.  --only-new runs (b) once per variant and nothing else: the
run to put under `rocprofv3 --kernel-trace --stats` (a run of its own; profiles/time_surfaces.md has the figures)."""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surfaces(n, h, w, fill, dtype, seed=0):
    rng = np.random.default_rng(seed)
    s = (rng.random((n, h, w)) * 0.8 + 0.1).astype(dtype)
    s[rng.random(s.shape) >= fill] = 0
    return s


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.5)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--groups", default="1,8,60")
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--time-limit", type=int, default=300)
    a = ap.parse_args(argv)
    signal.alarm(a.time_limit)
    import torch  # (torch's HIP runtime first: see tests/conftest.py)
    if torch.cuda.is_available():
        torch.cuda.init()
    from x_maps_amd import _native as N
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    from x_maps_amd.eval_depth import compute_depth_from_time_surface
    from x_maps_amd.synthetic import C_1M, make_tables
    from x_maps_amd.x_maps_disparity import XMapsDisparity

    tb = make_tables(C_1M)
    rng = np.random.default_rng(1)
    tb["cam_mapx_f32"] = (tb["cam_mapx_i16"] + rng.uniform(-0.45, 0.45, tb["cam_mapx_i16"].shape)).astype(np.float32)
    tb["cam_mapy_f32"] = (tb["cam_mapy_i16"] + rng.uniform(-0.45, 0.45, tb["cam_mapy_i16"].shape)).astype(np.float32)
    tb["Q"] = np.array([[1, 0, 0, -880.0], [0, 1, 0, -660.0], [0, 0, 0, 1490.0], [0, 0, -7.7, 0]])
    h, w = C_1M.cam_h, C_1M.cam_w
    px = h * w
    surf = surfaces(a.scans, h, w, a.fill, np.dtype(a.dtype))
    maps = CamProjMaps(tb, camera_perspective=True, n_slots=2)
    eng, xd = maps.engine, XMapsDisparity(maps)
    groups = [int(g) for g in a.groups.split(",")]
    res = {"scans": a.scans, "shape": [h, w], "fill": a.fill, "dtype": a.dtype, "reps": a.reps, "per_scan_ms": {}}

    def put(name, fn, reps, warmup):
        med, lo, hi = median_ms(fn, reps, warmup)
        res["per_scan_ms"][name] = {"median": round(med / a.scans, 5), "min": round(lo / a.scans, 5), "max": round(hi / a.scans, 5)}
        print(name, res["per_scan_ms"][name], flush=True)

    # the two routes compute the same depth maps
    ref = [compute_depth_from_time_surface(maps, xd, surf[i], fused=True)[0] for i in range(min(4, a.scans))]
    new = eng.process_time_surfaces(surf[:len(ref)], want_cloud=True)
    assert all(np.array_equal(r, d) for r, (d, _, _) in zip(ref, new))
    res["inlier_share"] = round(sum(st.n_inliers for _, _, st in new) / max(1, sum(st.n_events for _, _, st in new)), 4)

    reps, warmup = (1, 0) if a.only_new else (a.reps, a.warmup)
    if not a.only_new:
        put("a_fused_per_scan_host_prepared", lambda: [compute_depth_from_time_surface(maps, xd, surf[i], fused=True) for i in range(a.scans)],
            reps, warmup)
    d_in = eng.to_device(surf)
    d_depth, d_cloud = eng.dev_alloc(a.scans * px * 4), eng.dev_alloc(a.scans * px * 12)
    tdt = N.XM_T_FLOAT32 if a.dtype == "float32" else N.XM_T_FLOAT64
    esz = surf.dtype.itemsize

    def device_groups(g, cloud):
        for g0 in range(0, a.scans, g):
            k = min(g, a.scans - g0)
            N.check(eng._lib.xm_process_time_surfaces(eng._h, C.c_void_p(d_in + g0 * px * esz), tdt, k, N.XM_MEM_DEVICE,
                                                      C.c_void_p(d_depth + g0 * px * 4),
                                                      C.c_void_p(d_cloud + g0 * px * 12) if cloud else None, None))
        eng.sync()

    for g in groups:
        for cloud in (False, True):
            tag = f"group{g}_{'depth_cloud' if cloud else 'depth'}"
            put("b_host_" + tag, lambda: [eng.process_time_surfaces(surf[g0:g0 + g], want_cloud=cloud) for g0 in range(0, a.scans, g)],
                reps, warmup)
            put("b_device_" + tag, lambda: device_groups(g, cloud), reps, warmup)
    for p in (d_in, d_depth, d_cloud):
        eng.dev_free(p)
    eng.close()
    # S2's algorithmic bytes per pixel: the surface read + the packed LUT entry + 4 B of depth (the X-map / depth-table gathers of
    # the events come on top; they are the same for every route)
    res["pixel_kernel_algorithmic_bytes_per_scan"] = px * (esz + 4 + 4)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
