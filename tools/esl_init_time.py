#!/usr/bin/env python3
"""Time the ESL-init entries on the ESL geometry (640 x 480 camera, 1080 x 1920 projector, 3240 x 5760 rectified frame).

    python tools/esl_init_time.py [--md profiles/esl_init.md] [--repeats 20] [--groups 1 32]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/esl_init.md.  The surfaces are
RENDERED from x_maps_amd/rig.py's ESL-like stand-in (the reference's calibration numbers, a piecewise-planar scene) -- the ESL
recordings are not available here, and the output says so.  What is timed, each after warm-up, as the median of --repeats calls
that end in a device synchronise (host clock around a synchronous call):
  * xm_esl_init_time_surfaces, groups of 1 and 32: device-resident (kernels + launches + the final synchronise) and from host
    memory (plus the copies in and out);
  * xm_process_time_surfaces (X-maps) on the same surfaces from host memory, for context;
  * xm_esl_init_stage_disparity on one rectified frame (a 149 MB image in, 37 MB out: the copies are inside the call);
  * the NumPy restatement (tests/esl_init_ref.py) on a crop of that frame, for context.
Counted from the shapes and the maps, not measured: window entries walked (candidate evaluations) and bytes touched."""
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

PAPER_MS = 18.99  # X-maps paper, Table 2: ESL-init in the authors' CUDA on an RTX 4090


def walked(surface, t):
    """(camera pixels searched, window entries walked) of one surface, from the maps"""
    r2c, c2r = t["rect_to_cam_map"], t["cam_to_rect_map"]
    rx, ry = r2c[..., 0].astype(np.int64), r2c[..., 1].astype(np.int64)
    ok = (rx >= 0) & (rx < t["rect_w"]) & (ry >= 0) & (ry < t["rect_h"])
    m = c2r[ry[ok], rx[ok]].astype(np.int64)
    ok2 = (m[:, 0] >= 0) & (m[:, 0] < t["cam_w"]) & (m[:, 1] >= 0) & (m[:, 1] < t["cam_h"])
    v = surface.astype(np.float64)
    lo = v[v != 0].min()
    live = v[m[ok2, 1], m[ok2, 0]] > lo
    c = rx[ok][ok2][live]
    win = np.clip(np.minimum(c + t["max_disp"], t["rect_w"]) - (c + t["min_disp"]), 0, None)
    return int(live.sum()), int(win.sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-x-maps", action="store_true", help="skip the X-maps context measurement")
    a = ap.parse_args(argv)
    clocks = clock_state()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    import esl_init_ref as R

    g6 = np.load(os.path.join(ROOT, "tests", "golden", "g6_esl_calib.npz"))
    cp = C.CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g6["camera_K"], rig.NEBRA_CAMERA_D.copy(), g6["projector_K"],
                                    np.zeros(5), g6["R"], g6["T"])
    t0 = time.perf_counter()
    t = build_esl_init_tables(cp)
    t_tables = time.perf_counter() - t0
    n_max = max(a.groups)
    surfaces = cycle(render_surfaces(cp, t, min(8, n_max)), n_max)
    px = cp.camera_width * cp.camera_height
    res = {"geometry": {"camera": [640, 480], "projector": [1080, 1920], "rectified": [3240, 5760]},
           "surfaces": "rendered from rig.py's ESL-like stand-in (float32 microsecond stamps); NOT the ESL recordings",
           "events_per_surface": int(np.count_nonzero(surfaces[0])), "clock_state": clocks, "repeats": a.repeats,
           "table_build_seconds_host": round(t_tables, 2), "paper_esl_init_ms_rtx4090": PAPER_MS, "fused": {}, "x_maps": {}}
    per = [walked(s, t) for s in surfaces[:min(8, n_max)]]
    with EslInit(t, device=a.device) as esl:
        for n in a.groups:
            grp = surfaces[:n]
            searched = sum(per[i % len(per)][0] for i in range(n))
            entries = sum(per[i % len(per)][1] for i in range(n))
            out = esl.depths_from_time_surfaces(grp)
            assert sum(st.n_searched for _, _, st in out) == searched, "the tool's count of searched pixels differs from the device's"
            d_in = torch.from_numpy(grp).cuda(a.device)
            d_depth = torch.empty(grp.shape, dtype=torch.float32, device=d_in.device)
            torch.cuda.synchronize()
            dev = timed(lambda: esl.time_surfaces_device(d_in.data_ptr(), np.float32, n, d_depth.data_ptr()), a.repeats)
            host = timed(lambda: esl.depths_from_time_surfaces(grp), a.repeats).host
            assert np.array_equal(d_depth.cpu().numpy(), np.stack([o[0] for o in out]))
            # bytes: the surface is read by the extrema pass and gathered (px * 4 each), the back map (px * 4), one forward-map
            # entry and one window per searched pixel, the depth map out
            compulsory = n * (px * 4 * 2 + px * 4 + px * 4) + searched * 4
            res["fused"][str(n)] = {
                "ms_per_call_device_resident": round(dev.host, 4), "ms_per_surface_device_resident": round(dev.host / n, 4),
                "min_max_ms_per_call": [round(dev.host_min, 4), round(dev.host_max, 4)],
                "ms_per_surface_from_host_memory": round(host / n, 4),
                "pixels_searched_per_surface": searched // n, "matched_per_surface": sum(st.n_matched for _, _, st in out) // n,
                "candidate_evaluations_per_surface": entries // n,
                "candidate_evaluations_per_second": round(entries / (dev.host * 1e-3), 0),
                "bytes_requested_by_the_windows": entries * 4, "bytes_tables_surfaces_and_outputs": compulsory}
        # the stage entry: one rectified frame
        v, _ = R.normalise(surfaces[0])
        cam_rect = R.remap_nearest_i16(v, t["cam_to_rect_map"])
        st_ms = timed(lambda: esl.disparity_init(cam_rect), max(3, a.repeats // 4), warmup=1).host
        disp = esl.disparity_init(cam_rect)
        live = cam_rect > 0
        cols = np.nonzero(live)[1]
        st_entries = int(np.clip(np.minimum(cols + 900, 3240) - (cols + 5), 0, None).sum())
        res["stage"] = {"ms_per_frame_with_its_host_copies": round(st_ms, 3), "bytes_copied_in": cam_rect.nbytes, "bytes_copied_out": disp.nbytes,
                        "pixels_searched": int(live.sum()), "matched": int(np.count_nonzero(disp)), "candidate_evaluations": st_entries}
        # NumPy restatement on a crop (6 rows around the busiest one)
        r0 = int(np.argmax(live.sum(1)))
        r0 = min(max(r0 - 3, 0), cam_rect.shape[0] - 6)
        crop_cam, crop_proj = cam_rect[r0:r0 + 6], t["proj_rect"][r0:r0 + 6]
        c0 = time.perf_counter()
        crop = R.disparity_init(crop_cam, crop_proj)
        dt = time.perf_counter() - c0
        assert np.array_equal(crop, disp[r0:r0 + 6]), "stage entry differs from the restatement on the crop"
        n_crop = int((crop_cam > 0).sum())
        res["numpy_restatement_crop"] = {"rows": [r0, r0 + 6], "pixels_searched": n_crop, "seconds": round(dt, 4),
                                         "us_per_searched_pixel": round(dt / max(n_crop, 1) * 1e6, 2)}
    if not a.no_x_maps:
        from x_maps_amd import XMapsEngine
        tb = C.build_eval_tables(cp, device=a.device)
        with XMapsEngine(tb, camera_perspective=True, device=a.device) as eng:
            for n in a.groups:
                grp = surfaces[:n]
                ms = timed(lambda: eng.process_time_surfaces(grp), a.repeats).host
                res["x_maps"][str(n)] = {"ms_per_surface_from_host_memory": round(ms / n, 4)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.md:
        with open(a.md, "w") as f:
            f.write(markdown(res))
    return res


def markdown(r) -> str:
    rows = []
    for n, v in r["fused"].items():
        xm = r["x_maps"].get(n, {}).get("ms_per_surface_from_host_memory", "not measured")
        rows.append(f"| {n} | {v['ms_per_surface_device_resident']} | {v['ms_per_call_device_resident']} ({v['min_max_ms_per_call'][0]} .. "
                    f"{v['min_max_ms_per_call'][1]}) | {v['ms_per_surface_from_host_memory']} | {xm} | {v['candidate_evaluations_per_second']:.3g} |")
    f1 = next(iter(r["fused"].values()))
    s, c = r["stage"], r["numpy_restatement_crop"]
    return f"""# ESL-init on the device: times on the ESL geometry

Written by `tools/esl_init_time.py` on an MI355X.  Camera 640 x 480, projector 1080 x 1920, rectified frame 3240 x 5760, windows
of 895 candidates.  **The surfaces are rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in ({r['events_per_surface']} events per
surface), not the ESL recordings.  Medians of {r['repeats']} synchronous calls after warm-up, host clock around a call that ends in a
device synchronise.  Clock state of the box, queried idle before the first launch: {r['clock_state']}.

## Fused entry (`xm_esl_init_time_surfaces`)

| group | ms / surface, device-resident | ms / call (min .. max) | ms / surface from host memory | X-maps (`xm_process_time_surfaces`) ms / surface from host memory | candidate evaluations / s |
|---|---|---|---|---|---|
{chr(10).join(rows)}

Per surface: {f1['pixels_searched_per_surface']} of 307200 camera pixels searched ({f1['matched_per_surface']} matched),
{f1['candidate_evaluations_per_surface']} window entries walked (counted from the maps, not measured) = {f1['bytes_requested_by_the_windows'] // int(next(iter(r['fused'])))}
bytes requested by the windows, nearly all of them cache hits; surfaces, maps and outputs are
{f1['bytes_tables_surfaces_and_outputs'] // int(next(iter(r['fused'])))} bytes.  A group of 1 is three launches and a synchronise:
its time is mostly that overhead.

Context, not a pass mark: the paper's Table 2 gives ESL-init **{r['paper_esl_init_ms_rtx4090']} ms** in the authors' CUDA on an RTX 4090 -- on the
real recordings and over the whole rectified frame, so the figures are not like for like.  The X-maps column is this build's
time-surface entry on the same surfaces in the same run.

## Stage entry (`xm_esl_init_stage_disparity`), one rectified frame

{s['ms_per_frame_with_its_host_copies']} ms per frame **including its host copies** ({s['bytes_copied_in']} bytes in, {s['bytes_copied_out']} out): {s['pixels_searched']}
pixels searched, {s['matched']} matched, {s['candidate_evaluations']} candidate evaluations.

## NumPy restatement, for context

`tests/esl_init_ref.py` on rows {c['rows'][0]}..{c['rows'][1]} of the same frame: {c['pixels_searched']} pixels in {c['seconds']} s =
{c['us_per_searched_pixel']} us per searched pixel (equal to the device's result on the crop).

Unpinned, as everywhere in this build: the int16 rounding of the remap tables against a cv2 run (DESIGN.md section 5).
"""


if __name__ == "__main__":
    main()
