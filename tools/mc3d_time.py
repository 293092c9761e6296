#!/usr/bin/env python3
"""Time the MC3D entry on the ESL geometry (640 x 480 camera, 1080 x 1920 projector, windows of 256 projector rows).

    python tools/mc3d_time.py [--md profiles/mc3d.md] [--repeats 20] [--groups 1 8 32] [--also-lib NAME=PATH ...]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/mc3d.md.  The surfaces are RENDERED
from x_maps_amd/rig.py's ESL-like stand-in (the reference's calibration numbers, a piecewise-planar scene): a lit camera pixel
holds (proj_x * H + proj_y + 0.5) / (W * H) of the projector pixel that lit it, MC3D's own convention -- the ESL recordings are
not available here, and the output says so.

The parent process never opens the GPU: it builds the tables and the surfaces once, then runs every step -- one group size on one
build of the library -- in a fresh child process under its own time limit (--step-timeout), and starts no further step after one
that failed or ran out of time.  --also-lib times another build of the library (XM_LIB, e.g. one built with -DXM_MC3D_LANE_WALK)
on the same surfaces for the comparison of kernel shapes.  What a step times, after warm-up, as the median of --repeats calls that
end in a device synchronise (host clock around a synchronous call): xm_mc3d_time_surfaces device-resident (two launches and the
final synchronise) and from host memory (plus the copies in and out).  Counted from the shapes and the maps, not measured: window
entries walked and bytes."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from _timing import clock_state, cycle, timed  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured streaming rate of an MI355X (float4 copy)
L2_BYTES_PER_S = 34.5e12   # aggregate L2 rate of its eight XCDs
N_DISTINCT = 8
TRIED = "## What was tried\n"


def make_inputs(path):
    """tables and N_DISTINCT rendered surfaces -> an .npz the steps load (host work only)"""
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    from x_maps_amd.mc3d import build_mc3d_tables
    g6 = np.load(os.path.join(ROOT, "tests", "golden", "g6_esl_calib.npz"))
    cp = C.CamProjCalibrationParams(640, 480, 1080, 1920, 3240, 5760, g6["camera_K"], rig.NEBRA_CAMERA_D.copy(), g6["projector_K"],
                                    g6["projector_D"], g6["R"], g6["T"])
    t0 = time.perf_counter()
    t = build_mc3d_tables(cp)
    t_tables = time.perf_counter() - t0
    W, H = cp.projector_width, cp.projector_height
    surfaces = []
    for k in range(N_DISTINCT):
        evs, gt = rig.render_events(cp, t, row_stride=1, scan_upwards=False, seed=k)
        s = np.zeros((cp.camera_height, cp.camera_width), np.float32)
        s[evs["y"], evs["x"]] = ((gt["proj_u"] * H + gt["proj_v"] + 0.5) / (W * H)).astype(np.float32)  # (the last event of a pixel stays)
        surfaces.append(s)
    np.savez(path, cam_map=t["cam_map"], proj_map=t["proj_map"], p1_03=t["p1_03"], surfaces=np.stack(surfaces), t_tables=t_tables)


def walked(surface, cam_map, proj_h=1920, proj_w=1080, nc=128):
    """(pixels searched, window entries walked) of one surface, from the maps"""
    import mc3d_ref as R
    v = R.median_blur3(surface)
    xc, yc = cam_map[..., 0], cam_map[..., 1]
    wh = np.float32(proj_w * proj_h)
    ok = (v > 0) & (xc > 0) & (xc < 3 * proj_h) & (yc > 0) & (yc < 3 * proj_w) & (wh * v < wh)
    row = (wh * v[ok]).astype(np.int64) % proj_h
    return int(ok.sum()), int((np.minimum(row + nc, proj_h) - np.maximum(row - nc, 0)).sum())


def step(inputs, n, repeats, device):
    """one child process: group size n on whatever library XM_LIB names -> one JSON line"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    import mc3d_ref as R
    from x_maps_amd.mc3d import Mc3d
    d = np.load(inputs)
    cam_map, proj_map, p1_03 = d["cam_map"], d["proj_map"], float(d["p1_03"])
    base = d["surfaces"]
    grp = cycle(base, n)
    per = [walked(s, cam_map) for s in base[:min(n, len(base))]]
    searched = sum(per[i % len(per)][0] for i in range(n))
    entries = sum(per[i % len(per)][1] for i in range(n))
    tables = {"cam_w": 640, "cam_h": 480, "proj_w": 1080, "proj_h": 1920, "cam_map": cam_map, "proj_map": proj_map, "p1_03": p1_03}
    with Mc3d(tables, device=device) as mc:
        out = mc.depths_from_time_surfaces(grp, want_disparity=True)
        got = sum(st.n_in_rect - st.n_out_of_range for _, _, st in out)
        assert got == searched, f"the tool's count of searched pixels ({searched}) differs from the device's ({got})"
        # a band of rows of the first surface against the NumPy restatement (its first and last row see other neighbours: left out)
        r0 = int(np.argmax((grp[0] > 0).sum(1)))
        r0 = min(max(r0 - 4, 0), 480 - 8)
        w_depth, w_disp, _ = R.mc3d(grp[0][r0:r0 + 8], cam_map[r0:r0 + 8], proj_map, p1_03)
        assert np.array_equal(out[0][1][r0 + 1:r0 + 7], w_disp[1:7]) and np.array_equal(out[0][0][r0 + 1:r0 + 7], w_depth[1:7]), \
            "the entry differs from the restatement on the band"
        d_in = torch.from_numpy(grp).cuda(device)
        d_depth = torch.empty(grp.shape, dtype=torch.float32, device=d_in.device)
        torch.cuda.synchronize()
        dev = timed(lambda: mc.time_surfaces_device(d_in.data_ptr(), np.float32, n, d_depth.data_ptr()), repeats)
        host = timed(lambda: mc.depths_from_time_surfaces(grp), repeats).host
        assert np.array_equal(d_depth.cpu().numpy(), np.stack([o[0] for o in out]))
    px = 640 * 480
    positive = sum(st.n_positive for _, _, st in out)
    # bytes that must move per group: every surface in, every depth map out, a camera entry per positive pixel; the projector
    # table (8.3 MB of yp, read many times over) once
    compulsory = n * px * 4 * 2 + positive * 8 + 1080 * 1920 * 4
    res = {"n": n, "ms_per_call_device_resident": round(dev.host, 4), "ms_per_surface_device_resident": round(dev.host / n, 4),
           "min_max_ms_per_call": [round(dev.host_min, 4), round(dev.host_max, 4)], "ms_per_surface_from_host_memory": round(host / n, 4),
           "lit_per_surface": int(sum((s != 0).sum() for s in grp)) // n, "positive_after_blur_per_surface": positive // n,
           "pixels_searched_per_surface": searched // n, "matched_per_surface": sum(st.n_matched for _, _, st in out) // n,
           "poisoned_per_surface": sum(st.n_poisoned for _, _, st in out) // n,
           "window_entries_per_surface": entries // n, "window_entries_per_second": round(entries / (dev.host * 1e-3), 0),
           "window_bytes_per_second_over_L2_rate": round(entries * 4 / (dev.host * 1e-3) / L2_BYTES_PER_S, 4),
           "compulsory_bytes_per_group": compulsory,
           "hbm_roofline_share": round(compulsory / HBM_BYTES_PER_S / (dev.host * 1e-3), 4),
           "band_checked_against_restatement": [r0 + 1, r0 + 7]}
    print("MC3D_STEP " + json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step (one group size on one library) may take")
    ap.add_argument("--also-lib", action="append", default=[], metavar="NAME=PATH", help="time this build of the library as well")
    ap.add_argument("--step", nargs=2, metavar=("INPUTS", "N"), help=argparse.SUPPRESS)  # (internal: one step in this process)
    a = ap.parse_args(argv)
    if a.step:
        return step(a.step[0], int(a.step[1]), a.repeats, a.device)
    libs = [("default", None)] + [tuple(s.split("=", 1)) for s in a.also_lib]
    res = {"geometry": {"camera": [640, 480], "projector": [1080, 1920], "window": 256},
           "surfaces": "rendered from rig.py's ESL-like stand-in; NOT the ESL recordings", "clock_state": clock_state(),
           "repeats": a.repeats, "libs": {name: {} for name, _ in libs}}
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "mc3d_inputs.npz")
        make_inputs(inputs)
        res["table_build_seconds_host"] = round(float(np.load(inputs)["t_tables"]), 2)
        ok = True
        for n in a.groups:
            for name, path in libs:
                if not ok:
                    break
                env = dict(os.environ)
                env.pop("XM_LIB", None)
                if path:
                    env["XM_LIB"] = os.path.abspath(path)
                cmd = [sys.executable, os.path.abspath(__file__), "--step", inputs, str(n), "--repeats", str(a.repeats), "--device", str(a.device)]
                try:
                    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.step_timeout)
                except subprocess.TimeoutExpired:
                    res["libs"][name][str(n)] = {"error": f"no result within {a.step_timeout} s"}
                    ok = False
                    break
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("MC3D_STEP ")]
                if r.returncode != 0 or not line:
                    res["libs"][name][str(n)] = {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}
                    ok = False
                    break
                res["libs"][name][str(n)] = json.loads(line[-1][len("MC3D_STEP "):])
        res["complete"] = ok
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.md and ok:
        notes = ""
        if os.path.exists(a.md):  # the hand-written section of an earlier profile stays
            old = open(a.md).read()
            if TRIED in old:
                notes = old.split(TRIED, 1)[1].split("\nUnpinned: ", 1)[0]
        with open(a.md, "w") as f:
            f.write(markdown(res, notes))
    return res


def esl_init_lines() -> str:
    """the fused entry's rows of profiles/esl_init.md, quoted"""
    try:
        rows = [ln.strip() for ln in open(os.path.join(ROOT, "profiles", "esl_init.md")) if ln.startswith("| 1 |") or ln.startswith("| 32 |")]
    except OSError:
        rows = []
    return "\n".join(rows) if rows else "(profiles/esl_init.md not found)"


def markdown(r, notes="") -> str:
    out = []
    for name, steps in r["libs"].items():
        rows = [f"| {n} | {v['ms_per_surface_device_resident']} | {v['ms_per_call_device_resident']} ({v['min_max_ms_per_call'][0]} .. "
                f"{v['min_max_ms_per_call'][1]}) | {v['ms_per_surface_from_host_memory']} | {v['window_entries_per_second']:.3g} | "
                f"{v['window_bytes_per_second_over_L2_rate']} | {v['hbm_roofline_share']} |" for n, v in steps.items()]
        out.append(f"### Library build `{name}`\n\n| group | ms / surface, device-resident | ms / call (min .. max) | ms / surface from host memory | "
                   f"window entries / s | window bytes / s over the L2's 34.5 TB/s | HBM roofline share |\n|---|---|---|---|---|---|---|\n" + "\n".join(rows))
    f1 = next(iter(next(iter(r["libs"].values())).values()))
    return f"""# MC3D on the device: times on the ESL geometry

Written by `tools/mc3d_time.py` on an MI355X.  Camera 640 x 480, projector 1080 x 1920, windows of 256 projector rows, the
reference's limits.  **The surfaces are rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in (a lit pixel holds the id of the
projector pixel that lit it, MC3D's convention), not the ESL recordings.  Medians of {r['repeats']} synchronous calls after warm-up,
host clock around a call that ends in a device synchronise; every step (one group size, one build) in a process of its own.
Clock state of the box, queried idle before the first launch: {r['clock_state']}.

**Nothing was measured before this.**  The parent commit has no MC3D, the reference's `mc3d_baseline.py` is an interpreter
loop that takes minutes per scan (`eval/x-map-eval.sh` fans it out under GNU parallel), and this repository holds no MC3D time on
record.  So there is no time bar here: these are first numbers.

## The entry (`xm_mc3d_time_surfaces`)

{(chr(10) + chr(10)).join(out)}

Per surface: {f1['lit_per_surface']} of 307200 camera pixels lit, {f1['positive_after_blur_per_surface']} positive after the median,
{f1['pixels_searched_per_surface']} searched ({f1['matched_per_surface']} matched, {f1['poisoned_per_surface']} poisoned),
{f1['window_entries_per_surface']} window entries walked (counted from the maps, not measured) = {f1['window_entries_per_surface'] * 4}
bytes requested by the windows.  A group of 1 is two launches, a synchronise and the walk of the busiest wave, one window
after the other: it says little about throughput.

The HBM roofline share is (bytes that must move: every surface in, every depth map out, a camera entry per positive pixel, the
8.3 MB table of projector rows once) / 6.29 TB/s over the measured time of the call.  It is small by construction: the work is
the window walk, whose loads hit the caches (the whole table fits the L2s), so the column beside it -- bytes the windows request
per second over the L2's aggregate rate -- is the one that says how busy the memory side is.  A band of rows of the first
surface is compared with `tests/mc3d_ref.py` in every step.

ESL-init on the same geometry, for context (`profiles/esl_init.md`, fused entry; group | ms / surface device-resident | ms / call
| from host memory | X-maps | candidate evaluations / s):

{esl_init_lines()}

{TRIED}
{notes.strip() or "(written by hand below this heading; kept when the tool rewrites the file)"}

Unpinned: `cv2.medianBlur(., 3)` (the exact median of nine stands in) and the float maps of `cv2.undistortPoints` (DESIGN.md
section 5).  The search is pinned against the reference's own `compute_disparity` (golden G12).
"""


if __name__ == "__main__":
    main()
