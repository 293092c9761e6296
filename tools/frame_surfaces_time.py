#!/usr/bin/env python3
"""Time the frame -> time surface entry and the ingest's surface stage on the ESL-like stream.

    python tools/frame_surfaces_time.py [--md profiles/frame_surfaces.md] [--repeats 20] [--parent-lib PATH]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/frame_surfaces.md.  The frames are
the ones `bench.py --esl` renders (x_maps_amd/rig.py's ESL-like stand-in: the reference's calibration numbers, a rendered scene) --
the ESL recordings are not available here, and the output says so.

The parent process never opens the GPU: every step runs in a fresh child process under its own time limit (--step-timeout), and no
further step is started after one that failed or ran out of time.
  group    xm_frames_to_time_surfaces on a group of 32 frames, device-resident (records in, surfaces out, the final synchronise):
           after warm-up the median of --repeats calls, each between two device events (tools/_timing.py); the NumPy oracle
           (tests/frame_surface_cases.py) on the same group, host clock; the bytes the definition moves over the measured time.
           The first frame's surface is compared with the oracle's in every step.
  ingest   the ESL-like stream (48 frames, quarter-period packets of pinned records, activity filter on, BGR frames out) through
           one DeviceIngest, whole passes alternating stage off / on in ONE process, the median pass of each reported; with
           --parent-lib (a build of the parent commit's library, XM_LIB) the same stage-off passes on that build in a process of
           its own."""
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

HBM_BYTES_PER_S = 6.29e12  # measured streaming rate of an MI355X (float4 copy)
GROUP = 32
TRIED = "## Notes\n"


def _gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")
    torch.cuda.init()
    return torch


def step_group(repeats, device):
    _gpu()
    import ctypes as C

    import frame_surface_cases as K
    from x_maps_amd import XMapsEngine, rig
    from x_maps_amd import _native as N
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    frames = [rig.render_events(cp, tables, row_stride=13, seed=f)[0] for f in range(GROUP)]
    evs, offs = K.concat(frames)
    w, h = cp.camera_width, cp.camera_height
    px = w * h
    res = {"frames": GROUP, "events_per_frame": int(len(evs)) // GROUP, "cells": px}
    t0 = time.perf_counter()
    want = [K.oracle(f, w, h, "last", np.float32) for f in frames]
    res["numpy_oracle_ms_per_group"] = round((time.perf_counter() - t0) * 1e3, 2)
    taking_part = sum(st["n_events"] - st["n_index_errors"] for _, st in want)
    nz = sum(st["n_pixels"] for _, st in want)
    with XMapsEngine(tables, device=device) as eng:
        surfs, stats = eng.frames_to_time_surfaces(frames, "last", np.float32)
        assert np.array_equal(surfs[0].view(np.uint32), want[0][0].view(np.uint32)), "the entry differs from the oracle on frame 0"
        assert all(getattr(stats[i], k) == want[i][1][k] for i in range(GROUP) for k in K.STAT_FIELDS)
        d_ev = eng.to_device(evs)
        op = offs.ctypes.data_as(C.POINTER(C.c_uint64))
        for name, dt, esz in (("float32", N.XM_T_FLOAT32, 4), ("float64", N.XM_T_FLOAT64, 8)):
            d_out = eng.dev_alloc(GROUP * px * esz)

            def call():
                N.check(eng._lib.xm_frames_to_time_surfaces(eng._h, C.c_void_p(d_ev), op, GROUP, 0, N.XM_SURFACE_LAST, dt, N.XM_MEM_DEVICE,
                                                            C.c_void_p(d_out), None))
                eng.sync()
            t = timed(call, repeats)
            eng.dev_free(d_out)
            # bytes the definition moves: 16 per event read, 4 per taking-part event into the winner map, per cell 4 of the map read
            # and one store of the output type, per non-zero cell the 8-byte gather of the winner's stamp and 4 of the map zeroed
            moved = len(evs) * 16 + taking_part * 4 + GROUP * px * (4 + esz) + nz * 12
            res[name] = {"ms_per_group_device_events": round(t.ev, 4), "min_max_ms": [round(t.ev_min, 4), round(t.ev_max, 4)],
                         "ms_per_group_host_clock": round(t.host, 4), "us_per_frame": round(t.ev / GROUP * 1e3, 2),
                         "bytes_moved_per_group": int(moved), "share_of_hbm_rate": round(moved / HBM_BYTES_PER_S / (t.ev * 1e-3), 4),
                         "Gevents_per_s": round(len(evs) / (t.ev * 1e-3) / 1e9, 3)}
        t = timed(lambda: eng.frames_to_time_surfaces(frames, "last", np.float32), max(3, repeats // 4))
        res["ms_per_group_from_host_memory"] = round(t.host, 3)
        eng.dev_free(d_ev)
    res["non_zero_pixels_per_frame"] = nz // GROUP
    print("FS_STEP " + json.dumps(res), flush=True)


def step_ingest(passes, device, with_stage):
    _gpu()
    if not with_stage:  # (the parent commit's build through XM_LIB: it does not export the entries this step never calls)
        from x_maps_amd import _native as N
        for name in ("xm_frames_to_time_surfaces", "xm_ingest_set_surface_output", "xm_ingest_copy_surface", "xm_ingest_surface_dtype"):
            N.SYMBOLS.pop(name, None)
    from x_maps_amd import XMapsEngine, rig
    from x_maps_amd import synthetic as S
    from x_maps_amd.ingest import DeviceIngest
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    n_mean = int(np.mean([len(rig.render_events(cp, tables, row_stride=13, seed=f)[0]) for f in range(8)]))
    n_frames = 48
    stream, _ = rig.render_stream(cp, tables, n_frames=n_frames, row_stride=13, seed=9)
    res = {"events": int(len(stream)), "frames_rendered": n_frames}
    with XMapsEngine(tables, device=device, n_slots=4) as eng:
        pin = eng.host_empty((len(stream),), S.EVENT_CD_DTYPE)
        pin[:] = stream
        packet = int(1e6 / 60 / 4)
        cuts = np.searchsorted(pin["t"], np.arange(pin["t"][0], pin["t"][-1] + packet, packet))
        packets = [pin[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        with DeviceIngest(eng, 60, capacity_events=1 << 21, max_packet_events=1 << 18, expected_events_per_frame=n_mean,
                          result_ring=n_frames + 2, want_depth=False, want_bgr=True, activity_filter=True) as ing:
            def one_pass():
                c0 = time.perf_counter()
                for pk in packets:
                    ing.push_pinned(pk)
                ing.flush()
                got = ing.poll(copy=False)
                dt = time.perf_counter() - c0
                ing.reset()
                return dt, len(got)
            modes = [False, True] if with_stage else [False]
            for on in modes * 2:  # warm-up: both settings twice (the first on-pass allocates the stage's ring)
                if with_stage:
                    ing.set_surface_output("last" if on else None, np.float32)
                one_pass()
            times = {m: [] for m in modes}
            cut = None
            for k in range(passes * len(modes)):  # alternating, in one process
                on = modes[k % len(modes)]
                if with_stage:
                    ing.set_surface_output("last" if on else None, np.float32)
                dt, n = one_pass()
                times[on].append(dt)
                cut = n if cut is None else cut
                assert n == cut, "the passes cut different numbers of frames"
            res["frames_cut"] = cut
            for on, v in times.items():
                med = float(np.median(v))
                res["stage_on" if on else "stage_off"] = {"Mevents_per_s": round(len(stream) / med / 1e6, 1), "ms_per_pass_median": round(med * 1e3, 3),
                                                          "passes_ms": [round(x * 1e3, 3) for x in v]}
    print("FS_STEP " + json.dumps(res), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--md", help="write the profile (markdown) here")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7, help="timed passes of the stream per setting")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", help="a build of the parent commit's library: its stage-off passes, in a process of its own")
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--step", help=argparse.SUPPRESS)  # (internal: one step in this process)
    a = ap.parse_args(argv)
    if a.step == "group":
        return step_group(a.repeats, a.device)
    if a.step in ("ingest", "ingest_off_only"):
        return step_ingest(a.passes, a.device, a.step == "ingest")
    res = {"frames": "rendered from rig.py's ESL-like stand-in, as bench.py --esl renders them; NOT the ESL recordings",
           "clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    steps = [("group", "group", None), ("ingest", "ingest", None)]
    if a.parent_lib:
        steps.append(("ingest_parent_build", "ingest_off_only", os.path.abspath(a.parent_lib)))
    ok = True
    for name, step, lib in steps:
        env = dict(os.environ)
        env.pop("XM_LIB", None)
        if lib:
            env["XM_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--repeats", str(a.repeats), "--passes", str(a.passes),
               "--device", str(a.device)]
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res[name] = {"error": f"no result within {a.step_timeout} s"}
            ok = False
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("FS_STEP ")]
        if r.returncode != 0 or not line:
            res[name] = {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-1500:]}
            ok = False
            break
        res[name] = json.loads(line[-1][len("FS_STEP "):])
    res["complete"] = ok
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.md and ok:
        notes = ""
        if os.path.exists(a.md):  # the hand-written section of an earlier profile stays
            old = open(a.md).read()
            if TRIED in old:
                notes = old.split(TRIED, 1)[1]
        with open(a.md, "w") as f:
            f.write(markdown(res, notes))
    return res


def markdown(r, notes="") -> str:
    g, i = r["group"], r["ingest"]
    rows = "\n".join(f"| {k} | {g[k]['ms_per_group_device_events']} ({g[k]['min_max_ms'][0]} .. {g[k]['min_max_ms'][1]}) | {g[k]['us_per_frame']} | "
                     f"{g[k]['Gevents_per_s']} | {g[k]['bytes_moved_per_group'] / 1e6:.1f} | {g[k]['share_of_hbm_rate']} |" for k in ("float32", "float64"))
    off, on = i["stage_off"], i["stage_on"]
    par = r.get("ingest_parent_build")
    par_txt = (f"| parent commit's build, stage absent | {par['stage_off']['Mevents_per_s']} | {par['stage_off']['ms_per_pass_median']} | "
               f"{par['stage_off']['passes_ms']} |\n") if par else ""
    par_note = (f"Stage off against the parent's build: {off['Mevents_per_s']} / {par['stage_off']['Mevents_per_s']} = "
                f"{off['Mevents_per_s'] / par['stage_off']['Mevents_per_s']:.3f} (the README states a +-6 % run-to-run spread for this stream)."
                if par else "The parent commit's build was not timed in this run (--parent-lib).")
    return f"""# Frames of events -> camera time surfaces: times on the ESL-like stream

Written by `tools/frame_surfaces_time.py` on an MI355X.  **The frames are rendered** from `x_maps_amd/rig.py`'s ESL-like stand-in
(640 x 480 camera, the frames `bench.py --esl` renders), not the ESL recordings.  Every step in a process of its own.
Clock state of the box, queried idle before the first launch: {r['clock_state']}.

**Nothing was measured before this**: the parent commit has no such entry.  These are first numbers, not a bar.

## The group entry (`xm_frames_to_time_surfaces`)

A group of {g['frames']} frames of {g['events_per_frame']} events on {g['cells']} cells ({g['non_zero_pixels_per_frame']} non-zero pixels per
frame), records and surfaces device-resident, three launches and the final synchronise.  Medians of {r['repeats']} calls after
warm-up, each between two device events.

| output | ms / group (min .. max) | us / frame | Gev/s | MB moved / group | share of 6.29 TB/s |
|---|---|---|---|---|---|
{rows}

Host clock around the same call: {g['float32']['ms_per_group_host_clock']} ms (float32).  From host memory (records up, surfaces and
statistics back, synchronous): {g['ms_per_group_from_host_memory']} ms / group.  The NumPy oracle (`tests/frame_surface_cases.py`,
np.maximum.at on indices) on the same group: {g['numpy_oracle_ms_per_group']} ms on the host.

Bytes moved = 16 per event read + 4 per taking-part event into the winner map + per cell 4 of the map read and one store of the
output type + per non-zero cell the 8-byte gather of the winner's stamp and 4 of the map zeroed.  The share is those bytes over
6.29 TB/s (the measured float4 copy rate) over the measured time: a group is 32 x 1.2 MB of winner map, beyond one XCD's L2, so
the atomics and the map's re-read go through the Infinity Cache; the launches of a group this small (about 5 M events) are a
visible part of the time.

## The ingest's stage (`xm_ingest_set_surface_output`)

The ESL-like stream ({i['events']} events, {i['frames_rendered']} frames rendered, {i['frames_cut']} cut), quarter-period packets of
pinned records, activity filter on, BGR frames out; whole passes (push everything, flush, poll) alternating stage off / on in one
process, {r['passes']} timed passes each, the median reported.

| setting | Mev/s | ms / pass (median) | passes, ms |
|---|---|---|---|
| stage off | {off['Mevents_per_s']} | {off['ms_per_pass_median']} | {off['passes_ms']} |
| stage on (float32, last) | {on['Mevents_per_s']} | {on['ms_per_pass_median']} | {on['passes_ms']} |
{par_txt}
Stage on / off: {on['Mevents_per_s'] / off['Mevents_per_s']:.3f} of the rate.  {par_note}

{TRIED}
{notes.strip() or "(written by hand below this heading; kept when the tool rewrites the file)"}
"""


if __name__ == "__main__":
    main()
