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
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _frame_stage as F  # noqa: E402
from _frame_stage import GROUP, HBM_BYTES_PER_S  # noqa: E402
from _timing import clock_state, timed  # noqa: E402

NEW_SYMBOLS = ("xm_frames_to_time_surfaces", "xm_ingest_set_surface_output", "xm_ingest_copy_surface", "xm_ingest_surface_dtype")


def step_group(repeats, device):
    F.gpu()
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
    set_stage = (lambda ing, on: ing.set_surface_output("last" if on else None, np.float32)) if with_stage else None
    print("FS_STEP " + json.dumps(F.ingest_passes(passes, device, NEW_SYMBOLS, set_stage)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    F.add_arguments(ap, "a build of the parent commit's library: its stage-off passes, in a process of its own")
    a = ap.parse_args(argv)
    if a.step == "group":
        return step_group(a.repeats, a.device)
    if a.step in ("ingest", "ingest_off_only"):
        return step_ingest(a.passes, a.device, a.step == "ingest")
    res = {"frames": F.FRAMES_NOTE, "clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    steps = [("group", "group", None), ("ingest", "ingest", None)]
    if a.parent_lib:
        steps.append(("ingest_parent_build", "ingest_off_only", os.path.abspath(a.parent_lib)))
    if F.run_steps(__file__, "FS_STEP ", steps, a, res) and a.md:
        F.write_md(a.md, res, markdown)
    return res


def markdown(r, notes="") -> str:
    g, i = r["group"], r["ingest"]
    rows = "\n".join(f"| {k} | {g[k]['ms_per_group_device_events']} ({g[k]['min_max_ms'][0]} .. {g[k]['min_max_ms'][1]}) | {g[k]['us_per_frame']} | "
                     f"{g[k]['Gevents_per_s']} | {g[k]['bytes_moved_per_group'] / 1e6:.1f} | {g[k]['share_of_hbm_rate']} |" for k in ("float32", "float64"))
    off, on = i["stage_off"], i["stage_on"]
    par = r.get("ingest_parent_build")
    runs = [("stage off", off), ("stage on (float32, last)", on)] + ([("parent commit's build, stage absent", par["stage_off"])] if par else [])
    par_note = (f"Stage off against the parent's build: {off['Mevents_per_s']} / {par['stage_off']['Mevents_per_s']} = "
                f"{off['Mevents_per_s'] / par['stage_off']['Mevents_per_s']:.3f} (the README states a +-6 % run-to-run spread for this stream)."
                if par else "The parent commit's build was not timed in this run (--parent-lib).")
    return F.md_head("Frames of events -> camera time surfaces", "frame_surfaces_time.py", r["clock_state"]) + f"""
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

""" + F.md_ingest(r, "xm_ingest_set_surface_output", "", F.run_rows(runs), par_note, notes)


if __name__ == "__main__":
    main()
