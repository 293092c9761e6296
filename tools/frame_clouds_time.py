#!/usr/bin/env python3
"""Time the frame -> point cloud entry and the ingest's cloud stage on the ESL-like stream.

    python tools/frame_clouds_time.py [--md profiles/frame_clouds.md] [--repeats 20] [--parent-lib PATH]

NOT the benchmark (bench.py measures the flagship workload); this gives the numbers of profiles/frame_clouds.md.  The frames are
the ones `bench.py --esl` renders (x_maps_amd/rig.py's ESL-like stand-in: the reference's calibration numbers, a rendered scene) --
the ESL recordings are not available here, and the output says so.

The parent process never opens the GPU: every step runs in a fresh child process under its own time limit (--step-timeout), and no
further step is started after one that failed or ran out of time.
  group    xm_frames_to_point_clouds on a group of 32 frames, device-resident (records in, clouds out, the final synchronise):
           after warm-up the median of --repeats calls, each between two device events (tools/_timing.py); the NumPy oracle
           (tests/frame_cloud_cases.py) on the same group, host clock; the bytes of the event stream over the measured time.
           Every frame's row count and the first frame's cloud are compared with the oracle's.
  ingest   the ESL-like stream (48 frames, quarter-period packets of pinned records, activity filter on, BGR frames out) through
           one DeviceIngest, whole passes alternating stage off / on in ONE process, the median pass of each reported; with
           --parent-lib (a build of the parent commit's library, XM_LIB) the same stage-off passes on that build in processes of
           their own, alternating with this build's: this, parent, this, parent."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _frame_stage as F  # noqa: E402
from _frame_stage import GROUP, HBM_BYTES_PER_S  # noqa: E402
from _timing import clock_state, timed  # noqa: E402

MAX_POINTS = 262144
NEW_SYMBOLS = ("xm_cloud_set_tables", "xm_frames_to_point_clouds", "xm_ingest_set_cloud_output", "xm_ingest_copy_cloud")


def step_group(repeats, device):
    F.gpu()
    import ctypes as C

    import frame_cloud_cases as K
    from x_maps_amd import XMapsEngine, rig
    from x_maps_amd import _native as N
    cp, tables, _, _ = rig.make_esl_like(row_stride=13, device=device)
    tables = dict(tables)
    frames = [rig.render_events(cp, tables, row_stride=13, seed=f)[0] for f in range(GROUP)]
    evs, offs = K.concat(frames)
    res = {"frames": GROUP, "events_per_frame": int(len(evs)) // GROUP}
    t0 = time.perf_counter()
    want = [K.oracle(tables, f) for f in frames]
    res["numpy_oracle_ms_per_group"] = round((time.perf_counter() - t0) * 1e3, 2)
    rows = sum(o["stats"]["n_inliers"] for o in want)
    with XMapsEngine(tables, device=device) as eng:
        got = eng.frames_to_point_clouds(frames)
        assert all(getattr(got[i][1], k) == want[i]["stats"][k] for i in range(GROUP) for k in K.STAT_FIELDS), "statistics differ from the oracle's"
        fin = np.isfinite(want[0]["cloud"])
        assert np.array_equal(np.isfinite(got[0][0]), fin) and np.allclose(got[0][0][fin], want[0]["cloud"][fin], rtol=1e-5, atol=1e-5)
        d_ev = eng.to_device(evs)
        d_out = eng.dev_alloc(max(len(evs), 1) * 12)
        op = offs.ctypes.data_as(C.POINTER(C.c_uint64))

        def call():
            N.check(eng._lib.xm_frames_to_point_clouds(eng._h, C.c_void_p(d_ev), op, GROUP, 0, N.XM_MEM_DEVICE, C.c_void_p(d_out), None))
            eng.sync()
        t = timed(call, repeats)
        # the event stream alone: 16 bytes per record, read once by each of the two passes that need the whole record
        stream_bytes = len(evs) * 16
        # everything the passes move: the records twice, the 2-byte code written and read, x | y re-read and two map gathers and
        # 12 bytes stored per row, the 64-event counts and offsets
        moved = len(evs) * (32 + 4) + rows * (4 + 8 + 12) + (len(evs) // 64) * 16
        res["device"] = {"ms_per_group_device_events": round(t.ev, 4), "min_max_ms": [round(t.ev_min, 4), round(t.ev_max, 4)],
                         "ms_per_group_host_clock": round(t.host, 4), "us_per_frame": round(t.ev / GROUP * 1e3, 2),
                         "Gevents_per_s": round(len(evs) / (t.ev * 1e-3) / 1e9, 3),
                         "event_stream_share_of_hbm_rate": round(stream_bytes / HBM_BYTES_PER_S / (t.ev * 1e-3), 4),
                         "bytes_moved_per_group": int(moved), "moved_share_of_hbm_rate": round(moved / HBM_BYTES_PER_S / (t.ev * 1e-3), 4)}
        t = timed(lambda: eng.frames_to_point_clouds(frames), max(3, repeats // 4))
        res["ms_per_group_from_host_memory"] = round(t.host, 3)
        eng.dev_free(d_out)
        eng.dev_free(d_ev)
    res["rows_per_frame"] = rows // GROUP
    print("FC_STEP " + json.dumps(res), flush=True)


def step_ingest(passes, device, with_stage):
    def check(ing, got, on):  # the stage ran for the pass's frames, or for none of them
        held = [ing.cloud(fr.seq, with_stats=True) for fr in got]
        assert all((h is not None and len(h[0]) == min(h[1].n_inliers, MAX_POINTS) > 0) if on else h is None for h in held)
    set_stage = (lambda ing, on: ing.set_cloud_output(on, MAX_POINTS)) if with_stage else None
    print("FC_STEP " + json.dumps(F.ingest_passes(passes, device, NEW_SYMBOLS, set_stage, check)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    F.add_arguments(ap, "a build of the parent commit's library: its stage-off passes, in processes of their own")
    a = ap.parse_args(argv)
    if a.step == "group":
        return step_group(a.repeats, a.device)
    if a.step in ("ingest", "ingest_off_only"):
        return step_ingest(a.passes, a.device, a.step == "ingest")
    res = {"frames": F.FRAMES_NOTE, "clock_state": clock_state(), "repeats": a.repeats, "passes": a.passes}
    steps = [("group", "group", None), ("ingest", "ingest", None)]
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        steps += [("ingest_parent_build", "ingest_off_only", lib), ("ingest_again", "ingest", None), ("ingest_parent_build_again", "ingest_off_only", lib)]
    if F.run_steps(__file__, "FC_STEP ", steps, a, res) and a.md:
        F.write_md(a.md, res, markdown)
    return res


def markdown(r, notes="") -> str:
    g, d, i = r["group"], r["group"]["device"], r["ingest"]
    off, on = i["stage_off"], i["stage_on"]
    runs = [("this build, stage off", off), ("this build, stage on", on)]
    par = [r[k]["stage_off"] for k in ("ingest_parent_build", "ingest_parent_build_again") if k in r]
    if par:
        runs += [("parent commit's build (stage absent), run 1", par[0]), ("this build, stage off, run 2", r["ingest_again"]["stage_off"]),
                 ("this build, stage on, run 2", r["ingest_again"]["stage_on"]), ("parent commit's build, run 2", par[1])]
    if par:
        mine = np.mean([off["Mevents_per_s"], r["ingest_again"]["stage_off"]["Mevents_per_s"]])
        theirs = np.mean([p["Mevents_per_s"] for p in par])
        par_note = (f"Stage off against the parent's build, means of the two alternating runs: {mine:.1f} / {theirs:.1f} = {mine / theirs:.3f} "
                    f"(the README states a +-6 % run-to-run spread for this stream).")
    else:
        par_note = "The parent commit's build was not timed in this run (--parent-lib)."
    return F.md_head("Frames of events -> per-event point clouds", "frame_clouds_time.py", r["clock_state"]) + f"""
## The group entry (`xm_frames_to_point_clouds`)

A group of {g['frames']} frames of {g['events_per_frame']} events ({g['rows_per_frame']} cloud rows per frame), records and clouds
device-resident, four launches and the final synchronise.  Median of {r['repeats']} calls after warm-up, each between two device
events.

| ms / group (min .. max) | us / frame | Gev/s | event stream at 6.29 TB/s | MB moved / group | moved bytes at 6.29 TB/s |
|---|---|---|---|---|---|
| {d['ms_per_group_device_events']} ({d['min_max_ms'][0]} .. {d['min_max_ms'][1]}) | {d['us_per_frame']} | {d['Gevents_per_s']} | {d['event_stream_share_of_hbm_rate']} | {d['bytes_moved_per_group'] / 1e6:.1f} | {d['moved_share_of_hbm_rate']} |

Host clock around the same call: {d['ms_per_group_host_clock']} ms.  From host memory (records up, valid rows and statistics back,
synchronous): {g['ms_per_group_from_host_memory']} ms / group.  The NumPy oracle (`tests/frame_cloud_cases.py`) on the same group:
{g['numpy_oracle_ms_per_group']} ms on the host.

"Event stream" = 16 bytes per record once, over 6.29 TB/s (the measured float4 copy rate), over the measured time: the share of the
streaming rate at which the entry consumes events.  "Moved" counts what the four passes really move: the records twice, the 2-byte
code written and read, per row the record's first word, two map gathers and 12 bytes stored, and the 64-event counts and offsets.
A group this small (about 5 M events, 80 MB) lies inside the Infinity Cache, and its four launches are a visible part of the time.

""" + F.md_ingest(r, "xm_ingest_set_cloud_output", f"; max_points = {MAX_POINTS}", F.run_rows(runs), par_note, notes)


if __name__ == "__main__":
    main()
