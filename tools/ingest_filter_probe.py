#!/usr/bin/env python3
"""The frame event filters on the ESL-like stream of `bench.py --esl` (rig.render_stream, 48 frames, quarter-period packets of
pageable EventCD records) through DepthReprojectionProcessor, for each of the four filters twice:

    host chain   RuntimeParams(device_frame_filters=False): while a filter is selected the stream takes the host chain (NumPy
                 trigger finder, one GPU call per packet for the activity filter, the cut frame's round trips) -- the comparator
    device       RuntimeParams(device_frame_filters=True): the filter is a stage of the device ingest

and once with no filter selected.  Per leg: one untimed pass over the stream, then `--passes` timed ones; Mev/s and ms per shown
frame of the median pass, every pass's time beside it.  One JSON line per leg.

    python tools/ingest_filter_probe.py                       # every leg
    python tools/ingest_filter_probe.py --profile OUTDIR      # + one rocprofv3 --kernel-trace --stats run of a device leg (a child
                                                              #   process of its own): the filter kernels' share of the frame stream
    python tools/ingest_filter_probe.py --counters OUTDIR     # + counters of the same leg, in a run of their own
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = {1: "FirstEventPerYT", 2: "FirstEventPerXY", 3: "LastEventPerXY", 4: "MeanFirstLastEventPerXY"}  # = presses of key E


def run_leg(tables, packets, n_events, presses, device, passes):
    import numpy as np
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    shown = []

    class Window:
        def should_close(self):
            return False

        def show_async(self, img):
            shown.append(int(img[::97, ::89].sum()))  # (consumes the frame inside the callback)

    params = RuntimeParams(camera_width=640, camera_height=480, projector_width=tables["proj_w"], projector_height=tables["proj_h"],
                           projector_fps=60, z_near=tables.get("z_near", 0.1), z_far=tables.get("z_far", 1.2), calib=None,
                           projector_time_map=None, no_frame_dropping=True, tables=tables, device_frame_filters=device,
                           ingest_frame_views=True, ingest_result_ring=64)
    with DepthReprojectionProcessor(params, window=Window()) as proc:
        for _ in range(presses):
            proc.keyboard_cb("e", None, "release")
        name = str(proc._pipe.ev_filter_proc.selected_filter())
        times, sums = [], []
        for rep in range(passes + 1):  # (the first pass is the warm-up)
            if rep:
                proc.reset()
            shown.clear()
            c0 = time.perf_counter()
            for pk in packets:
                proc.process_events(pk)
            proc.flush()
            times.append(time.perf_counter() - c0)
            sums.append(list(shown))
        on_host = bool(proc._pipe._host_chain_active)
        out_pct = proc.stats_printer.metrics["frame evs filtered out [%]"]
    timed = sorted(times[1:])
    dt = timed[len(timed) // 2]
    return {"filter": name, "device_frame_filters": bool(device), "host_chain": on_host, "Mevents_per_s": round(n_events / dt / 1e6, 2),
            "ms_per_shown_frame": round(dt / max(len(sums[-1]), 1) * 1e3, 4), "frames_shown": len(sums[-1]),
            "every_pass_the_same_frames": all(s == sums[0] for s in sums), "passes_ms": [round(t * 1e3, 2) for t in times[1:]],
            "warmup_ms": round(times[0] * 1e3, 2), "filtered_out_pct_mean": round(out_pct.mean(), 2) if len(out_pct) else None,
            "frame_checksums": sums[-1][:4]}


def kernel_shares(outdir):
    """the kernels' share of the GPU time in a rocprofv3 --stats run: rows of its kernel statistics, filter kernels marked"""
    rows = []
    for fn in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        with open(fn) as f:
            for r in csv.DictReader(f):
                rows.append(r)
    if not rows:
        return {"error": "no kernel statistics found under " + outdir}
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"total_ms": round(tot / 1e6, 3), "kernels": []}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        out["kernels"].append({"name": r["Name"][:60], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                               "share_pct": round(float(r["TotalDurationNs"]) / tot * 100, 2)})
    out["frame_filter_share_pct"] = round(sum(k["share_pct"] for k in out["kernels"] if "k_ff_" in k["name"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", default="1,2,3,4", help="presses of key E per leg (0: no filter)")
    ap.add_argument("--legs", default="host,device")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--no-filter-leg", action="store_true", help="also a leg with no filter selected")
    ap.add_argument("--profile", metavar="OUTDIR", help="rocprofv3 --kernel-trace --stats of one device leg (--profile-filter)")
    ap.add_argument("--counters", metavar="OUTDIR", help="rocprofv3 --pmc of the same leg, a run of its own")
    ap.add_argument("--profile-filter", type=int, default=3)
    args = ap.parse_args()
    child = [sys.executable, os.path.abspath(__file__), "--legs", "device", "--filters", str(args.profile_filter), "--passes", "1",
             "--frames", str(args.frames)]
    if args.profile:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.profile, "--"] + child, check=True)
        print(json.dumps({"profile": FILTERS[args.profile_filter], **kernel_shares(args.profile)}), flush=True)
        return
    if args.counters:
        subprocess.run(["rocprofv3", "--pmc", "SQ_WAVES", "GRBM_GUI_ACTIVE", "--output-format", "csv", "-d", args.counters, "--"] + child, check=True)
        return
    import numpy as np
    from x_maps_amd import rig
    cp, tables, _, _ = rig.make_esl_like(row_stride=13)
    stream, _ = rig.render_stream(cp, tables, n_frames=args.frames, row_stride=13, seed=9)
    q = int(1e6 / 60 / 4)
    cuts = np.searchsorted(stream["t"], np.arange(stream["t"][0], stream["t"][-1] + q, q))
    packets = [np.array(stream[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    legs = [(int(f), leg == "device") for f in args.filters.split(",") if f != "" for leg in args.legs.split(",")]
    if args.no_filter_leg:
        legs = [(0, False), (0, True)] + legs
    for presses, device in legs:
        print(json.dumps(run_leg(tables, packets, len(stream), presses, device, args.passes)), flush=True)


if __name__ == "__main__":
    main()
