#!/usr/bin/env python3
"""Calibrate the projector time map from a white-frame recording.

    python tools/calibrate_time_map.py RECORDING --calib YAML --out DIR

RECORDING is a Prophesee RAW file (EVT 2.0 / 2.1 / 3.0) or a DAT file of a white image projected onto a plane.  It is decoded by the
existing readers and the device ingest (polarity filter, activity filter, trigger finder), whose surface stage gives every cut
frame's camera time surface (first event per pixel, float64); every surface goes to x_maps_amd.time_map_calibration, which
averages them, finds the projected frame's corners, warps the quadrilateral to the projector's size and fills what is missing.
Written:

    DIR/time_map_proj.npy   the projector-space time map, float32 [proj_h][proj_w] (build_tables(projector_time_map=))
    DIR/time_map_rect.npy   the same rectified as the live pipe rectifies it: the file RuntimeParams.projector_time_map
                            (the reference's --projector-time-map) takes

and the statistics are printed as one JSON line.  The arithmetic is this build's definition (include/xmaps.h): the reference ships no
code for this step.  No run on a real white-plane recording has been made: none exists beside this project.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def _corners(text):
    v = [float(t) for t in text.replace(";", ",").split(",")]
    if len(v) != 8:
        raise argparse.ArgumentTypeError("corners: x,y of TL, TR, BR, BL -- eight numbers")
    return tuple((v[2 * k], v[2 * k + 1]) for k in range(4))


def calibrate(recording, calib, out_dir, camera=(640, 480), projector=(1080, 1920), fps=60, min_share=0.5, corners=None, corner_order=0,
              chunk_words=1 << 20, device=0, activity_filter=True, group=16, frame_sync="pauses", trigger_id=-1, trigger_edge="rising",
              trigger_activity_filter=False):
    from run_esl_on_arrival import raw_format
    from x_maps_amd import calibration as C
    from x_maps_amd import dat, evt2, evt21, evt3
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    from x_maps_amd.time_map_calibration import TimeMapCalibrator
    fmt = raw_format(recording)
    mod = {3: evt3, 2: evt2, 21: evt21, "dat": dat}[fmt]
    cp = C.CamProjCalibrationParams.from_yaml(calib, camera[0], camera[1], projector[0], projector[1])
    tables = C.build_tables(cp, device=device)  # (the ingest needs a rig; its frames are not looked at)

    class Window:
        def should_close(self):
            return False

        def show_async(self, img):
            pass

    with TimeMapCalibrator(camera, device=device) as cal:
        pending = []

        def hand_over():
            if pending:
                cal.add_surfaces(np.stack(pending))
                pending.clear()

        def surface_cb(surf):
            pending.append(surf)
            if len(pending) >= group:
                hand_over()

        params = RuntimeParams(camera_width=camera[0], camera_height=camera[1], projector_width=projector[0], projector_height=projector[1],
                               projector_fps=fps, z_near=0.1, z_far=1.2, calib=None, projector_time_map=None, no_frame_dropping=True,
                               camera_perspective=False, tables=tables, device=device, device_ingest=True, activity_filter=activity_filter,
                               surface_callback=surface_cb, surface_select="first", surface_dtype=np.float64,
                               raw_legacy_halves=fmt == 21 and evt21.raw_legacy_halves(recording), frame_sync=frame_sync,
                               ext_trigger_id=trigger_id, ext_trigger_edge=trigger_edge,  # ("ext_trigger": a frame per trigger-to-trigger span)
                               ext_trigger_activity_filter=bool(trigger_activity_filter))
        with DepthReprojectionProcessor(params, window=Window()) as proc:
            push = {3: proc.process_evt3_words, 2: proc.process_evt2_words, 21: proc.process_evt21_words, "dat": proc.process_dat_records}[fmt]
            for words in mod.read_raw_words(recording, chunk_words=chunk_words):
                push(words)
            proc.flush()
        hand_over()
        if cal.stats.n_used == 0:
            raise ValueError(f"{recording}: no usable frame was cut ({cal.stats.n_added} surfaces, {cal.stats.n_skipped} skipped)")
        cal.mean(min_share, need_corners=corners is None)
        time_map, st = cal.solve(projector, corners=corners, corner_order=corner_order)
    rect = C.build_tables(cp, device=device, projector_time_map=time_map)["time_map_rect"]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "time_map_proj.npy"), time_map)
    np.save(os.path.join(out_dir, "time_map_rect.npy"), rect)
    return {"recording": recording, "format": {3: "EVT 3.0", 2: "EVT 2.0", 21: "EVT 2.1", "dat": "DAT"}[fmt],
            "surfaces_added": st.n_added, "surfaces_skipped": st.n_skipped, "min_count": st.min_count, "n_valid": st.n_valid,
            "n_core": st.n_core, "corners_detected": None if st.corners is None else [list(c) for c in st.corners],
            "corners_used": [list(c) for c in (corners or st.corners)], "corner_order": corner_order,
            "n_missing": st.n_missing, "n_unfilled": st.n_unfilled,
            "time_map_proj": os.path.join(out_dir, "time_map_proj.npy"), "time_map_rect": os.path.join(out_dir, "time_map_rect.npy"),
            "definition": "this build's definition (include/xmaps.h, projector time-map calibration): the reference ships no code for it"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("recording")
    ap.add_argument("--calib", required=True, help="the rig's calibration YAML (the reference's format)")
    ap.add_argument("--out", required=True, help="directory for time_map_proj.npy and time_map_rect.npy")
    ap.add_argument("--camera", type=_size, default=(640, 480), help="WxH")
    ap.add_argument("--projector", type=_size, default=(1080, 1920), help="WxH")
    ap.add_argument("--fps", type=int, default=60)
    ap.add_argument("--min-share", type=float, default=0.5, help="a pixel is valid when this share of the frames saw it")
    ap.add_argument("--corners", type=_corners, default=None, help="x,y of TL,TR,BR,BL in the camera image instead of the detected ones")
    ap.add_argument("--corner-order", type=int, default=0, help="0..7: which symmetry of the square maps the corners to the projector's")
    ap.add_argument("--chunk-words", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-activity-filter", action="store_true")
    ap.add_argument("--frame-sync", choices=("pauses", "ext-trigger"), default="pauses",
                    help="cut the white frames at pauses (the trigger finder) or at the recording's EXT_TRIGGER words (sync jack wired)")
    ap.add_argument("--trigger-id", type=int, default=-1, help="--frame-sync ext-trigger: the trigger channel (-1: any)")
    ap.add_argument("--trigger-edge", choices=("rising", "falling", "both"), default="rising")
    ap.add_argument("--trigger-activity-filter", action="store_true",
                    help="--frame-sync ext-trigger: the activity filter in front of the cut, so that noise is not averaged into the map (off by default)")
    a = ap.parse_args(argv)
    rep = calibrate(a.recording, a.calib, a.out, a.camera, a.projector, a.fps, a.min_share, a.corners, a.corner_order, a.chunk_words,
                    a.device, not a.no_activity_filter, frame_sync=a.frame_sync.replace("-", "_"), trigger_id=a.trigger_id,
                    trigger_edge=a.trigger_edge, trigger_activity_filter=a.trigger_activity_filter)
    print(json.dumps(rep))
    return rep


if __name__ == "__main__":
    main()
