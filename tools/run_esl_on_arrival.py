#!/usr/bin/env python3
"""The day the ESL data is there: BASELINE configs 0 / 2 and the reference's Table-1 row, in one command.

    python tools/run_esl_on_arrival.py --raw /ESL_data/static/seq1/data.raw --bias /ESL_data/static/seq1/data.bias \\
        --calib data/ESL_calib_hhi.yaml --scans /ESL_data/static/seq1/ --eval-calib data/calib.yaml --out report.json

Part A -- the replay (`.vscode/launch.json:24-49`: depth_reprojection.py --projector-width 1080 --projector-height 1920 --calib
data/ESL_calib_hhi.yaml --input data.raw --z-near 0.1 --z-far 1.2 --no-frame-dropping): the recording's words (EVT 3.0, 2.0 or
2.1 by a RAW file's header, or the records of a DAT file) go through `with DepthReprojectionProcessor(params)` in chunks -- decoded on the device, polarity / activity
filter, trigger finder and the hot path there too (this build's default RuntimeParams) --; reported: frames shown, events, events/s,
ms per shown frame next to the reference's published 2.67 ms (Threadripper PRO 5955WX, frame stage only), and -- with
--compare-host-chain -- the same file through the opt-out host chain (NumPy decoder + filters + trigger finder), frame by frame.
The bias file only configures a live camera (bias_events_iterator.py:69-78): accepted, recorded, not used for a file.
With --scans-from-raw DIR part A also writes every shown frame's camera time surface to DIR/scans_np/scansNNN.npy (built on the
device from the cut frame: RuntimeParams.surface_callback) and part B runs on DIR: a recording without the dataset's scans_np -- a
rig of one's own -- gets its table rows from the RAW file alone.  They are this build's surfaces, not the ESL dataset's.
With --clouds-from-raw DIR part A also writes every shown frame's per-event point cloud to DIR/pointcloud_live/frameNNNNNN.ply
(the reference's construct_point_cloud on the cut frame's inlier events, built on the device: RuntimeParams.cloud_callback).
With --record-frames FILE.raw part A also writes the frames it shows to FILE.raw -- EVT 3.0 words encoded on the device from the cut
frames, behind the filters, one EXT_TRIGGER word in front of each (RuntimeParams.record_callback, evt3.FrameRecordingWriter) --,
a recording that `--raw FILE.raw --frame-sync ext-trigger --trigger-id 0` replays to the same frames.

Part B -- the accuracy row (eval/x-map-eval.sh:24-72 -> python/eval/compute_depth_x_maps.py:22-133 ->
python/eval/create_evaluation_table.py:84-180): every `<scans>/scans_np/*.npy` time surface -> X-maps depth in camera view on
the evaluation's tables (from_ESL_yaml, rect = 3 x projector, scan downwards) -> `<scans>/x_maps/depth_init/scansNNN.npy`
(+ point clouds as PLY with --point-clouds), then fill rate / RMSE against `<scans>/esl/depth_optim_filtered/*.npy` -- the
table's ground truth, which the reference's ESL optimisation and its two filters write (the filters are not part of this build:
without that directory the depth maps are written and the row is reported as not computable) -- next to the published Book-Duck cell, FR 0.91 / RMSE 0.31 cm.  With --esl-init the
same scans also go through the ESL-init baseline on the device (x_maps_amd/esl_init.py) -> `<scans>/esl/depth_init/scansNNN.npy`
and the table's "ESL (init)" row is printed beside the X-maps one; with --mc3d they go through the MC3D baseline
(x_maps_amd/mc3d.py) -> `<scans>/mc3d/depth/scansNNN.npy` and the "MC3D" and "MC3D (1 sec)" rows are printed too.  With
--esl-optim (which implies --esl-init) every group's depth_init stays on the device and goes straight into ESL's depth optimisation
(x_maps_amd/esl_optim.py) -> `<scans>/esl/depth_optim/scansNNN.npy`, the reference's directory and naming
(compute_depth_esl.py:236).  `esl/depth_optim_filtered` still needs the bilateral and TV filters behind it: nothing is scored
without them, and the report says so.  With --esl-filter (which implies --esl-optim) the optimisation's device buffer goes on
through both filters (x_maps_amd/esl_filter.py) -> `<scans>/esl/depth_optim_filtered/scansNNN.npy` (:247), and every row is then
scored against it.  With --table-on-device the rows whose depth maps are on disk are scored once more, all of them in ONE
device call (x_maps_amd.eval_table.sequence_table: every file read once, no NumPy arithmetic, the same bits every run), and
reported as `table_1_on_device` beside the per-pair rows, which stay as they are.

Tables come from the cv2-free builder (x_maps_amd/calibration.py: rectifying rotations pinned to OpenCV's on this calibration,
map rounding unpinned): a difference from the published numbers on the real data is therefore a finding about that builder or
the decoders, which is what this command exists to surface.  tests/test_gpu_on_arrival.py drives both parts on a recording this
build's own encoder writes; with the real files present (XM_ESL_DATA=/ESL_data/static/seq1) it runs them too."""
from __future__ import annotations

import argparse
import contextlib
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PUBLISHED = {"ms_per_frame": 2.67, "ms_per_frame_sd": 0.31, "hardware": "AMD Ryzen Threadripper PRO 5955WX",
             "seq1_book_duck": {"fill_rate": 0.91, "rmse_cm": 0.31}}


def raw_format(path: str):
    """3, 2, 21 or "dat": what a Prophesee recording holds -- the encoding a RAW file's header declares (one that declares none is
    EVT 3.0), or DAT by its suffix or its header fields.  An encoding this build does not know is a ValueError that names it."""
    from x_maps_amd import dat, evt2, evt21, evt3
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    fields, _ = evt3.split_raw_header(head)
    if dat.is_dat(path, fields):
        return "dat"
    if evt2._is_evt2(fields):
        return 2
    if evt21._is_evt21(fields):
        return 21
    name = evt3.raw_format(fields, "3.0")
    if name not in evt3._FORMAT_NAMES:
        raise ValueError(f"{path}: the header names the encoding {fields.get('evt', fields.get('format'))!r}, which this build does not "
                         f"decode (EVT 2.0, EVT 2.1, EVT 3.0 and DAT are)")
    return 3


def replay_raw(raw, calib, proj_w, proj_h, fps, z_near, z_far, camera_perspective=False, device=0, chunk_words=1 << 20,
               device_ingest=True, keep_frames=0, tables=None, max_chunks=0, scans_dir=None, clouds_dir=None, frame_sync="pauses",
               trigger_id=-1, trigger_edge="rising", trigger_activity_filter=False, record_frames=None):
    """Part A.  -> dict(report), list of (frame checksum, shape) per shown frame, the first `keep_frames` frames
    scans_dir: every shown frame's camera time surface (RuntimeParams.surface_callback: float32, this build's definition) is
    written to <scans_dir>/scans_np/scansNNN.npy, N counting the shown frames from 0 -- what part B reads
    clouds_dir: every shown frame's per-event point cloud (RuntimeParams.cloud_callback) is written to
    <clouds_dir>/pointcloud_live/frameNNNNNN.ply, N counting the same way
    frame_sync: "pauses" (the trigger finder) or "ext_trigger" (RuntimeParams.frame_sync: the frames are cut at the recording's
    EXT_TRIGGER words of channel trigger_id / edge trigger_edge -- one surface / cloud file per trigger-to-trigger frame)
    trigger_activity_filter: frame_sync="ext_trigger" only -- the activity filter in front of the cut (RuntimeParams.ext_trigger_activity_filter)
    record_frames: a .raw file that receives the shown frames as EVT 3.0 words encoded on the device (RuntimeParams.record_callback
    through evt3.FrameRecordingWriter): a recording that --frame-sync ext-trigger --trigger-id 0 replays to the same frames"""
    from x_maps_amd import dat, evt2, evt21, evt3
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    fmt = raw_format(raw)
    mod = {3: evt3, 2: evt2, 21: evt21, "dat": dat}[fmt]
    shown, kept = [], []

    class Window:
        def should_close(self):
            return False

        def show_async(self, img):
            shown.append((img.shape, int(img[::7, ::5].astype(np.uint32).sum())))
            if len(kept) < keep_frames:
                kept.append(np.array(img))

    n_surfaces = [0]
    surface_cb = None
    if scans_dir:
        os.makedirs(os.path.join(scans_dir, "scans_np"), exist_ok=True)

        def surface_cb(surf):
            np.save(os.path.join(scans_dir, "scans_np", scan_name(n_surfaces[0])), surf)
            n_surfaces[0] += 1

    cloud_points = []
    cloud_cb = None
    if clouds_dir:
        os.makedirs(os.path.join(clouds_dir, "pointcloud_live"), exist_ok=True)

        def cloud_cb(cloud):
            write_ply(os.path.join(clouds_dir, "pointcloud_live", cloud_name(len(cloud_points))), cloud)
            cloud_points.append(len(cloud))

    recorder = evt3.FrameRecordingWriter(record_frames, 640, 480) if record_frames else None
    t_setup = time.perf_counter()
    params = RuntimeParams(camera_width=640, camera_height=480, projector_width=proj_w, projector_height=proj_h, projector_fps=fps,
                           z_near=z_near, z_far=z_far, calib=calib, projector_time_map=None, no_frame_dropping=True,
                           camera_perspective=camera_perspective, tables=tables, device=device, device_ingest=device_ingest,
                           surface_callback=surface_cb, cloud_callback=cloud_cb, record_callback=recorder,
                           raw_legacy_halves=fmt == 21 and evt21.raw_legacy_halves(raw), frame_sync=frame_sync,
                           ext_trigger_id=trigger_id, ext_trigger_edge=trigger_edge, ext_trigger_activity_filter=bool(trigger_activity_filter))
    n_words = n_chunks = 0
    with DepthReprojectionProcessor(params, window=Window()) as proc:
        t_setup = time.perf_counter() - t_setup
        push = {3: proc.process_evt3_words, 2: proc.process_evt2_words, 21: proc.process_evt21_words, "dat": proc.process_dat_records}[fmt]
        c0 = time.perf_counter()
        for words in mod.read_raw_words(raw, chunk_words=chunk_words):
            push(words)
            n_words += len(words)
            n_chunks += 1
            if max_chunks and n_chunks >= max_chunks:
                break
        proc.flush()
        dt = time.perf_counter() - c0
        ds = proc._pipe.ingest.device_stats() if proc._pipe.ingest is not None else None
        trig_stats = proc._pipe._trig.stats() if proc._pipe._trig is not None else None
        trig_filter_stats = proc._pipe._trig.filter_stats() if proc._pipe._trig is not None else None
        clouds_lost = int(proc._pipe.stats_printer.counters.get("cloud lost", 0)) if clouds_dir else 0
        records_lost = int(proc._pipe.stats_printer.counters.get("record lost", 0)) if recorder else 0
    if recorder:
        recorder.close()
    rep = {"raw": raw, "format": {3: "EVT 3.0", 2: "EVT 2.0", 21: "EVT 2.1", "dat": "DAT"}[fmt], "words": n_words, "chunks": n_chunks, "chunk_words": chunk_words,
           "path": "external triggers (decode + trigger records + polarity + frames cut at the trigger words + hot path on the GPU)"
                   if frame_sync == "ext_trigger" else
                   "device ingest (decode + filters + trigger finder + hot path on the GPU)" if device_ingest else
                   "host chain (NumPy decoder, filters, trigger finder; one fused GPU call per frame)",
           "setup_seconds": round(t_setup, 3), "replay_seconds": round(dt, 4), "frames_shown": len(shown),
           "ms_per_shown_frame": round(dt / max(len(shown), 1) * 1e3, 4), "reference_published_ms_per_frame": PUBLISHED["ms_per_frame"],
           "frame_shape": list(shown[0][0]) if shown else None}
    if scans_dir:
        rep["scans_from_raw"] = {"dir": os.path.join(scans_dir, "scans_np"), "surfaces_written": n_surfaces[0],
                                 "definition": "this build's surfaces (per pixel the stamp of the cut frame's last event there, t - the "
                                               "frame's first stamp + 1, float32; include/xmaps.h xm_frames_to_time_surfaces), NOT the ESL "
                                               "dataset's scans_np: ESL's own events-to-scan converter is not part of the reference"}
    if clouds_dir:
        rep["clouds_from_raw"] = {"dir": os.path.join(clouds_dir, "pointcloud_live"), "frames": len(cloud_points),
                                  "points": int(sum(cloud_points)), "points_per_frame": cloud_points, "clouds_lost": clouds_lost}
    if recorder:
        rep["record_frames"] = {"file": record_frames, "frames": recorder.frames, "words": recorder.words_written,
                                "frames_below_replay_minimum": recorder.frames_below_replay_minimum,
                                "frames_without_words": recorder.frames_without_words, "records_lost": records_lost,
                                "replay_with": "--frame-sync ext-trigger --trigger-id 0"}
    if trig_stats is not None:
        rep["ext_trigger"] = dict(trig_stats, id=trigger_id, edge=trigger_edge, activity_filter=bool(trigger_activity_filter), filters=trig_filter_stats)
    if ds is not None:
        rep["device"] = ds
        rep["events_behind_the_filters"] = ds["events_appended"]
        rep["Mevents_per_s_behind_the_filters"] = round(ds["events_appended"] / dt / 1e6, 2)
    return rep, shown, kept


def write_ply(path, pts):
    """binary little-endian PLY of an (k, 3) float32 point list (the reference writes its clouds through pyntcloud)"""
    pts = np.ascontiguousarray(pts, dtype="<f4")
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\n"
                 f"property float z\nend_header\n").encode("ascii"))
        f.write(pts.tobytes())


def depth_from_scans(object_dir, eval_calib, proj_w, proj_h, num_scans=0, start_scan=0, point_clouds=False, device=0, tables=None,
                     surfaces_on_device=False, group=8, tables_on_device=False):
    """Part B, first half: compute_depth_x_maps.py:22-133.  -> report
    surfaces_on_device: the scans go through the time-surface entry in groups of `group` (surfaces in, depth maps and clouds out
    in one device call each) instead of one scan at a time through the stage sequence; same files."""
    from x_maps_amd import calibration as C
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    from x_maps_amd.eval_depth import compute_depth_from_time_surface, compute_depths_from_time_surfaces
    from x_maps_amd.x_maps_disparity import XMapsDisparity
    names, err = scan_files(object_dir)
    if err:
        return err
    depth_dir = os.path.join(object_dir, "x_maps", "depth_init")
    cloud_dir = os.path.join(object_dir, "x_maps", "pointcloud_init")
    os.makedirs(depth_dir, exist_ok=True)
    if point_clouds:
        os.makedirs(cloud_dir, exist_ok=True)
    t0 = time.perf_counter()
    if tables is None:
        cp = C.CamProjCalibrationParams.from_ESL_yaml(eval_calib, 640, 480, proj_w, proj_h)
        tables = C.build_eval_tables(cp, device=device, maps_on_device=tables_on_device)
    maps = CamProjMaps(tables, camera_perspective=True, device=device)
    xd = XMapsDisparity(maps)
    t_setup = time.perf_counter() - t0
    per, skipped, filled = [], 0, []
    def results():
        if not surfaces_on_device:
            for (i,) in scan_groups(names, start_scan, num_scans, 1):
                surf = np.load(names[i])
                c0 = time.perf_counter()
                depth, cloud = compute_depth_from_time_surface(maps, xd, surf, want_point_cloud=point_clouds)
                yield i, depth, cloud, time.perf_counter() - c0
            return
        for idx in scan_groups(names, start_scan, num_scans, group):
            surfs = [np.load(names[i]) for i in idx]
            c0 = time.perf_counter()
            out = compute_depths_from_time_surfaces(maps, surfs, want_point_cloud=point_clouds)
            dt = (time.perf_counter() - c0) / len(idx)
            for i, (depth, cloud) in zip(idx, out):
                yield i, depth, cloud, dt

    try:
        for i, depth, cloud, seconds in results():
            if depth is None:  # "Skip camera npy file ... since it is empty" (:132)
                skipped += 1
                continue
            per.append(seconds)
            np.save(os.path.join(depth_dir, scan_name(i)), depth)
            filled.append(float((depth > 0).mean()))
            if point_clouds:
                write_ply(os.path.join(cloud_dir, "scans" + str(i).zfill(3) + ".ply"), cloud)
    finally:
        maps.engine.close()
    return dict(common_keys(names, len(per), skipped, t_setup), ms_per_scan_disparity_to_depth=mean(per, 1e3),
                mean_fraction_of_pixels_with_depth=mean(filled), reference_published_ms_per_frame=PUBLISHED["ms_per_frame"],
                depth_dir=depth_dir)


def scan_files(object_dir):
    """-> (the sorted scans of <object_dir>/scans_np, None), or ([], the report that says there are none)"""
    names = sorted(glob.glob(os.path.join(object_dir, "scans_np", "*.npy")))
    return names, None if names else {"error": f"no camera files found in {os.path.join(object_dir, 'scans_np')}"}


def scan_groups(names, start_scan, num_scans, group):
    """the scans start_scan .. start_scan + num_scans (0 = to the end) in index ranges of at most `group`"""
    last = len(names) if not num_scans else min(len(names), start_scan + num_scans)
    for g0 in range(start_scan, last, max(1, group)):
        yield range(g0, min(last, g0 + max(1, group)))


def cloud_name(i):
    return "frame" + str(i).zfill(6) + ".ply"


def scan_name(i):
    return "scans" + str(i).zfill(3) + ".npy"


def mean(v, scale=1.0):
    return round(float(np.mean(v)) * scale, 4) if v else None


def common_keys(names, processed, skipped, t_setup):
    return {"scans_found": len(names), "scans_processed": processed, "scans_empty": skipped, "setup_seconds": round(t_setup, 3)}


def baseline_from_scans(object_dir, depth_dir, make_object, num_scans, start_scan, group, ms_key, unpinned, **more):
    """What ESL-init and MC3D do alike: every scan of <scans>/scans_np through make_object()'s depths_from_time_surfaces in groups
    of `group` -> depth_dir/scansNNN.npy (an all-zero scan is skipped).  -> report: the common keys, ms_key, the fill, `more`, depth_dir, unpinned"""
    names, err = scan_files(object_dir)
    if err:
        return err
    os.makedirs(depth_dir, exist_ok=True)
    t0 = time.perf_counter()
    per, skipped, filled = [], 0, []
    with make_object() as obj:
        t_setup = time.perf_counter() - t0
        for idx in scan_groups(names, start_scan, num_scans, group):
            surfs = [np.load(names[i]) for i in idx]
            c0 = time.perf_counter()
            out = obj.depths_from_time_surfaces(surfs)
            dt = (time.perf_counter() - c0) / len(idx)
            for i, (depth, _, st) in zip(idx, out):
                if st.n_nonzero == 0:
                    skipped += 1
                    continue
                per.append(dt)
                np.save(os.path.join(depth_dir, scan_name(i)), depth)
                filled.append(float((depth > 0).mean()))
    return dict(common_keys(names, len(per), skipped, t_setup), **{ms_key: mean(per, 1e3)}, mean_fraction_of_pixels_with_depth=mean(filled),
                **more, depth_dir=depth_dir, unpinned=unpinned)


ESL_INIT_UNPINNED = "the int16 rounding of the two remap tables (np.rint) has not been compared with a cv2.remap run"


def esl_init_from_scans(object_dir, eval_calib, proj_w, proj_h, num_scans=0, start_scan=0, device=0, tables=None, group=8,
                        tables_on_device=False):
    """Part B for the baseline: compute_depth_esl.py:179-226 up to depth_init.  Every scan of <scans>/scans_np through
    x_maps_amd.esl_init in groups of `group` -> <scans>/esl/depth_init/scansNNN.npy (an all-zero scan is skipped, :205).  -> report"""
    from x_maps_amd import calibration as C
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    depth_dir = os.path.join(object_dir, "esl", "depth_init")

    def make():
        t = build_esl_init_tables(C.CamProjCalibrationParams.from_ESL_yaml(eval_calib, 640, 480, proj_w, proj_h),
                                  maps_on_device=tables_on_device, device=device) if tables is None else tables
        return EslInit(t, device=device)

    return baseline_from_scans(object_dir, depth_dir, make, num_scans, start_scan, group, "ms_per_scan_depth_init",
                               ESL_INIT_UNPINNED, paper_esl_init_ms_rtx4090=18.99)


def esl_optim_from_scans(object_dir, eval_calib, proj_w, proj_h, num_scans=0, start_scan=0, device=0, init_tables=None,
                         optim_tables=None, group=8, esl_filter=False, tables_on_device=False):
    """Part B for the ground truth's solver: compute_depth_esl.py:204-236.  Every scan of <scans>/scans_np through x_maps_amd.esl_init
    and, chained on the device, x_maps_amd.esl_optim in groups of `group` -> <scans>/esl/depth_init/scansNNN.npy and
    <scans>/esl/depth_optim/scansNNN.npy (an all-zero scan is skipped, :205).  esl_filter: the optimisation's device buffer goes on
    into x_maps_amd.esl_filter (:243-247) -> <scans>/esl/depth_optim_filtered/scansNNN.npy, the table's ground truth.
    -> (the ESL-init report, the optimisation's report[, the filters' report])"""
    import torch
    from x_maps_amd import _native as N
    from x_maps_amd import calibration as C
    from x_maps_amd._group import stats_dtype, surface_group
    from x_maps_amd.esl_init import EslInit, build_esl_init_tables
    from x_maps_amd.esl_optim import EslOptim, build_esl_optim_tables
    from x_maps_amd.esl_filter import EslFilter
    optim_stats, filter_stats = stats_dtype(N.xm_esl_optim_stats), stats_dtype(N.xm_esl_filter_stats)
    names, err = scan_files(object_dir)
    if err:
        return (err, err, err) if esl_filter else (err, err)
    init_dir, optim_dir = os.path.join(object_dir, "esl", "depth_init"), os.path.join(object_dir, "esl", "depth_optim")
    os.makedirs(init_dir, exist_ok=True)
    os.makedirs(optim_dir, exist_ok=True)
    filtered_dir = os.path.join(object_dir, "esl", "depth_optim_filtered")
    if esl_filter:
        os.makedirs(filtered_dir, exist_ok=True)
    t0 = time.perf_counter()
    if init_tables is None or optim_tables is None:
        cp = C.CamProjCalibrationParams.from_ESL_yaml(eval_calib, 640, 480, proj_w, proj_h)
        init_tables = build_esl_init_tables(cp, maps_on_device=tables_on_device, device=device) if init_tables is None else init_tables
        optim_tables = build_esl_optim_tables(cp) if optim_tables is None else optim_tables
    dev = torch.device("cuda", device)
    per_init, per_optim, skipped, filled_init, filled_optim = [], [], 0, [], []
    totals = {k: 0 for k in optim_stats.names[:4]}
    per_filter, outer, trips = [], [], []
    with contextlib.ExitStack() as stack:
        esl, opt = stack.enter_context(EslInit(init_tables, device=device)), stack.enter_context(EslOptim(optim_tables, device=device))
        flt = stack.enter_context(EslFilter(opt.cam_w, opt.cam_h, device=device)) if esl_filter else None
        t_setup = time.perf_counter() - t0
        for idx in scan_groups(names, start_scan, num_scans, group):
            loaded = [(i, np.load(names[i])) for i in idx]
            live = [(i, s) for i, s in loaded if np.count_nonzero(s) > 0]
            skipped += len(loaded) - len(live)
            if not live:
                continue
            grp = surface_group([s for _, s in live], opt.cam_h, opt.cam_w)
            n, dt = len(live), grp.dtype
            d_in = torch.from_numpy(grp).to(dev)
            d_init = torch.empty(grp.shape, dtype=torch.float32, device=dev)
            d_optim = torch.empty(grp.shape, dtype=torch.float32, device=dev)
            d_stats = torch.zeros(n * optim_stats.itemsize, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            c0 = time.perf_counter()
            esl.time_surfaces_device(d_in.data_ptr(), dt, n, d_init.data_ptr())
            c1 = time.perf_counter()
            opt.time_surfaces_device(d_in.data_ptr(), dt, n, d_init.data_ptr(), d_optim.data_ptr(), None, d_stats.data_ptr())
            c2 = time.perf_counter()
            if flt is not None:
                d_filtered = torch.empty(grp.shape, dtype=torch.float64, device=dev)
                d_fstats = torch.zeros(n * filter_stats.itemsize, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                flt.maps_device(d_optim.data_ptr(), n, d_filtered.data_ptr(), None, None, d_fstats.data_ptr())
                c3 = time.perf_counter()
                filtered, fstats = d_filtered.cpu().numpy(), d_fstats.cpu().numpy().view(filter_stats)
            init, optim = d_init.cpu().numpy(), d_optim.cpu().numpy()
            stats = d_stats.cpu().numpy().view(optim_stats)
            for k, (i, _) in enumerate(live):
                np.save(os.path.join(init_dir, scan_name(i)), init[k])
                np.save(os.path.join(optim_dir, scan_name(i)), optim[k])
                if flt is not None:
                    np.save(os.path.join(filtered_dir, scan_name(i)), filtered[k])
                    per_filter.append((c3 - c2) / n)
                    outer.append(int(fstats[k]["n_outer"]))
                    trips.append(int(fstats[k]["sum_itn"]))
                per_init.append((c1 - c0) / n)
                per_optim.append((c2 - c1) / n)
                filled_init.append(float((init[k] > 0).mean()))
                filled_optim.append(float((optim[k] > 0).mean()))
                for key in totals:
                    totals[key] += int(stats[k][key])
    common = common_keys(names, len(per_init), skipped, t_setup)
    rep_init = dict(common, ms_per_scan_depth_init=mean(per_init, 1e3), mean_fraction_of_pixels_with_depth=mean(filled_init),
                    paper_esl_init_ms_rtx4090=18.99, depth_dir=init_dir, unpinned=ESL_INIT_UNPINNED)
    rep_optim = dict(common, ms_per_scan_depth_optim=mean(per_optim, 1e3), mean_fraction_of_pixels_with_depth=mean(filled_optim),
                     depth_dir=optim_dir, **totals,
                     evaluations_per_optimised_pixel=round(totals["n_evals"] / totals["n_optimised"], 2) if totals["n_optimised"] else None,
                     still_needed="esl/depth_optim_filtered, the table's ground truth, is these maps behind cv2.bilateralFilter(., 5, 3, 3) and "
                                  "the pylops TV denoiser (compute_depth_esl.py:243-247); neither filter is part of this build, so "
                                  "nothing is scored from them",
                     unpinned="cv2.undistortPoints, cv2.Rodrigues and cv2.projectPoints have not been compared with a cv2 run")
    if not esl_filter:
        return rep_init, rep_optim
    del rep_optim["still_needed"]
    rep_filter = dict(common, ms_per_scan_filters=mean(per_filter, 1e3), mean_outer_iterations=mean(outer), mean_lsqr_iterations=mean(trips),
                      depth_dir=filtered_dir,
                      unpinned="cv2.bilateralFilter and pylops' SplitBregman (its loop, stacking, stencil, threshold and float32 operator "
                               "dtype) have not been compared with a cv2 / pylops run; scipy's lsqr and the reference's call are pinned")
    return rep_init, rep_optim, rep_filter


def mc3d_from_scans(object_dir, eval_calib, proj_w, proj_h, num_scans=0, start_scan=0, device=0, tables=None, group=8,
                    tables_on_device=False):
    """Part B for the other baseline: mc3d_baseline.py:116-140.  Every scan of <scans>/scans_np through x_maps_amd.mc3d in groups
    of `group` -> <scans>/mc3d/depth/scansNNN.npy (an all-zero scan is skipped, :129).  -> report"""
    from x_maps_amd import calibration as C
    from x_maps_amd.mc3d import Mc3d, build_mc3d_tables
    depth_dir = os.path.join(object_dir, "mc3d", "depth")

    def make():
        t = build_mc3d_tables(C.CamProjCalibrationParams.from_ESL_yaml(eval_calib, 640, 480, proj_w, proj_h),
                              maps_on_device=tables_on_device, device=device) if tables is None else tables
        return Mc3d(t, device=device)

    return baseline_from_scans(object_dir, depth_dir, make, num_scans, start_scan, group, "ms_per_scan_depth",
                               "cv2.medianBlur(., 3) and the float maps of cv2.undistortPoints have not been compared with a cv2 run")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw", help="Prophesee recording (RAW: EVT 3.0 / 2.0 / 2.1, or DAT), e.g. /ESL_data/static/seq1/data.raw")
    ap.add_argument("--bias", help="camera bias file of the recording (recorded in the report; a file replay does not use it)")
    ap.add_argument("--calib", default=os.path.join(ROOT, "..", "reference", "data", "ESL_calib_hhi.yaml"),
                    help="calibration YAML of the live pipe (the reference's data/ESL_calib_hhi.yaml)")
    ap.add_argument("--scans", help="sequence directory holding scans_np/*.npy (and, for the table row, esl/depth_optim_filtered/*.npy)")
    ap.add_argument("--scans-from-raw", metavar="DIR",
                    help="part A also writes every shown frame's camera time surface to DIR/scans_np/scansNNN.npy (this build's "
                         "surfaces, not the ESL dataset's); part B then runs on --scans DIR unless --scans names another directory")
    ap.add_argument("--clouds-from-raw", metavar="DIR",
                    help="part A also writes every shown frame's per-event point cloud to DIR/pointcloud_live/frameNNNNNN.ply")
    ap.add_argument("--record-frames", metavar="FILE.raw",
                    help="part A also writes the frames it shows to FILE.raw as EVT 3.0 words encoded on the device, one EXT_TRIGGER word "
                         "(id 0) in front of each: replays to the same frames with --frame-sync ext-trigger --trigger-id 0")
    ap.add_argument("--frame-sync", choices=("pauses", "ext-trigger"), default="pauses",
                    help="part A: cut the frames at pauses (the trigger finder) or at the recording's EXT_TRIGGER words (a rig with the sync jack wired)")
    ap.add_argument("--trigger-id", type=int, default=-1, help="--frame-sync ext-trigger: the trigger channel (-1: any)")
    ap.add_argument("--trigger-edge", choices=("rising", "falling", "both"), default="rising")
    ap.add_argument("--trigger-activity-filter", action="store_true",
                    help="--frame-sync ext-trigger: the activity filter in front of the cut, as the reference's pipe has it (off by default)")
    ap.add_argument("--eval-calib", help="the ESL dataset's calib.yaml (cam_K, cam_kc, proj_K, proj_kc, R, T) for part B")
    ap.add_argument("--projector-width", type=int, default=1080)
    ap.add_argument("--projector-height", type=int, default=1920)
    ap.add_argument("--projector-fps", type=int, default=60)
    ap.add_argument("--z-near", type=float, default=0.1)
    ap.add_argument("--z-far", type=float, default=1.2)
    ap.add_argument("--camera-perspective", action="store_true")
    ap.add_argument("--compare-host-chain", action="store_true", help="part A a second time through the opt-out host chain, frames compared")
    ap.add_argument("--chunk-words", type=int, default=1 << 20)
    ap.add_argument("--num-scans", type=int, default=0, help="part B: scans to process (0 = all)")
    ap.add_argument("--start-scan", type=int, default=0)
    ap.add_argument("--point-clouds", action="store_true")
    ap.add_argument("--surfaces-on-device", action="store_true",
                    help="part B: the scans go through the time-surface entry in groups (one device call per group)")
    ap.add_argument("--surface-group", type=int, default=8, help="scans per group with --surfaces-on-device")
    ap.add_argument("--esl-init", action="store_true",
                    help="part B: also write <scans>/esl/depth_init/scansNNN.npy (the ESL-init baseline on the device) and print its row")
    ap.add_argument("--esl-optim", action="store_true",
                    help="part B: implies --esl-init; also write <scans>/esl/depth_optim/scansNNN.npy (ESL's depth optimisation, chained "
                         "on the device behind ESL-init; esl/depth_optim_filtered still needs the two filters behind it)")
    ap.add_argument("--esl-filter", action="store_true",
                    help="part B: implies --esl-optim; also write <scans>/esl/depth_optim_filtered/scansNNN.npy (the bilateral filter and "
                         "the TV denoiser, chained on the device behind the optimisation): the ground truth every row is scored against")
    ap.add_argument("--mc3d", action="store_true",
                    help="part B: also write <scans>/mc3d/depth/scansNNN.npy (the MC3D baseline on the device) and print its two rows")
    ap.add_argument("--table-on-device", action="store_true",
                    help="part B: also score every row whose depth maps are on disk in ONE device call (x_maps_amd.eval_table."
                         "sequence_table) and report it as table_1_on_device, when the ground-truth directory exists")
    ap.add_argument("--tables-on-device", action="store_true",
                    help="part B: build every table set (X-maps, ESL-init, MC3D) with its maps on the device (maps_on_device=True: "
                         "x_maps_amd.rig_maps, the same tables bit for bit)")
    ap.add_argument("--min-depth", type=float, default=20)
    ap.add_argument("--max-depth", type=float, default=500, help="eval/x-map-eval.sh:72 passes 500 (the table script's own default is 120)")
    ap.add_argument("--save-frames", type=int, default=0, help="part A: keep the first N BGR frames as frame_NNN.npy beside --out")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", help="write the JSON report here as well")
    a = ap.parse_args(argv)
    if not a.raw and not a.scans:
        ap.error("nothing to do: give --raw and / or --scans")
    if a.scans_from_raw and not a.raw:
        ap.error("--scans-from-raw needs --raw")
    if a.clouds_from_raw and not a.raw:
        ap.error("--clouds-from-raw needs --raw")
    if a.record_frames and not a.raw:
        ap.error("--record-frames needs --raw")
    report = {"published": PUBLISHED}
    if a.raw:
        if a.bias:
            report["bias_file"] = {"path": a.bias, "present": os.path.exists(a.bias), "note": "configures a live camera only"}
        rep, shown, kept = replay_raw(a.raw, a.calib, a.projector_width, a.projector_height, a.projector_fps, a.z_near, a.z_far,
                                      a.camera_perspective, a.device, a.chunk_words, True, a.save_frames, scans_dir=a.scans_from_raw,
                                      clouds_dir=a.clouds_from_raw, frame_sync=a.frame_sync.replace("-", "_"), trigger_id=a.trigger_id,
                                      trigger_edge=a.trigger_edge, trigger_activity_filter=a.trigger_activity_filter,
                                      record_frames=a.record_frames)
        report["replay"] = rep
        if a.scans_from_raw and not a.scans and a.eval_calib:
            a.scans = a.scans_from_raw  # part B on the surfaces part A has just written
        if a.save_frames and a.out:
            for i, f in enumerate(kept):
                np.save(os.path.join(os.path.dirname(os.path.abspath(a.out)), f"frame_{i:03d}.npy"), f)
        if a.compare_host_chain:
            rep_h, shown_h, _ = replay_raw(a.raw, a.calib, a.projector_width, a.projector_height, a.projector_fps, a.z_near, a.z_far,
                                           a.camera_perspective, a.device, a.chunk_words, False, 0)
            report["replay_host_chain"] = rep_h
            report["replay"]["same_frames_as_host_chain"] = bool(shown == shown_h)
    if a.scans:
        if not a.eval_calib:
            ap.error("--scans needs --eval-calib (the ESL dataset's calib.yaml)")
        report["depth_from_scans"] = depth_from_scans(a.scans, a.eval_calib, a.projector_width, a.projector_height, a.num_scans,
                                                      a.start_scan, a.point_clouds, a.device,
                                                      surfaces_on_device=a.surfaces_on_device, group=a.surface_group,
                                                      tables_on_device=a.tables_on_device)
        if "error" not in report["depth_from_scans"]:
            from x_maps_amd.eval_table import x_maps_table_row
            row = x_maps_table_row(a.scans, a.min_depth, a.max_depth, device=a.device)
            row["published_cell_seq1"] = "{fill_rate} & {rmse_cm}".format(**PUBLISHED["seq1_book_duck"])
            report["table_1_row_x_maps"] = row
        if a.esl_filter:
            report["esl_init_from_scans"], report["esl_optim_from_scans"], report["esl_filter_from_scans"] = esl_optim_from_scans(
                a.scans, a.eval_calib, a.projector_width, a.projector_height, a.num_scans, a.start_scan, a.device, group=a.surface_group,
                esl_filter=True, tables_on_device=a.tables_on_device)
            if "table_1_row_x_maps" in report:  # (the ground truth exists only now)
                row = x_maps_table_row(a.scans, a.min_depth, a.max_depth, device=a.device)
                row["published_cell_seq1"] = "{fill_rate} & {rmse_cm}".format(**PUBLISHED["seq1_book_duck"])
                report["table_1_row_x_maps"] = row
        elif a.esl_optim:
            report["esl_init_from_scans"], report["esl_optim_from_scans"] = esl_optim_from_scans(
                a.scans, a.eval_calib, a.projector_width, a.projector_height, a.num_scans, a.start_scan, a.device, group=a.surface_group,
                tables_on_device=a.tables_on_device)
        elif a.esl_init:
            report["esl_init_from_scans"] = esl_init_from_scans(a.scans, a.eval_calib, a.projector_width, a.projector_height,
                                                                a.num_scans, a.start_scan, a.device, group=a.surface_group,
                                                                tables_on_device=a.tables_on_device)
        if a.esl_init or a.esl_optim or a.esl_filter:
            if "error" not in report["esl_init_from_scans"]:
                from x_maps_amd.eval_table import esl_init_table_row
                report["table_1_row_esl_init"] = esl_init_table_row(a.scans, a.min_depth, a.max_depth, device=a.device)
        if a.mc3d:
            report["mc3d_from_scans"] = mc3d_from_scans(a.scans, a.eval_calib, a.projector_width, a.projector_height, a.num_scans,
                                                        a.start_scan, a.device, group=a.surface_group,
                                                        tables_on_device=a.tables_on_device)
            if "error" not in report["mc3d_from_scans"]:
                from x_maps_amd.eval_table import mc3d_table_rows
                rows = mc3d_table_rows(a.scans, a.min_depth, a.max_depth, device=a.device)
                report["table_1_row_mc3d"], report["table_1_row_mc3d_1s"] = rows["mc3d"], rows["mc3d_1s"]
        if a.table_on_device and os.path.isdir(os.path.join(a.scans, "esl", "depth_optim_filtered")):
            from x_maps_amd.eval_table import sequence_table
            report["table_1_on_device"] = sequence_table(a.scans, a.min_depth, a.max_depth, device=a.device)
    txt = json.dumps(report, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    return report


if __name__ == "__main__":
    main()
