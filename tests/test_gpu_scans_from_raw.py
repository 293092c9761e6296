"""-m gpu: tools/run_esl_on_arrival.py --scans-from-raw -- a RAW recording alone is enough for part B: part A writes every shown
frame's camera time surface to DIR/scans_np/scansNNN.npy, part B runs on DIR.

The recording is written by this build's own encoder, as in tests/test_gpu_on_arrival.py.  Expected surfaces never come from the
package's device path: the host decoder's events of every chunk go through oracle/ingest_oracle's polarity filter, activity
filter and trigger finder, and tests/frame_surface_cases.oracle turns each cut frame into its surface."""
import os

import numpy as np
import pytest

import frame_surface_cases as K
import ingest_oracle as IO
from test_gpu_on_arrival import _tool, _write_esl_yaml, _write_live_yaml
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
CHUNK_WORDS = 1 << 16


def test_part_a_writes_the_surfaces_part_b_reads(tmp_path, golden_dir):
    from x_maps_amd import calibration as C
    from x_maps_amd import evt3, rig
    from x_maps_amd.cam_proj_calibration import CamProjMaps
    from x_maps_amd.eval_depth import compute_depths_from_time_surfaces
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    live_yaml, esl_yaml = tmp_path / "ESL_calib_hhi.yaml", tmp_path / "calib.yaml"
    _write_live_yaml(live_yaml, g, rig.NEBRA_CAMERA_D)
    _write_esl_yaml(esl_yaml, g, rig.NEBRA_CAMERA_D)
    cp = C.CamProjCalibrationParams.from_yaml(str(live_yaml), 640, 480, 1080, 1920)
    stream, _ = rig.render_stream(cp, C.build_tables(cp), n_frames=6, row_stride=13, seed=11)
    lead = np.zeros(2, S.EVENT_CD_DTYPE)  # (the trigger finder's first pause: see tests/test_gpu_on_arrival.py)
    lead["t"] = stream["t"][0] - np.array([1600, 1500])
    lead["x"], lead["y"], lead["p"] = [100, 101], [100, 100], 1
    both = np.zeros(len(stream) + 2, S.EVENT_CD_DTYPE)
    both[:2], both[2:] = lead, stream
    raw = tmp_path / "data.raw"
    evt3.write_raw(str(raw), both)
    # the CPU chain on the packets the pipe sees: one per chunk of words
    dec, act, tf = evt3.Evt3Decoder(), IO.ActivityFilterC(640, 480, int(1e6 / 60)), IO.TriggerFinderOracle(60)
    for words in evt3.read_raw_words(str(raw), chunk_words=CHUNK_WORDS):
        tf.process_events(act.process(IO.polarity_filter(dec.decode(words))))
    frames = tf.frames
    assert len(frames) >= 3 and all(len(f) > 1000 for f in frames)

    out_dir = tmp_path / "from_raw"
    rep = tool.main(["--raw", str(raw), "--calib", str(live_yaml), "--scans-from-raw", str(out_dir), "--eval-calib", str(esl_yaml),
                     "--surfaces-on-device", "--chunk-words", str(CHUNK_WORDS)])
    a = rep["replay"]
    assert a["frames_shown"] == len(frames) == a["scans_from_raw"]["surfaces_written"]
    assert "this build's surfaces" in a["scans_from_raw"]["definition"] and "NOT the ESL dataset's" in a["scans_from_raw"]["definition"]
    names = sorted(os.listdir(out_dir / "scans_np"))
    assert names == [tool.scan_name(i) for i in range(len(frames))]  # one file per shown frame, scan_name's naming
    surfs = [np.load(out_dir / "scans_np" / n) for n in names]
    for i, (s, evs) in enumerate(zip(surfs, frames)):
        want, st = K.oracle(evs, 640, 480, "last", np.float32)
        assert s.dtype == np.float32 and np.array_equal(s.view(np.uint32), want.view(np.uint32)), i
        assert st["n_index_errors"] == 0 and st["n_pixels"] > 1000
    # part B ran on the directory part A wrote: its depth maps == the group entry on the same arrays
    b = rep["depth_from_scans"]
    assert b["scans_found"] == b["scans_processed"] == len(frames) and b["scans_empty"] == 0
    maps = CamProjMaps(C.build_eval_tables(C.CamProjCalibrationParams.from_ESL_yaml(str(esl_yaml), 640, 480, 1080, 1920)), camera_perspective=True)
    try:
        want = compute_depths_from_time_surfaces(maps, surfs)
    finally:
        maps.engine.close()
    assert any((d > 0).sum() > 100 for d, _ in want)
    for i, (depth, _) in enumerate(want):
        got = np.load(out_dir / "x_maps" / "depth_init" / tool.scan_name(i))
        assert np.array_equal(got.view(np.uint32), depth.view(np.uint32)), i
