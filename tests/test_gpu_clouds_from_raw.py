"""-m gpu: tools/run_esl_on_arrival.py --clouds-from-raw -- part A writes every shown frame's per-event point cloud to
DIR/pointcloud_live/frameNNNNNN.ply.

The recording is written by this build's own encoder, as in tests/test_gpu_scans_from_raw.py.  Expected frames never come from the
package's device path: the host decoder's events of every chunk go through oracle/ingest_oracle's polarity filter, activity filter
and trigger finder; tests/frame_cloud_cases.oracle gives each cut frame's row count and (to the CPU oracle's tolerance) its rows."""
import os

import numpy as np
import pytest

import frame_cloud_cases as K
import ingest_oracle as IO
from test_gpu_on_arrival import _tool, _write_live_yaml
from x_maps_amd import synthetic as S

pytestmark = pytest.mark.gpu
CHUNK_WORDS = 1 << 16


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode("ascii").splitlines() if ln.startswith("element vertex")][0].split()[-1])
    pts = np.frombuffer(body, "<f4").reshape(-1, 3)
    assert len(pts) == n
    return pts


def test_part_a_writes_one_ply_per_shown_frame(tmp_path, golden_dir):
    from x_maps_amd import calibration as C
    from x_maps_amd import evt3, rig
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    live_yaml = tmp_path / "ESL_calib_hhi.yaml"
    _write_live_yaml(live_yaml, g, rig.NEBRA_CAMERA_D)
    cp = C.CamProjCalibrationParams.from_yaml(str(live_yaml), 640, 480, 1080, 1920)
    tables = C.build_tables(cp)
    stream, _ = rig.render_stream(cp, tables, n_frames=5, row_stride=13, seed=11)
    lead = np.zeros(2, S.EVENT_CD_DTYPE)  # (the trigger finder's first pause: see tests/test_gpu_on_arrival.py)
    lead["t"] = stream["t"][0] - np.array([1600, 1500])
    lead["x"], lead["y"], lead["p"] = [100, 101], [100, 100], 1
    both = np.zeros(len(stream) + 2, S.EVENT_CD_DTYPE)
    both[:2], both[2:] = lead, stream
    raw = tmp_path / "data.raw"
    evt3.write_raw(str(raw), both)
    dec, act, tf = evt3.Evt3Decoder(), IO.ActivityFilterC(640, 480, int(1e6 / 60)), IO.TriggerFinderOracle(60)
    for words in evt3.read_raw_words(str(raw), chunk_words=CHUNK_WORDS):
        tf.process_events(act.process(IO.polarity_filter(dec.decode(words))))
    frames = tf.frames
    assert len(frames) >= 3 and all(len(f) > 1000 for f in frames)

    out_dir = tmp_path / "from_raw"
    rep = tool.main(["--raw", str(raw), "--calib", str(live_yaml), "--clouds-from-raw", str(out_dir), "--chunk-words", str(CHUNK_WORDS)])
    a = rep["replay"]
    c = a["clouds_from_raw"]
    assert a["frames_shown"] == len(frames) == c["frames"] and c["clouds_lost"] == 0
    names = sorted(os.listdir(out_dir / "pointcloud_live"))
    assert names == [tool.cloud_name(i) for i in range(len(frames))] and names[0] == "frame000000.ply"
    clouds = [_read_ply(out_dir / "pointcloud_live" / n) for n in names]
    assert [len(p) for p in clouds] == c["points_per_frame"] and sum(len(p) for p in clouds) == c["points"] > 1000
    tb = dict(tables)
    for i, (pts, evs) in enumerate(zip(clouds, frames)):
        o = K.oracle(tb, evs)
        assert len(pts) == o["stats"]["n_inliers"] > 100, i
        fin = np.isfinite(o["cloud"])
        assert np.array_equal(np.isfinite(pts), fin), i
        assert np.allclose(pts[fin], o["cloud"][fin], rtol=1e-5, atol=1e-5), i
