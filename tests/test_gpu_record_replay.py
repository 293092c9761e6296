"""-m gpu: the closed loop.  A pause-cut session recorded through RuntimeParams.record_callback and evt3.FrameRecordingWriter -- the
frames' EVT 3.0 words encoded on the device, one EXT_TRIGGER word in front of each -- is the input the frame_sync="ext_trigger"
chain takes, and every frame comes back bit for bit.  No fixture from outside: both halves are this build's.

The stream: ingest_helpers._tiny_stream(12, seed=6) on S.C_TINY's 64 x 48 camera, shifted so that its stamps start above 2^24 and
cross 2^25 inside the session: the recording's stamps come back shifted by 2^24 (its first loop counts as 0), and its 24-bit
time wraps once on the way."""
import functools
import os

import numpy as np
import pytest

import evt3_record_cases as K
from ingest_helpers import Window, _packets, _processor_params, _shifted, _tiny_stream
from test_gpu_on_arrival import _tool, _write_live_yaml
from x_maps_amd import XMapsEngine, evt3
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor
from x_maps_amd.ingest import DeviceIngest

pytestmark = pytest.mark.gpu

CFG = S.C_TINY
SHIFT = 31_450_000  # the stream starts at 33 450 000 > 2^24 and passes 2^25 = 33 554 432 about 0.1 s in


@functools.lru_cache(maxsize=None)
def _tables():
    return S.make_tables(CFG)


@functools.lru_cache(maxsize=None)
def _session():
    stream = _shifted(_tiny_stream(12, seed=6), SHIFT)
    assert stream["t"][0] > 1 << 24 and stream["t"][0] < 1 << 25 < stream["t"][-1]
    return _packets(stream, int(1e6 / 60 / 4))


def _record(path, **kw):
    """the session through DepthReprojectionProcessor with record_callback -> (shown BGR frames, the writer, [(words, stats)])"""
    shown, recs = [], []
    with evt3.FrameRecordingWriter(path, CFG.cam_w, CFG.cam_h) as rec:
        def cb(words, st):
            assert len(shown) == len(recs)  # in front of the frame's frame_callback
            recs.append((np.array(words), st))
            rec(words, st)
        with DepthReprojectionProcessor(_processor_params(_tables(), record_callback=cb, **kw), window=Window(shown)) as proc:
            for p in _session():
                proc.process_events(p)
    return [np.array(f) for f in shown], rec, recs


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """the first run, on default RuntimeParams (device ingest, activity filter): computed once"""
    path = str(tmp_path_factory.mktemp("rec") / "session.raw")
    shown, rec, recs = _record(path)
    assert len(shown) == len(recs) == rec.frames >= 4 and rec.frames_below_replay_minimum == 0 == rec.frames_without_words
    assert all(st.n_events > 1000 and st.t_first > 1 << 24 for _, st in recs) and len({f.tobytes() for f in shown}) == len(shown)
    return path, shown, recs


def test_the_recording_replays_to_the_same_frames(recorded):
    path, shown, recs = recorded
    words = np.concatenate(list(evt3.read_raw_words(path)))
    again = []
    with DepthReprojectionProcessor(_processor_params(_tables(), frame_sync="ext_trigger", ext_trigger_id=0), window=Window(again)) as proc:
        assert proc._pipe.ingest is None
        for a in range(0, len(words), 5001):  # (chunks that end inside frames)
            proc.process_evt3_words(words[a:a + 5001])
        st = proc._pipe._trig.stats()
    assert st["frames_cut"] == len(shown) and st["frames_skipped"] == 0 and st["events_dropped_open_frame"] == 0
    assert len(again) == len(shown)
    for i, (a, b) in enumerate(zip(again, shown)):
        assert a.shape == b.shape and np.array(a).tobytes() == b.tobytes(), i


def test_the_recording_holds_the_frames_the_session_processed(recorded):
    """the file through the host decoder and cutter: every frame's events are what the record stage encoded (stamps shifted by
    2^24), and the words are the host encoder's on them"""
    path, shown, recs = recorded
    words = np.concatenate(list(evt3.read_raw_words(path)))
    got = X.TriggerFrameCutter(id=0, min_events=1000).cut_all([X.ExtTriggerExtractor(3).extract(words)])
    assert len(got) == len(recs)
    for i, ((ev, trig), (w, st)) in enumerate(zip(got, recs)):
        ev = ev.copy()
        ev["t"] += 1 << 24
        assert (len(ev), int(ev["t"][0]), int(ev["t"][-1])) == (st.n_events, st.t_first, st.t_last), i
        assert int(trig["t"]) + (1 << 24) == st.t_first and (ev["p"] == 1).all(), i
        assert np.array_equal(K.oracle(ev)[0], w) and st.n_words == len(w), i


def test_the_host_chain_records_the_same_words(recorded, tmp_path):
    path, shown, recs = recorded
    shown_h, rec_h, recs_h = _record(str(tmp_path / "host.raw"), device_ingest=False)
    assert len(recs_h) == len(recs) and rec_h.frames == len(recs)
    for i, ((w, st), (wh, sth)) in enumerate(zip(recs, recs_h)):
        assert np.array_equal(w, wh) and wh.dtype == np.uint16 and st == sth, i
    assert open(path, "rb").read() == open(str(tmp_path / "host.raw"), "rb").read()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(shown, shown_h))


def test_depth_frames_come_back_bit_for_bit(tmp_path):
    """where depth is requested: DeviceIngest's frames (depth + BGR) against the engine on the frames recut from the recording"""
    path = str(tmp_path / "depth.raw")
    with XMapsEngine(_tables()) as eng, DeviceIngest(eng, 60, activity_filter=True, capacity_events=1 << 13, max_packet_events=1 << 11,
                                                      result_ring=16) as ing:
        ing.set_record_output(True, True, 1 << 14)
        for p in _session():
            ing.push(p)
        ing.flush()
        frames = ing.poll()
        with evt3.FrameRecordingWriter(path, CFG.cam_w, CFG.cam_h) as rec:
            for fr in frames:
                rec(*ing.record(fr.seq))
        words = np.concatenate(list(evt3.read_raw_words(path)))
        got = X.TriggerFrameCutter(id=0, min_events=1000).cut_all([X.ExtTriggerExtractor(3).extract(words)])
        assert len(got) == len(frames) >= 4
        for i, ((ev, _), fr) in enumerate(zip(got, frames)):
            depth, bgr, _ = eng.process_events(ev)
            assert depth.tobytes() == fr.depth.tobytes() and bgr.tobytes() == fr.bgr.tobytes(), i


def test_the_tool_records_the_frames_it_shows(tmp_path, golden_dir):
    """tools/run_esl_on_arrival.py --record-frames on a small rendered recording, then the tool again on what it wrote"""
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    live_yaml = tmp_path / "ESL_calib_hhi.yaml"
    _write_live_yaml(live_yaml, g, rig.NEBRA_CAMERA_D)
    cp = C.CamProjCalibrationParams.from_yaml(str(live_yaml), 640, 480, 1080, 1920)
    stream, _ = rig.render_stream(cp, C.build_tables(cp), n_frames=6, row_stride=13, seed=11, t_start_us=2_000_000 + SHIFT)
    lead = np.zeros(2, S.EVENT_CD_DTYPE)  # (two events in front of the first scan give the trigger finder its first pause)
    lead["t"] = stream["t"][0] - np.array([1600, 1500])
    lead["x"], lead["y"], lead["p"] = [100, 101], [100, 100], 1
    both = np.zeros(len(stream) + 2, S.EVENT_CD_DTYPE)
    both[:2], both[2:] = lead, stream
    raw, out = tmp_path / "data.raw", tmp_path / "a" / "report.json"
    os.makedirs(out.parent)
    evt3.write_raw(str(raw), both)
    rec_file = tmp_path / "frames.raw"
    rep = tool.main(["--raw", str(raw), "--calib", str(live_yaml), "--record-frames", str(rec_file), "--chunk-words", str(1 << 16),
                     "--save-frames", "8", "--out", str(out)])
    a = rep["replay"]
    r = a["record_frames"]
    assert a["frames_shown"] == r["frames"] >= 2 and r["frames_without_words"] == 0 == r["records_lost"] == r["frames_below_replay_minimum"]
    assert r["words"] * 2 + len(evt3._raw_header(640, 480)) == os.path.getsize(rec_file)
    out2 = tmp_path / "b" / "report.json"
    os.makedirs(out2.parent)
    rep2 = tool.main(["--raw", str(rec_file), "--calib", str(live_yaml), "--frame-sync", "ext-trigger", "--trigger-id", "0",
                      "--chunk-words", str(1 << 15), "--save-frames", "8", "--out", str(out2)])
    b = rep2["replay"]
    assert b["frames_shown"] == a["frames_shown"] and b["ext_trigger"]["frames_skipped"] == 0
    for i in range(a["frames_shown"]):
        assert np.load(out.parent / f"frame_{i:03d}.npy").tobytes() == np.load(out2.parent / f"frame_{i:03d}.npy").tobytes(), i
