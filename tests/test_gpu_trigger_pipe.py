"""-m gpu: RuntimeParams.frame_sync = "ext_trigger" -- the pipe cuts its frames at the recording's EXT_TRIGGER words (decoder with
extraction on -> xm_trigframes -> the group entries on the device buffer) -- on a small synthetic rig (x_maps_amd/synthetic.py)
with frames of a few thousand events, in all three encodings.  The oracle's frames: the word-by-word checker's events and
triggers per chunk (tests/ext_trigger_ref.py), p == 1, cut by TriggerFrameCutter with the reference's MIN_EVENTS_PER_FRAME.
BGR frames == XMapsEngine.process_events on those frames; surfaces and clouds == the group entries on them; every frame is
delivered from inside the call whose words hold its closing trigger.  Then the tool once: --scans-from-raw --frame-sync
ext-trigger on a three-frame rendered recording (in the manner of tests/test_gpu_scans_from_raw.py)."""
import os

import numpy as np
import pytest

import ext_trigger_cases as K
import ext_trigger_ref as R
import frame_cloud_cases as FC
import frame_surface_cases as FS
from test_gpu_on_arrival import _tool, _write_live_yaml
from x_maps_amd import XMapsEngine, evt2, evt21, evt3
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams

pytestmark = pytest.mark.gpu
ENCODE = {3: evt3.encode_evt3, 2: evt2.encode_evt2, 21: evt21.encode_evt21}
N_EVENTS = (3000, 2600, 800, 3400, 2900, 3100)  # per frame, both polarities; the third has fewer than 1000 positive ones: skipped


@pytest.fixture(scope="module")
def tb():
    return FC.add_cloud_tables(S.make_tables(S.C_TINY))


def _stream(fmt):
    """six frames of the synthetic rig, a fifth of the events negative, a trigger in front of every frame and behind the last;
    channel 1 pulses and falling edges in between -> (words, the events as encoded)"""
    parts = [S.make_events(S.C_TINY, frame=f, n=n, p_zero_fraction=0.2, t0=5_000_000 + f * 16_600) for f, n in enumerate(N_EVENTS)]
    evs = np.zeros(sum(N_EVENTS), S.EVENT_CD_DTYPE)
    starts = np.concatenate(([0], np.cumsum(N_EVENTS)))
    for a, p in zip(starts, parts):
        evs[a:a + len(p)] = p
    at, ids, vals = [], [], []
    for f, a in enumerate(starts):
        at += [int(a), int(a), int(min(a + 500, len(evs)))]
        ids += [1, 0, 0]      # another channel's pulse, THE trigger, its falling edge
        vals += [1, 1, 0]
    return X.insert_ext_triggers(ENCODE[fmt](evs), fmt, at, ids, vals), evs


def _params(tb, **kw):
    return RuntimeParams(camera_width=S.C_TINY.cam_w, camera_height=S.C_TINY.cam_h, projector_width=S.C_TINY.proj_w,
                         projector_height=S.C_TINY.proj_h, projector_fps=60, z_near=0.1, z_far=1.2, calib=None, tables=tb, **kw)


class Window:
    def __init__(self, log):
        self.log = log

    def should_close(self):
        return False

    def show_async(self, img):
        self.log.append(("frame", np.array(img)))


def _oracle(fmt, chunks):
    """-> (frames, frames closed per chunk) of the CPU chain"""
    ref, cut = R.machine(fmt), X.TriggerFrameCutter(cap_events=1 << 22, id=0, edge="rising", min_events=1000)
    frames, per_chunk = [], []
    for c in chunks:
        ev, tr = ref.feed(c)
        got = cut.cut_all([X.keep_positive(ev, tr)])
        frames += [e for e, _ in got]
        per_chunk.append(len(got))
    return frames, per_chunk


def _push(proc, fmt, words):
    {3: proc.process_evt3_words, 2: proc.process_evt2_words, 21: proc.process_evt21_words}[fmt](words)


@pytest.mark.parametrize("fmt", K.FMTS)
def test_frames_surfaces_and_clouds_of_the_triggered_chain(tb, fmt):
    words, evs = _stream(fmt)
    cuts = [0, len(words) // 7, len(words) // 3, len(words) // 3 + 1, len(words) // 2, len(words)]  # (one chunk holds several closing triggers)
    chunks = [words[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    frames, per_chunk = _oracle(fmt, chunks)
    assert len(frames) == 5 and max(per_chunk) >= 3 and [len(f) for f in frames] == [int((evs[a:b]["p"] == 1).sum()) for a, b in
                                                                                       zip(np.cumsum((0,) + N_EVENTS[:-1]), np.cumsum(N_EVENTS))
                                                                                       if (evs[a:b]["p"] == 1).sum() > 1000]
    with XMapsEngine(tb) as eng:
        want_bgr = [eng.process_events(f)[1] for f in frames]
        want_surf, _ = eng.frames_to_time_surfaces(frames, "last", np.float32)
        want_cloud = [c for c, _ in eng.frames_to_point_clouds(frames)]
    assert all(len(c) > 100 for c in want_cloud) and len({b.tobytes() for b in want_bgr}) == len(frames)
    log = []
    made = X.TriggeredFrames.created
    params = _params(tb, frame_sync="ext_trigger", ext_trigger_id=0, ext_trigger_cap_events=1 << 15,
                     surface_callback=lambda s: log.append(("surface", np.array(s))), cloud_callback=lambda c: log.append(("cloud", np.array(c))))
    with DepthReprojectionProcessor(params, window=Window(log)) as proc:
        proc._pipe.replay_group = 2  # (several runs inside one call)
        assert proc._pipe.ingest is None
        for c, n_closed in zip(chunks, per_chunk):
            before = sum(1 for k, _ in log if k == "frame")
            _push(proc, fmt, c)
            assert sum(1 for k, _ in log if k == "frame") - before == n_closed  # delivered inside the call that holds the closing trigger
        st = proc._pipe._trig.stats()
        assert st["frames_cut"] == 5 and st["frames_skipped"] == 1 and st["events_dropped_open_frame"] == 0
        with pytest.raises(ValueError):
            proc.process_events(evs[:10])
        with pytest.raises(ValueError):
            proc._pipe.process_dat_records(np.zeros(4, "<u8"))
    assert X.TriggeredFrames.created == made + 1
    assert [k for k, _ in log] == ["surface", "cloud", "frame"] * len(frames)
    for f in range(len(frames)):
        surf, cloud, bgr = (a for _, a in log[3 * f:3 * f + 3])
        assert np.array_equal(bgr, want_bgr[f]), f
        assert surf.dtype == np.float32 and np.array_equal(surf.view(np.uint32), want_surf[f].view(np.uint32)), f
        assert np.array_equal(cloud.view(np.uint32), want_cloud[f].view(np.uint32)), f


def test_reset_and_a_selected_frame_event_filter(tb):
    fmt = 3
    words, _ = _stream(fmt)
    frames, _ = _oracle(fmt, [words])
    # what the host path shows for these frames while the first frame event filter is selected
    want = []
    with DepthReprojectionProcessor(_params(tb, device_ingest=False, activity_filter=False), window=Window(want)) as host:
        host._pipe.select_next_frame_event_filter()
        for f in frames:
            host._pipe.process_ev_frame(f)
    log = []
    with DepthReprojectionProcessor(_params(tb, frame_sync="ext_trigger", ext_trigger_id=0), window=Window(log)) as proc:
        _push(proc, fmt, words[:len(words) // 2])
        n_half = len(log)
        assert 0 < n_half < len(frames)
        proc._pipe.reset()  # the open frame is not a frame; decoder and cutter start a stream
        _push(proc, fmt, words)
        assert len(log) == n_half + len(frames)
        assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(log[:n_half], log[n_half:]))
        proc._pipe.reset()
        proc._pipe.select_next_frame_event_filter()
        del log[:]
        _push(proc, fmt, words)
    assert len(log) == len(want) == len(frames)
    for f in range(len(frames)):
        assert np.array_equal(log[f][1], want[f][1]), f


def test_default_params_still_take_the_ingest(tb):
    words, _ = _stream(3)
    made = X.TriggeredFrames.created
    assert RuntimeParams.__dataclass_fields__["frame_sync"].default == "pauses"
    log = []
    with DepthReprojectionProcessor(_params(tb, activity_filter=False), window=Window(log)) as proc:
        assert proc._pipe.ingest is not None
        proc.process_evt3_words(words)
        assert proc._pipe._trig is None and not proc._pipe._trig_dev and len(proc._pipe._raw_dev) == 1
    assert X.TriggeredFrames.created == made
    with pytest.raises(ValueError):
        DepthReprojectionProcessor(_params(tb, frame_sync="sync jack"), window=Window(log)).__enter__()


def test_the_tool_writes_one_surface_per_triggered_frame(tmp_path, golden_dir):
    from x_maps_amd import calibration as C
    from x_maps_amd import rig
    tool = _tool()
    g = np.load(os.path.join(golden_dir, "g6_esl_calib.npz"))
    live_yaml = tmp_path / "ESL_calib_hhi.yaml"
    _write_live_yaml(live_yaml, g, rig.NEBRA_CAMERA_D)
    cp = C.CamProjCalibrationParams.from_yaml(str(live_yaml), 640, 480, 1080, 1920)
    stream, _ = rig.render_stream(cp, C.build_tables(cp), n_frames=3, row_stride=13, seed=11)
    t_frame = 2_000_000 + 16_600 * np.arange(4)  # render_stream's t_start_us and period_us
    at = np.searchsorted(stream["t"], t_frame)
    words = X.insert_ext_triggers(evt3.encode_evt3(stream), 3, at, id=0, value=1, t=t_frame - 100)
    raw = tmp_path / "data.raw"
    with open(raw, "wb") as f:
        f.write(b"% evt 3.0\n% format EVT3;height=480;width=640\n% geometry 640x480\n% end\n")
        f.write(words.tobytes())
    ev, tr = R.decode(words, 3)
    assert tr["t"].tolist() == (t_frame - 100).tolist() and tr["event_index"].tolist() == at.tolist()
    frames = [e for e, _ in X.TriggerFrameCutter(min_events=1000).cut_all([X.keep_positive(ev, tr)])]
    assert len(frames) == 3 and all(len(f) > 1000 for f in frames)
    out_dir = tmp_path / "from_raw"
    rep = tool.main(["--raw", str(raw), "--calib", str(live_yaml), "--scans-from-raw", str(out_dir), "--frame-sync", "ext-trigger",
                     "--trigger-id", "0", "--chunk-words", str(1 << 15)])
    a = rep["replay"]
    assert a["frames_shown"] == 3 == a["scans_from_raw"]["surfaces_written"] and a["path"].startswith("external triggers")
    assert a["ext_trigger"]["frames_cut"] == 3 and a["ext_trigger"]["triggers_selected"] == 4 and "device" not in a
    names = sorted(os.listdir(out_dir / "scans_np"))
    assert names == [tool.scan_name(i) for i in range(3)]
    for i, (n, evs) in enumerate(zip(names, frames)):
        s = np.load(out_dir / "scans_np" / n)
        want, st = FS.oracle(evs, 640, 480, "last", np.float32)
        assert s.dtype == np.float32 and np.array_equal(s.view(np.uint32), want.view(np.uint32)), i
        assert st["n_pixels"] > 1000
