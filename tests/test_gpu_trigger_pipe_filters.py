"""-m gpu: the triggered chain of the pipe (RuntimeParams.frame_sync = "ext_trigger") with its two filters --
ext_trigger_activity_filter (polarity -> activity -> cut, on the device inside the append) and device_frame_filters (key E: the
run of ready frames is filtered where it lies) -- on stream A (tests/trigger_filter_cases.py) in the five uneven chunks of
tests/test_gpu_trigger_pipe.py.  Expected frames: the CPU chain's, rendered by XMapsEngine.process_events; surfaces and clouds:
the group entries on them.  Then the tool once with --trigger-activity-filter."""
import os

import numpy as np
import pytest

import frame_cloud_cases as FC
import frame_surface_cases as FS
import trigger_filter_cases as TC
from test_gpu_on_arrival import _tool, _write_live_yaml
from x_maps_amd import XMapsEngine, evt3
from x_maps_amd import ext_trigger as X
from x_maps_amd import synthetic as S
from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams

pytestmark = pytest.mark.gpu
CUT = dict(cap_events=1 << 22, id=0, edge="rising", min_events=1000)
FMT = 3


@pytest.fixture(scope="module")
def tb():
    return FC.add_cloud_tables(S.make_tables(S.C_TINY))


def _params(tb, fps=60, **kw):
    return RuntimeParams(camera_width=S.C_TINY.cam_w, camera_height=S.C_TINY.cam_h, projector_width=S.C_TINY.proj_w,
                         projector_height=S.C_TINY.proj_h, projector_fps=fps, z_near=0.1, z_far=1.2, calib=None, tables=tb,
                         frame_sync="ext_trigger", ext_trigger_id=0, ext_trigger_cap_events=1 << 15, **kw)


class Window:
    def __init__(self, log):
        self.log = log

    def should_close(self):
        return False

    def show_async(self, img):
        self.log.append(("frame", np.array(img)))


def _chunks():
    return TC.uneven_chunks(TC.stream_a(FMT)[0])


def _expected(thresh):
    return TC.expected(TC.decoded_chunks(FMT, _chunks()), thresh, **CUT)


def _n_frames(log):
    return sum(1 for k, _ in log if k == "frame")


def test_the_activity_filter_in_front_of_the_cut(tb):
    """projector_fps = 2000: T = 500.  Frames, surfaces and clouds are the engine's on the oracle's frames, each delivered inside the
    call that holds its closing trigger."""
    want = _expected(500)
    frames = [f for f, _ in want["frames"]]
    assert [len(f) for f in frames] == [1876, 1514, 2228, 1804, 1928] and max(want["per_chunk"]) >= 3
    with XMapsEngine(tb) as eng:
        want_bgr = [eng.process_events(f)[1] for f in frames]
        want_surf, _ = eng.frames_to_time_surfaces(frames, "last", np.float32)
        want_cloud = [c for c, _ in eng.frames_to_point_clouds(frames)]
        plain_bgr = [eng.process_events(f)[1] for f, _ in _expected(None)["frames"]]
    assert not any(np.array_equal(a, b) for a, b in zip(want_bgr, plain_bgr))  # (the filter changes every frame shown)
    log = []
    params = _params(tb, fps=2000, ext_trigger_activity_filter=True, surface_callback=lambda s: log.append(("surface", np.array(s))),
                     cloud_callback=lambda c: log.append(("cloud", np.array(c))))
    with DepthReprojectionProcessor(params, window=Window(log)) as proc:
        proc._pipe.replay_group = 2
        for c, n_closed in zip(_chunks(), want["per_chunk"]):
            before = _n_frames(log)
            proc.process_evt3_words(c)
            assert _n_frames(log) - before == n_closed
        st, fst = proc._pipe._trig.stats(), proc._pipe._trig.filter_stats()
    assert st["frames_cut"] == 5 and st["frames_skipped"] == 1 and st["events_kept"] == 9586 == fst["events_active"]
    assert fst["events_positive"] == TC.N_POSITIVE and fst["chunks_sequential"] == want["n_sequential"] == 4
    assert [k for k, _ in log] == ["surface", "cloud", "frame"] * 5
    for f in range(5):
        surf, cloud, bgr = (a for _, a in log[3 * f:3 * f + 3])
        assert np.array_equal(bgr, want_bgr[f]), f
        assert np.array_equal(surf.view(np.uint32), want_surf[f].view(np.uint32)), f
        assert np.array_equal(cloud.view(np.uint32), want_cloud[f].view(np.uint32)), f


def test_min_events_applies_behind_the_filter(tb):
    """projector_fps = 5000: T = 200 -- four frames shown, two skipped (the frame of 991 kept events among them); activity_strict
    is T - 1, as on the ingest"""
    for strict, thresh in ((False, 200), (True, 199)):
        want = _expected(thresh)
        with XMapsEngine(tb) as eng:
            want_bgr = [eng.process_events(f)[1] for f, _ in want["frames"]]
        log = []
        with DepthReprojectionProcessor(_params(tb, fps=5000, ext_trigger_activity_filter=True, activity_strict=strict), window=Window(log)) as proc:
            for c in _chunks():
                proc.process_evt3_words(c)
            st = proc._pipe._trig.stats()
        assert (st["frames_cut"], st["frames_skipped"]) == (4, 2) == (len(want_bgr), 2)
        assert all(np.array_equal(a, b) for (_, a), b in zip(log, want_bgr)) and len(log) == 4


def test_default_parameters_and_activity_filter_false_give_todays_frames(tb):
    want = _expected(None)
    with XMapsEngine(tb) as eng:
        want_bgr = [eng.process_events(f)[1] for f, _ in want["frames"]]
    assert RuntimeParams.__dataclass_fields__["ext_trigger_activity_filter"].default is False
    for kw in ({}, {"ext_trigger_activity_filter": True, "activity_filter": False}, {"device_frame_filters": True}):
        log = []
        with DepthReprojectionProcessor(_params(tb, **kw), window=Window(log)) as proc:
            for c in _chunks():
                proc.process_evt3_words(c)
            assert proc._pipe._trig.filter_stats() == dict.fromkeys(X.TriggeredFrames.FILTER_COUNTERS, 0)
        assert len(log) == len(want_bgr) == 5 and all(np.array_equal(a, b) for (_, a), b in zip(log, want_bgr)), kw


def test_key_e_keeps_the_frames_on_the_device(tb, monkeypatch):
    """Each of the four filters selected (E pressed once more per pass): device_frame_filters shows the BGR frames of the download
    path on the same words, and downloads nothing."""
    calls = []
    real = X.TriggeredFrames.download
    monkeypatch.setattr(X.TriggeredFrames, "download", lambda self, *a: (calls.append(1), real(self, *a))[1])
    shown = {}
    for on_device in (False, True):
        for presses in (1, 2, 3, 4):
            log = []
            surf = []
            with DepthReprojectionProcessor(_params(tb, device_frame_filters=on_device, surface_callback=lambda s: surf.append(np.array(s))),
                                            window=Window(log)) as proc:
                proc._pipe.replay_group = 3
                for _ in range(presses):
                    proc._pipe.select_next_frame_event_filter()
                name = type(proc._pipe.ev_filter_proc.selected_filter()).__name__
                n_calls = len(calls)
                for c in _chunks():
                    proc.process_evt3_words(c)
                assert (len(calls) == n_calls) == on_device, (name, on_device)
                if on_device:
                    fst = proc._pipe._trig.filter_stats()
                    assert fst["frames_filtered"] == 5 and 0 < fst["events_after_frame_filter"] < 0.8 * TC.N_POSITIVE
            assert len(log) == 5 == len(surf)
            shown[(on_device, name)] = ([a for _, a in log], surf)
    names = sorted({n for _, n in shown})
    assert len(names) == 4
    plain = None
    for n in names:
        (host_bgr, host_surf), (dev_bgr, dev_surf) = shown[(False, n)], shown[(True, n)]
        assert all(np.array_equal(a, b) for a, b in zip(host_bgr, dev_bgr)), n
        assert all(np.array_equal(a, b) for a, b in zip(host_surf, dev_surf)), n  # (the cut frames', in front of the filter)
        plain = plain or host_surf
        assert all(np.array_equal(a, b) for a, b in zip(plain, host_surf))


def test_the_tool_with_the_trigger_activity_filter(tmp_path, golden_dir):
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
    chunk_words = 1 << 15
    chunks = [words[a:a + chunk_words] for a in range(0, len(words), chunk_words)]
    ch = TC.Chain(int(1e6 / 60), c_form=True, cam=(640, 480), min_events=1000)
    frames = []
    for ev, tr in TC.decoded_chunks(3, chunks):
        ch.feed(ev, tr)
        frames += [e for e, _ in ch.drain()]
    plain = TC.Chain(None, cam=(640, 480), min_events=1000)
    for ev, tr in TC.decoded_chunks(3, chunks):
        plain.feed(ev, tr)
    assert len(frames) == 3 and 0 < ch.n_active < ch.n_positive == plain.cut.stats["events_kept"]
    out_dir = tmp_path / "from_raw"
    rep = tool.main(["--raw", str(raw), "--calib", str(live_yaml), "--scans-from-raw", str(out_dir), "--frame-sync", "ext-trigger",
                     "--trigger-id", "0", "--chunk-words", str(chunk_words), "--trigger-activity-filter"])
    a = rep["replay"]
    assert a["frames_shown"] == 3 == a["scans_from_raw"]["surfaces_written"]
    assert a["ext_trigger"]["activity_filter"] is True and a["ext_trigger"]["events_kept"] == ch.n_active
    assert a["ext_trigger"]["filters"]["events_active"] == ch.n_active and a["ext_trigger"]["filters"]["events_positive"] == ch.n_positive
    for i, evs in enumerate(frames):
        s = np.load(out_dir / "scans_np" / tool.scan_name(i))
        want, _ = FS.oracle(evs, 640, 480, "last", np.float32)
        assert np.array_equal(s.view(np.uint32), want.view(np.uint32)), i
