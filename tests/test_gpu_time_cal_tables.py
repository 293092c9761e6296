"""GPU: a calibrated projector time map on its way into the tables -- build_tables(projector_time_map=) against the same call on
the map rectified by hand, with and without maps_on_device -- and the calibration end to end: frames of events -> add_frames ->
mean -> solve against the oracle of tests/time_cal_cases.py on the surfaces tests/frame_surface_cases.oracle makes of the same
frames; tools/calibrate_time_map.py on a recording this build's own EVT 3.0 encoder writes, and a DepthReprojectionProcessor on
the file it leaves."""
import importlib.util
import os

import numpy as np
import pytest

import frame_surface_cases as K
import ingest_oracle as IO
import rig_maps_cases as RC
import time_cal_cases as T
from x_maps_amd import XMapsEngine
from x_maps_amd import calibration as cal
from x_maps_amd import time_map_calibration as TMC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_array(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return RC.bits_equal(a, b) if a.dtype == np.float32 else bool(np.array_equal(a, b))


def _same_dict(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert isinstance(got[k], np.ndarray) and _same_array(got[k], w), k
        else:
            assert type(got[k]) is type(w) and got[k] == w, k


def _curved_map(cp):
    """an unrectified [proj_h][proj_w] float32 time map that is not the linear one"""
    W, H = cp.projector_width, cp.projector_height
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return (((u * H + v) / (W * H)) ** 1.3).astype(np.float32)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "maps_on_device"])
@pytest.mark.parametrize("rig,builder", [("L", "build_tables"), ("S", "build_eval_tables")])
def test_build_tables_rectifies_the_projector_time_map(rig, builder, on_device):
    cp, fn = RC.params(rig), getattr(cal, builder)
    kw = RC.TABLE_KW[rig]
    M = _curved_map(cp)
    plain = fn(cp)
    size = (cp.rect_image_width, cp.rect_image_height)
    pmx, pmy = cal.init_undistort_rectify_map(cp.projector_K, np.zeros(5) if kw["zero_undistort_proj_map"] else cp.projector_D,
                                              plain["R2"], plain["P2"], size)
    rect = cal.remap_nearest(M, pmx, pmy, kw["time_map_border"])
    want = fn(cp, projector_time_map_rectified=rect, maps_on_device=on_device)
    got = fn(cp, projector_time_map=M, maps_on_device=on_device)
    _same_dict(got, want)
    assert _same_array(got["time_map_rect"], rect) and not np.array_equal(got["proj_x_map"], plain["proj_x_map"])
    with pytest.raises(ValueError, match="one"):
        fn(cp, projector_time_map=M, projector_time_map_rectified=rect)
    with pytest.raises(ValueError, match="must be"):
        fn(cp, projector_time_map=M[:-1])


# ---- frames of events -> the map ----------------------------------------------------------------------------------------------
def test_frames_of_events_to_the_map():
    surf = T.render(T.CAM, T.PROJ, T.QUAD_PERSP, T.curved_time(T.PROJ), 6, span=9000.0, drop=0.25, seed=21)
    frames = [T.events_from_surface(s, 1_000_000 + 16_600 * k) for k, s in enumerate(surf)]
    o = T.Oracle(T.CAM)
    o.add([K.oracle(f, T.CAM[0], T.CAM[1], "first", np.float64)[0] for f in frames])
    want = T.solve(o, T.min_count_for(0.5, o.n_used), T.PROJ)
    assert o.n_used == 6 and want["n_core"] > 500
    with XMapsEngine(K.rig_tables(*T.CAM)) as eng, TMC.TimeMapCalibrator(T.CAM) as c:
        c.add_frames(eng, frames, max_group=4)  # (two calls: 4 + 2)
        c.mean(0.5)
        got, st = c.solve(T.PROJ)
    assert list(st.corners) == want["corners"] and (st.n_added, st.n_valid, st.n_core) == (6, want["n_valid"], want["n_core"])
    assert _same_array(got, want["time_map"])


# ---- the tool on a recording, the processor on its file -----------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("calibrate_time_map", os.path.join(ROOT, "tools", "calibrate_time_map.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


CAM, PROJ_L = (80, 60), (135, 240)  # rig L of tests/rig_maps_cases.py
QUAD_L = ((9, 7), (66, 11), (71, 53), (6, 45))
CHUNK_WORDS = 1 << 12  # (the trigger finder cuts at most one frame per packet)


def _scaled(Kmat):
    Kmat = np.array(Kmat, np.float64)
    Kmat[:2] *= 0.125
    return Kmat


def test_the_tool_on_a_white_frame_recording_and_the_processor_on_its_file(tmp_path, golden_dir):
    from test_gpu_on_arrival import _write_live_yaml
    from x_maps_amd import evt3
    from x_maps_amd import synthetic as S
    from x_maps_amd.depth_reprojection_processor import DepthReprojectionProcessor, RuntimeParams
    g = dict(np.load(os.path.join(golden_dir, "g6_esl_calib.npz")))
    yaml_path = tmp_path / "calib_l.yaml"
    _write_live_yaml(yaml_path, dict(g, camera_K=_scaled(g["camera_K"]), projector_K=_scaled(g["projector_K"])), g["camera_D"].ravel())
    cp = cal.CamProjCalibrationParams.from_yaml(str(yaml_path), *CAM, *PROJ_L)
    assert (cp.rect_image_width, cp.rect_image_height) == (220, 165)
    # a white frame on a plane, 7 projector frames at 60 Hz: a 13 ms sweep along the projector's diagonal, then the dark gap
    surf = T.render(CAM, PROJ_L, QUAD_L, T.diagonal_time(PROJ_L), 7, span=13_000.0, drop=0.1, seed=4)
    frames = [T.events_from_surface(s, 2_000_000 + 16_600 * k) for k, s in enumerate(surf)]
    lead = np.zeros(2, S.EVENT_CD_DTYPE)  # (the trigger finder's first pause: see tests/test_gpu_on_arrival.py)
    lead["t"] = frames[0]["t"][0] - np.array([1600, 1500])
    lead["x"], lead["y"], lead["p"] = [30, 31], [30, 30], 1
    stream = np.concatenate([lead] + frames)
    raw = tmp_path / "white.raw"
    evt3.write_raw(str(raw), stream, width=CAM[0], height=CAM[1])
    # the frames the CPU chain cuts out of the very chunks the tool pushes
    dec, act, tf = evt3.Evt3Decoder(), IO.ActivityFilterC(CAM[0], CAM[1], int(1e6 / 60)), IO.TriggerFinderOracle(60)
    for words in evt3.read_raw_words(str(raw), chunk_words=CHUNK_WORDS):
        tf.process_events(act.process(IO.polarity_filter(dec.decode(words))))
    cut = tf.frames
    assert len(cut) >= 4 and all(len(f) > 1000 for f in cut)
    o = T.Oracle(CAM)
    o.add([K.oracle(f, CAM[0], CAM[1], "first", np.float64)[0] for f in cut])
    want = T.solve(o, T.min_count_for(0.5, o.n_used), PROJ_L)

    out = tmp_path / "out"
    rep = _tool().main([str(raw), "--calib", str(yaml_path), "--out", str(out), "--camera", "80x60", "--projector", "135x240",
                        "--chunk-words", str(CHUNK_WORDS)])
    assert rep["surfaces_added"] == len(cut) and rep["surfaces_skipped"] == 0 and rep["corners_detected"] == [list(c) for c in want["corners"]]
    assert (rep["n_valid"], rep["n_core"], rep["n_missing"], rep["n_unfilled"]) == (want["n_valid"], want["n_core"], want["n_missing"], want["n_unfilled"])
    proj_map, rect_map = np.load(out / "time_map_proj.npy"), np.load(out / "time_map_rect.npy")
    assert _same_array(proj_map, want["time_map"])
    tables = cal.build_tables(cp, projector_time_map=want["time_map"])
    assert _same_array(rect_map, tables["time_map_rect"])

    # the live pipe on the file the tool wrote == the pipe on tables built from the oracle's map
    def run(**kw):
        shown = []

        class Window:
            def should_close(self):
                return False

            def show_async(self, img):
                shown.append(np.array(img))

        params = RuntimeParams(camera_width=CAM[0], camera_height=CAM[1], projector_width=PROJ_L[0], projector_height=PROJ_L[1],
                               projector_fps=60, z_near=0.1, z_far=1.2, no_frame_dropping=True, camera_perspective=False, **kw)
        with DepthReprojectionProcessor(params, window=Window()) as proc:
            for words in evt3.read_raw_words(str(raw), chunk_words=CHUNK_WORDS):
                proc.process_evt3_words(words)
            proc.flush()
        return shown

    a = run(calib=str(yaml_path), projector_time_map=str(out / "time_map_rect.npy"))
    b = run(calib=None, projector_time_map=None, tables=tables)
    linear = run(calib=None, projector_time_map=None, tables=cal.build_tables(cp))
    assert len(a) == len(b) == len(cut) == len(linear)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, linear))  # (the calibrated map is not the linear one)
