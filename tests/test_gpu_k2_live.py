"""-m gpu: the pipelined K2 (x_maps_amd/csrc/xmaps_k2pipe.hpp) does not load the 16-byte quads of the column tiles' disparity
frame that no (row, time column) pair can ever store into (host/xm_k2_live.hpp builds one bit per tile and loader slot in
xm_create).  Depth and BGR must be what the CPU oracle gives, bit for bit, and the same with XM_K2_LIVE=0 -- all ones in the
mask, the same kernel -- on the small rigs of test_gpu_k2pipe.py (camera 160 x 128, groups of 5 frames, processed twice so
that stale cells are met; XM_K2_PIPE=2 sends their groups to the pipelined kernel):

* the column rigs at the projector widths where the loader's slot arithmetic can go wrong, two / four pixels per thread,
  strided / consecutive;
* a steep X-map (one frame column per 3 rows, time columns 4 frame columns apart: octets with a single live cell at their
  first or last row); patches of 9 - 10 row octets (more than one loader register); owner-tile rigs (all ones by rule);
* a captured batch whose unsorted frame is redone beside masked frames; a short frame after a dense one in the same slot;
* eight frames that between them put an event on every camera pixel in every time column: every cell a camera pixel can reach
  holds a winner in one of them."""
import functools

import numpy as np
import pytest

from conftest import xm_option

import xmaps_oracle as O
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from k2_frame_cases import every_pixel_frames, steep_tables as _steep_tables

pytestmark = pytest.mark.gpu


def _ref(tb, evs):
    x, y, t, _ = S.to_soa(evs)
    r = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t)
    return r["depth"], r["bgr"]


@functools.lru_cache(maxsize=None)
def _rig(kind, proj_w):
    """(cfg, tables, frames, references): computed once per rig, shared by every case that uses it, never modified"""
    if kind == "own":  # several time columns per cell: owner tiles, sheared frame -> all ones
        cfg = S.RigConfig("k2l-own", 160, 128, proj_w, 120, 40_000)
        tb = S.make_tables_shared_cells(cfg, cols_per_cell=proj_w / 82.0)
    elif kind == "tall":  # patches of 9 - 10 row octets
        cfg = S.RigConfig("k2l-tall", 160, 128, proj_w, 96, 60_000)
        tb = S.make_tables(cfg)
    elif kind == "steep":
        cfg = S.RigConfig("k2l-steep", 160, 128, proj_w, 128, 60_000)
        tb = _steep_tables(cfg)
    else:
        cfg = S.RigConfig("k2l-cols", 160, 128, proj_w, 128, 60_000)
        tb = S.make_tables(cfg)
    frames = [S.make_events(cfg, frame=70 + f, n=cfg.n_events + 3_000 * f) for f in range(5)]
    frames[1] = frames[1][: len(frames[1]) // 2].copy()  # a shorter scan
    return cfg, tb, frames, [_ref(tb, e) for e in frames]


def _run(tb, groups, live, n_slots, want_mode="cols"):
    """every group twice through one engine; [(depth, bgr)] per group and repetition"""
    xm_option("XM_K2_LIVE", live)
    outs = []
    with XMapsEngine(tb, n_slots=n_slots) as eng:
        assert eng.cols_info()["mode"] == want_mode
        n = 0
        for frames in groups:
            for _ in range(2):
                outs.append(eng.process_event_frames(frames))
                n += len(frames)
        assert eng.path_counts()["cols"] == n and eng.sorted_fallbacks() == 0, (eng.path_counts(), eng.cols_info())
        assert eng.debug_k2_pipe_frames() == n
    return outs


def _check(tb, groups, refs, n_slots, want_mode="cols"):
    on = _run(tb, groups, "1", n_slots, want_mode)
    off = _run(tb, groups, "0", n_slots, want_mode)
    for k, (a, b) in enumerate(zip(on, off)):
        ref = refs[k // 2]
        for f, ((d1, b1), (d0, b0)) in enumerate(zip(a, b)):
            assert np.array_equal(d1, ref[f][0]) and np.array_equal(b1, ref[f][1]), ("live mask", k, f)
            assert np.array_equal(d0, ref[f][0]) and np.array_equal(b0, ref[f][1]), ("all ones", k, f)
            assert np.array_equal(d1, d0) and np.array_equal(b1, b0), (k, f)


@pytest.mark.parametrize("consec", ["0", "1"])
@pytest.mark.parametrize("ppt", ["2", "4"])
@pytest.mark.parametrize("kind,proj_w", [("cols", 256), ("cols", 264), ("cols", 260), ("cols", 250), ("steep", 256), ("tall", 256)])
def test_masked_loads_against_the_oracle_and_against_all_ones(kind, proj_w, ppt, consec):
    xm_option("XM_K2_PIPE", "2")
    xm_option("XM_K2_PIPE_PPT", ppt)
    xm_option("XM_K2_CONSEC", consec)
    cfg, tb, frames, refs = _rig(kind, proj_w)
    _check(tb, [frames], [refs], len(frames))


@pytest.mark.parametrize("proj_w", [270, 320])
def test_owner_tile_rigs_are_unchanged(proj_w):
    """another flush, a sheared frame: their mask is all ones whatever the switch says"""
    xm_option("XM_K2_PIPE", "2")
    cfg, tb, frames, refs = _rig("own", proj_w)
    _check(tb, [frames], [refs], len(frames), want_mode="own")


def test_a_short_frame_after_a_dense_one_in_the_same_slot():
    xm_option("XM_K2_PIPE", "2")
    cfg, tb, frames, refs = _rig("steep", 256)
    short = [frames[4][: len(frames[4]) // 6].copy(), frames[0][: len(frames[0]) // 3].copy(), frames[2]]
    short_refs = [_ref(tb, e) for e in short[:2]] + [refs[2]]
    _check(tb, [frames[:3], short], [refs[:3], short_refs], 3)


def test_a_captured_batch_redoes_its_unsorted_frame_beside_masked_frames():
    """COND = 2: the pipelined K2 of a captured group skips the frame whose tiles objected; that frame comes from the 64-bit path"""
    torch = pytest.importorskip("torch")
    xm_option("XM_K2_PIPE", "2")
    cfg, tb, frames, refs = _rig("cols", 260)
    n = 120_000  # (a captured group takes the tiles only where the frames are dense enough for the tiled K1 of its redo)
    evs = [S.make_events(cfg, frame=80 + f, n=n) for f in range(4)]
    a, b = evs[2][5_000:6_000].copy(), evs[2][80_000:81_000].copy()
    evs[2][5_000:6_000], evs[2][80_000:81_000] = b, a  # not sorted
    want = [_ref(tb, e) for e in evs]
    F = len(evs)
    dev = torch.device("cuda", 0)
    cat = np.concatenate(evs)
    x, y, t, _ = S.to_soa(cat)
    X = torch.from_numpy(x.view(np.int16)).to(dev)
    Y = torch.from_numpy(y.view(np.int16)).to(dev)
    T = torch.from_numpy(t).to(dev)
    offs = np.arange(F + 1, dtype=np.uint64) * n
    got = {}
    for live in ("1", "0"):
        xm_option("XM_K2_LIVE", live)
        depth = torch.zeros((F, cfg.proj_h, cfg.proj_w), dtype=torch.float32, device=dev)
        bgr = torch.zeros((F, cfg.proj_h, cfg.proj_w, 3), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with XMapsEngine(tb, n_slots=8, default_priority_streams=True) as eng:
            g = eng.graph_create(X.data_ptr(), Y.data_ptr(), T.data_ptr(), None, offs, depth.data_ptr(), bgr.data_ptr())
            assert eng.path_counts()["cols"] == F and eng.debug_k2_pipe_frames() == F, (eng.path_counts(), eng.debug_k2_pipe_frames())
            for rep in range(2):
                g.launch()
                eng.sync()
                d, bb = depth.cpu().numpy(), bgr.cpu().numpy()
                for f in range(F):
                    assert np.array_equal(d[f], want[f][0]) and np.array_equal(bb[f], want[f][1]), (live, rep, f)
                depth.zero_()
                bgr.zero_()
                torch.cuda.synchronize()
            g.launch()
            eng.sync()
            got[live] = (depth.cpu().numpy(), bgr.cpu().numpy())
            g.close()
    assert np.array_equal(got["1"][0], got["0"][0]) and np.array_equal(got["1"][1], got["0"][1])


def test_every_cell_a_camera_pixel_can_reach_holds_a_winner():
    """8 frames: frame k carries one event per time column for every camera pixel with x = k mod 8 (2 560 events per time
    column: under 65 527 per tile at any tile width).  A live cell the mask left out would lose its winner."""
    xm_option("XM_K2_PIPE", "2")
    cfg, tb, _, _ = _rig("cols", 256)
    n_cols = tb["proj_x_map"].shape[1]
    frames = every_pixel_frames(tb, cfg)
    assert n_cols * (cfg.cam_w // 8) * cfg.cam_h == len(frames[0]) and (cfg.cam_w // 8) * cfg.cam_h * 16 < 65_527
    refs = [_ref(tb, e) for e in frames]
    assert sum(int(np.count_nonzero(r[0])) for r in refs) > 0
    _check(tb, [frames], [refs], 8)


@pytest.mark.parametrize("kind,proj_w,derived", [("cols", 256, True), ("cols", 250, True), ("steep", 256, True), ("tall", 256, True),
                                                 ("own", 270, False)])
def test_the_column_rigs_run_on_a_derived_mask_not_on_all_ones(capfd, kind, proj_w, derived):
    """XM_K2_LIVE=2 reports what xm_create derived, one line per tile geometry: on the column rigs a share of the loader's slots
    strictly between 0 and 1 (the cases above would pass on all ones as well); on owner tiles nothing is derived"""
    import re
    xm_option("XM_K2_LIVE", "2")
    cfg, tb, _, _ = _rig(kind, proj_w)
    capfd.readouterr()
    with XMapsEngine(tb, n_slots=2) as eng:
        assert eng.cols_info()["mode"] == ("cols" if derived else "own")
    err = capfd.readouterr().err
    shares = [float(v) for v in re.findall(r"K2 live quads.*loader slots ([0-9.]+)", err)]
    if derived:
        assert len(shares) == 2 and all(0.05 < v < 0.95 for v in shares), err
    else:
        assert shares == [], err
