"""-m gpu: the persistent WALK of the pipelined K2 (x_maps_amd/csrc/xmaps_k2pipe.hpp).  A block strides through (frame, tile)
items with item i + 1's patch quads and pixel offsets in registers while it reduces and samples item i; it crosses frame
boundaries in advance(), skips frames that are not valid or were redone, and leaves on m1.f >= n_frames.  The launcher sizes the
grid to the chip (>= 1024 blocks on 256 CUs) and cuts it to the item count, so on the suite's rigs (<= 800 items) every block
gets ONE item: the prologue, one iteration, break.  XM_K2_PIPE_BLOCKS=N caps the grid (host/xm_launch.hpp): with N blocks for
320 items the loop-bottom issue(), m0 = m1, p0 = p1, a second to_lds over a patch just sampled and items of different frames in
one block all run.  The rigs, groups (5 frames, one a shorter scan, processed twice through one engine) and variants are those
of tests/test_gpu_k2pipe.py; every case is compared with the CPU oracle bit for bit.

Walks, with T = tiles per frame at the requested pixels per thread: 1 (one block walks every item of the group across every
frame boundary), 3, 8, 13 (coprime to T: a block's tile changes with every item), T - 1, T, T + 1 (every block's next item is a
neighbouring tile of the next frame, and blocks >= T start in frame 1), 2T + 5."""
import functools

import numpy as np
import pytest

from conftest import xm_option

import xmaps_oracle as O
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from test_gpu_k2pipe import _rig

pytestmark = pytest.mark.gpu

N_FRAMES = 5
WALKS = ["1", "3", "8", "13", "T-1", "T", "T+1", "2T+5"]
REDUCED = ["1", "13", "T+1"]


def _blocks(walk, cfg, ppt):
    T = -(-cfg.proj_w // (16 * int(ppt))) * -(-cfg.proj_h // 16)
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+5": 2 * T + 5}.get(walk) or int(walk)


def _ref(tb, evs):
    x, y, t, _ = S.to_soa(evs)
    r = O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t)
    return r["depth"], r["bgr"]


@functools.lru_cache(maxsize=None)
def _case(kind, proj_w):
    """(cfg, tables, frames, references): computed once per rig, shared by every case that uses it, never modified"""
    cfg, tb = _rig(kind, proj_w)
    frames = [S.make_events(cfg, frame=70 + f, n=cfg.n_events + 3_000 * f) for f in range(N_FRAMES)]
    frames[1] = frames[1][: len(frames[1]) // 2].copy()  # a shorter scan: stale cells must not show
    return cfg, tb, frames, [_ref(tb, e) for e in frames]


def _walk(kind, proj_w, ppt, consec, walk, n_frames=N_FRAMES, **kw):
    cfg, tb, frames, refs = _case(kind, proj_w)
    xm_option("XM_K2_PIPE", "2")
    if ppt is not None:
        xm_option("XM_K2_PIPE_PPT", ppt)
    xm_option("XM_K2_CONSEC", consec)
    xm_option("XM_K2_PIPE_BLOCKS", str(_blocks(walk, cfg, ppt or "2")))
    with XMapsEngine(tb, n_slots=n_frames) as eng:
        for rep in range(2):  # twice: the second group finds the first one's frames in its slots
            out = eng.process_event_frames(frames[:n_frames], **kw)
            for f, (d, b) in enumerate(out):
                if kw.get("want_depth", True):
                    assert np.array_equal(d, refs[f][0]), (rep, f)
                if kw.get("want_bgr", True):
                    assert np.array_equal(b, refs[f][1]), (rep, f)
        assert eng.path_counts()["cols"] == 2 * n_frames and eng.sorted_fallbacks() == 0, (eng.path_counts(), eng.cols_info())
        assert eng.debug_k2_pipe_frames() == 2 * n_frames


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("consec", ["0", "1"])
@pytest.mark.parametrize("ppt", ["2", "4"])
@pytest.mark.parametrize("kind,proj_w", [("cols", 256), ("cols", 250), ("own", 270), ("fine", 604)])
def test_every_walk_in_every_variant(kind, proj_w, ppt, consec, walk):
    _walk(kind, proj_w, ppt, consec, walk)


@pytest.mark.parametrize("walk", REDUCED)
@pytest.mark.parametrize("consec", ["0", "1"])
@pytest.mark.parametrize("ppt", ["2", "4"])
@pytest.mark.parametrize("kind,proj_w", [("cols", 264), ("cols", 260), ("own", 320), ("fine", 640), ("fine", 600), ("fine", 570), ("tall", 256)])
def test_the_other_widths_on_three_walks(kind, proj_w, ppt, consec, walk):
    _walk(kind, proj_w, ppt, consec, walk)


@pytest.mark.parametrize("consec", ["0", "1"])
@pytest.mark.parametrize("nlds", ["1", "24"])
def test_disparities_beyond_the_lds_copy_of_the_table_on_a_walk(nlds, consec):
    xm_option("XM_K2_NLDS_MAX", nlds)  # the shared-cell rig's disparities are around 30
    _walk("own", 272, None, consec, "3", n_frames=3)


@pytest.mark.parametrize("consec", ["0", "1"])
def test_depth_only_and_bgr_only_on_a_walk(consec):
    _walk("cols", 256, None, consec, "3", n_frames=3, want_bgr=False)
    _walk("cols", 256, None, consec, "3", n_frames=3, want_depth=False)


def _soa_on_device(eng, frames):
    x, y, t, _ = S.to_soa(np.concatenate(frames))
    return eng.to_device(x), eng.to_device(y), eng.to_device(t)


@pytest.mark.parametrize("consec", ["0", "1"])
@pytest.mark.parametrize("shift", [1, 4, 8])
def test_output_rows_at_any_address_on_a_walk(shift, consec):
    """the BGR rows leave as 16 / 8 / 4-byte or single-byte stores, whichever the frame's address and row length allow"""
    cfg, tb, frames, refs = _case("cols", 256)
    xm_option("XM_K2_PIPE", "2")
    xm_option("XM_K2_CONSEC", consec)
    xm_option("XM_K2_PIPE_PPT", "4")
    xm_option("XM_K2_PIPE_BLOCKS", "3")
    F, px = 3, cfg.proj_w * cfg.proj_h
    offs = np.concatenate(([0], np.cumsum([len(f) for f in frames[:F]]))).astype(np.uint64)
    with XMapsEngine(tb, n_slots=F) as eng:
        X, Y, T = _soa_on_device(eng, frames[:F])
        depth, bgr = eng.to_device(np.zeros(F * px, np.float32)), eng.to_device(np.zeros(F * px * 3 + 64, np.uint8))
        try:
            eng.process_batch_device(X, Y, T, None, offs, depth, bgr + shift)
            eng.sync()
            assert eng.debug_k2_pipe_frames() == F and eng.path_counts()["cols"] == F and eng.sorted_fallbacks() == 0
            got_d, raw = np.empty((F, cfg.proj_h, cfg.proj_w), np.float32), np.empty(F * px * 3 + 64, np.uint8)
            eng.dev_download(got_d, depth)
            eng.dev_download(raw, bgr)
        finally:
            for p in (X, Y, T, depth, bgr):
                eng.dev_free(p)
    assert not raw[:shift].any() and not raw[shift + F * px * 3:].any()  # nothing before the first row or behind the last
    got_b = raw[shift: shift + F * px * 3].reshape(F, cfg.proj_h, cfg.proj_w, 3)
    for f in range(F):
        assert np.array_equal(got_d[f], refs[f][0]) and np.array_equal(got_b[f], refs[f][1]), f


@pytest.mark.parametrize("walk", ["1", "13"])
@pytest.mark.parametrize("live", ["1", "0"])
@pytest.mark.parametrize("kind,proj_w", [("cols", 256), ("cols", 250), ("tall", 256)])
def test_the_live_mask_and_all_ones_on_a_walk(kind, proj_w, live, walk):
    xm_option("XM_K2_LIVE", live)
    _walk(kind, proj_w, None, "1", walk)


@pytest.mark.parametrize("walk", [1, 5])
def test_a_captured_batch_skips_its_redone_frame_in_the_middle_of_a_walk(walk):
    """COND = 2: the frame whose tiles objected is skipped between two run frames of one block; it comes from the 64-bit path"""
    xm_option("XM_K2_PIPE", "2")
    xm_option("XM_K2_PIPE_BLOCKS", str(walk))
    cfg, tb = _rig("cols", 260)
    n = 120_000  # (a captured group takes the tiles only where the frames are dense enough for the tiled K1 of its redo)
    evs = [S.make_events(cfg, frame=80 + f, n=n) for f in range(4)]
    a, b = evs[2][5_000:6_000].copy(), evs[2][80_000:81_000].copy()
    evs[2][5_000:6_000], evs[2][80_000:81_000] = b, a  # not sorted
    want = [_ref(tb, e) for e in evs]
    F, px = len(evs), cfg.proj_w * cfg.proj_h
    offs = np.arange(F + 1, dtype=np.uint64) * n
    with XMapsEngine(tb, n_slots=8, default_priority_streams=True) as eng:
        X, Y, T = _soa_on_device(eng, evs)
        depth, bgr = eng.dev_alloc(F * px * 4), eng.dev_alloc(F * px * 3)
        try:
            g = eng.graph_create(X, Y, T, None, offs, depth, bgr)
            assert eng.path_counts()["cols"] == F and eng.debug_k2_pipe_frames() == F, (eng.path_counts(), eng.debug_k2_pipe_frames())
            d, bb = np.empty((F, cfg.proj_h, cfg.proj_w), np.float32), np.empty((F, cfg.proj_h, cfg.proj_w, 3), np.uint8)
            for rep in range(3):
                eng.dev_upload(depth, np.full(F * px, 7.0, np.float32))
                eng.dev_upload(bgr, np.full(F * px * 3, 0x5A, np.uint8))
                g.launch()
                eng.sync()
                eng.dev_download(d, depth)
                eng.dev_download(bb, bgr)
                for f in range(F):
                    assert np.array_equal(d[f], want[f][0]) and np.array_equal(bb[f], want[f][1]), (rep, f)
            g.close()
        finally:
            for p in (X, Y, T, depth, bgr):
                eng.dev_free(p)


def test_a_group_with_an_empty_frame_in_the_middle():
    """n == 0 with valid != 0: a defined empty frame.  Such a group has no (t[0], t[n-1]) for every frame, so it does not take the
    column tiles: it goes down the general path (64-bit key frames, the one-block-per-tile K2), whatever the walk says."""
    cfg, tb, frames, refs = _case("cols", 256)
    xm_option("XM_K2_PIPE", "2")
    xm_option("XM_K2_PIPE_BLOCKS", "3")
    evs, F, px = [frames[0], frames[2], frames[3]], 4, cfg.proj_w * cfg.proj_h
    lens = [len(evs[0]), 0, len(evs[1]), len(evs[2])]
    want = [refs[0], None, refs[2], refs[3]]
    offs = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    with XMapsEngine(tb, n_slots=F) as eng:
        X, Y, T = _soa_on_device(eng, evs)
        depth, bgr = eng.to_device(np.full(F * px, 7.0, np.float32)), eng.to_device(np.full(F * px * 3, 0x5A, np.uint8))
        try:
            eng.process_batch_device(X, Y, T, None, offs, depth, bgr)
            eng.sync()
            pc = eng.path_counts()
            assert pc["general"] == F and pc["cols"] == 0 and eng.debug_k2_pipe_frames() == 0 and eng.sorted_fallbacks() == 0, pc
            d, b = np.empty((F, cfg.proj_h, cfg.proj_w), np.float32), np.empty((F, cfg.proj_h, cfg.proj_w, 3), np.uint8)
            eng.dev_download(d, depth)
            eng.dev_download(b, bgr)
        finally:
            for p in (X, Y, T, depth, bgr):
                eng.dev_free(p)
    for f, r in enumerate(want):
        if r is None:  # no event: an all-zero disparity frame
            assert not d[f].any() and (b[f] == 255).all()
        else:
            assert np.array_equal(d[f], r[0]) and np.array_equal(b[f], r[1]), f
