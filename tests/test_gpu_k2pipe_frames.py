"""-m gpu: the group frame kernels on ARBITRARY disparity frames, through xm_debug_k2_group_u16 (it places caller-supplied frames
into the slots' layout and calls launch_k2_batch<2>).  The pipelined K2 (x_maps_amd/csrc/xmaps_k2pipe.hpp) otherwise only sees
what K1 made of synthetic event streams: smooth frames, disparities around 30, the last rectified row never written, border
cells rarely.  Here, against the 49-tap definition and the oracle's A5 - A7 (tests/k2_frame_cases.py: expected()), bit for bit:

* borders: targets 0 - 3 px from every edge and outside on all four sides, one-tile projectors, patches that stick out of the
  frame above and below -- octets outside the frame read as zeros;
* the value range: the LDS copy of the per-disparity table against the global one (best < n_lds, min(best, 65535)) at
  n_lds - 1, n_lds, n_lds + 1, the u16 range's ends, the depth clamp's and the white pixel's edges;
* the whole table of k_build_dlut: frames that between them sample every disparity 0 .. 65535;
* the live-quad mask from the reference's side: frames filled at exactly the cells the oracle writes, with and without the mask;
* the sheared frame addressing of the owner-tile rigs; frames that are not run; the one-block-per-tile kernel on the same frames;
  the handle afterwards.

Every rig runs with XM_K2_PIPE=2 at two / four pixels per thread, strided / consecutive, and with XM_K2_PIPE_BLOCKS unset, 1
and 5 (tests/test_gpu_k2pipe_walk.py: several items per block); xm_debug_k2_pipe_frames tells that the pipelined kernel ran."""
import functools

import numpy as np
import pytest

from conftest import xm_option

import k2_frame_cases as K
import xmaps_oracle as O
from x_maps_amd import XMapsEngine
from x_maps_amd import synthetic as S
from test_gpu_k2pipe import _rig as _pipe_rig

pytestmark = pytest.mark.gpu

VARIANTS = [("2", "0"), ("2", "1"), ("4", "0"), ("4", "1")]
BLOCKS = [None, "1", "5"]
CASE_IDS = ["x".join(str(v) for v in c[:4]) for c in K.BORDER_CASES]


def _options(ppt, consec, blocks, pipe="2", **more):
    xm_option("XM_K2_PIPE", pipe)
    xm_option("XM_K2_PIPE_PPT", ppt)
    xm_option("XM_K2_CONSEC", consec)
    xm_option("XM_K2_PIPE_BLOCKS", blocks)
    for k, v in more.items():
        xm_option(k, v)


def _group(eng, frames, valid=None, fill=None):
    """frames u16 [n][rect_h][rect_w] -> (depth [n][H][W], bgr [n][H][W][3]); fill = (depth value, BGR byte) the outputs hold before"""
    n, H, W = len(frames), eng.out_h, eng.out_w
    d0 = np.full((n, H, W), 0.0 if fill is None else fill[0], np.float32)
    b0 = np.full((n, H, W, 3), 0 if fill is None else fill[1], np.uint8)
    depth, bgr = eng.to_device(d0), eng.to_device(b0)
    try:
        eng.debug_k2_group_u16(frames, valid, depth, bgr)
        eng.dev_download(d0, depth)
        eng.dev_download(b0, bgr)
    finally:
        eng.dev_free(depth)
        eng.dev_free(bgr)
    return d0, b0


def _expected(tb, frames):
    return [K.expected(tb, f) for f in frames]


def _check(tb, frames, want, mode="none", pipe_frames=None, **engine_kw):
    with XMapsEngine(tb, n_slots=1, **engine_kw) as eng:
        assert eng.cols_info()["mode"] == mode  # ('none': no column tiles, so the live mask is all ones)
        d, b = _group(eng, frames)
        assert eng.debug_k2_pipe_frames() == (len(frames) if pipe_frames is None else pipe_frames)
    for f, (wd, wb) in enumerate(want):
        assert np.array_equal(d[f], wd), ("depth", f)
        assert np.array_equal(b[f], wb), ("bgr", f)
    return d, b


# ---- borders ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _border(i):
    tb, frames = K.border_group(K.BORDER_CASES[i])
    return tb, frames, _expected(tb, frames)


@pytest.mark.parametrize("ppt,consec", VARIANTS)
@pytest.mark.parametrize("i", range(len(K.BORDER_CASES)), ids=CASE_IDS)
def test_border_frames(i, ppt, consec):
    tb, frames, want = _border(i)
    for blocks in BLOCKS:
        _options(ppt, consec, blocks)
        _check(tb, frames, want)


# ---- the value range ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _values(i, nlds_max):
    tb, frames = K.value_group(K.BORDER_CASES[i], nlds_max)
    return tb, frames, _expected(tb, frames)


@pytest.mark.parametrize("ppt,consec", VARIANTS)
@pytest.mark.parametrize("nlds", [None, "1", "24"])
@pytest.mark.parametrize("i", range(len(K.BORDER_CASES)), ids=CASE_IDS)
def test_the_value_range_around_the_lds_copy_of_the_table(i, nlds, ppt, consec):
    tb, frames, want = _values(i, int(nlds or 2048))
    assert K.n_lds_of(tb, int(nlds or 2048)) == {None: 300, "1": 1, "24": 24}[nlds]
    for blocks in BLOCKS:
        _options(ppt, consec, blocks, XM_K2_NLDS_MAX=nlds)
        _check(tb, frames, want)


# ---- the whole table --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table():
    tb, frames = K.table_tables(), K.table_frames()
    return tb, frames, _expected(tb, frames)


@pytest.mark.parametrize("ppt,consec", VARIANTS)
@pytest.mark.parametrize("nlds", [None, "1"])
def test_every_entry_of_the_per_disparity_table(nlds, ppt, consec):
    """all 65 536 entries of k_build_dlut against the oracle (tests/test_k2_frame_cases_cpu.py: the frames sample every disparity):
    the first 2048 through the LDS copy, the rest -- with XM_K2_NLDS_MAX=1 all but the first -- through the global table"""
    tb, frames, want = _table()
    assert K.n_lds_of(tb, int(nlds or 2048)) == int(nlds or 2048)
    for blocks in BLOCKS:
        _options(ppt, consec, blocks, XM_K2_NLDS_MAX=nlds)
        _check(tb, frames, want)


# ---- the live mask, from the reference's side ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _writable(kind, proj_w):
    cfg, tb = K.column_rig(kind, proj_w)
    cells = K.writable_cells(tb, cfg)
    rng = np.random.default_rng(proj_w + len(kind))
    frames = np.stack([np.where(cells, rng.integers(1, 65536, cells.shape), 0) for _ in range(3)]).astype(np.uint16)
    return cfg, tb, frames, _expected(tb, frames)


@pytest.mark.parametrize("ppt,consec", VARIANTS)
@pytest.mark.parametrize("kind,proj_w", [("cols", 256), ("cols", 250), ("steep", 256), ("tall", 256)])
def test_a_value_in_every_cell_the_oracle_can_write_survives_the_live_mask(kind, proj_w, ppt, consec):
    """a mask that is too tight at a patch border loses a cell here, whatever K1 and the camera LUT do"""
    cfg, tb, frames, want = _writable(kind, proj_w)
    for blocks in BLOCKS:
        got = {}
        for live in ("1", "0"):
            _options(ppt, consec, blocks, XM_K2_LIVE=live)
            got[live] = _check(tb, frames, want, mode="cols")
        assert np.array_equal(got["1"][0], got["0"][0]) and np.array_equal(got["1"][1], got["0"][1])


# ---- sheared frames -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sheared(proj_w):
    cfg, tb = _pipe_rig("own", proj_w)
    rng = np.random.default_rng(proj_w)
    frames = np.concatenate((K.value_frames(rng, cfg.rect_w, cfg.rect_h, K.n_lds_of(tb))[:2],  # (the two with special values along the border)
                             K.sparse_frame(rng, cfg.rect_w, cfg.rect_h, 0.2)[None].astype(np.uint16),
                             rng.integers(1, 65536, (1, cfg.rect_h, cfg.rect_w)).astype(np.uint16)))  # a value in every cell
    for f in frames:  # row 0, the last row and both edge columns carry values
        assert f[0].any() and f[-1].any() and f[:, 0].any() and f[:, -1].any()
    return tb, frames, _expected(tb, frames)


@pytest.mark.parametrize("ppt,consec", VARIANTS)
@pytest.mark.parametrize("proj_w", [270, 320])
def test_sheared_frames_of_the_owner_tile_rigs(proj_w, ppt, consec):
    """the entry applies the shear (frame16_col), the kernel addresses rect_w + shear_extra columns; all ones in the mask by rule"""
    tb, frames, want = _sheared(proj_w)
    for blocks in BLOCKS:
        _options(ppt, consec, blocks)
        with XMapsEngine(tb, n_slots=1) as eng:
            info = eng.cols_info()
            assert info["mode"] == "own" and info["shear_m"] != 0 and info["shear_extra"] > 0, info
        _check(tb, frames, want, mode="own")


# ---- frames that are not run --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["1", "3", "T+1"])
@pytest.mark.parametrize("valid", ["10110010", "01111111", "11111110", "00000000"])
@pytest.mark.parametrize("ppt,consec", [("2", "0"), ("4", "1")])
def test_frames_that_are_not_run_keep_what_their_outputs_held(ppt, consec, valid, walk):
    cfg, tb, frames, want = _writable("cols", 256)
    T = -(-cfg.proj_w // (16 * int(ppt))) * -(-cfg.proj_h // 16)
    _options(ppt, consec, str(T + 1) if walk == "T+1" else walk)
    group = np.stack([frames[f % 3] for f in range(8)])
    flags = np.array([int(c) for c in valid], np.uint8)
    with XMapsEngine(tb, n_slots=1) as eng:
        d, b = _group(eng, group, flags, fill=(7.0, 0x5A))
        assert eng.debug_k2_pipe_frames() == 8
    for f in range(8):
        if flags[f]:
            assert np.array_equal(d[f], want[f % 3][0]) and np.array_equal(b[f], want[f % 3][1]), f
        else:
            assert (d[f] == np.float32(7.0)).all() and (b[f] == 0x5A).all(), f


# ---- the other kernel on the same frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k2_ppt", ["1", "2"])
@pytest.mark.parametrize("i", range(len(K.BORDER_CASES)), ids=CASE_IDS)
def test_the_one_block_per_tile_kernel_on_the_same_frames(i, k2_ppt):
    """XM_K2_PIPE=0: k_frame_proj_tiled_batch<2, 0, .> takes the group, one / two pixels per thread; the counter stays 0"""
    for tb, frames, want in (_border(i), _values(i, 2048)):
        _options(None, None, None, pipe="0", XM_K2_PPT=k2_ppt)
        _check(tb, frames, want, pipe_frames=0)


@pytest.mark.parametrize("pipe", ["0", "2"])
@pytest.mark.parametrize("k2_ppt", ["1", "2"])
@pytest.mark.parametrize("case", [(151, 101, 50, 37, 0.3), (40, 23, 19, 17, 0.5)], ids=["151x101x50x37", "40x23x19x17"])
def test_frame_heights_the_pipelined_loader_does_not_take(case, k2_ppt, pipe):
    """rect_h % 8 != 0: the rig keeps the one-block-per-tile kernel even when XM_K2_PIPE=2 asks for the other one"""
    tb, frames = K.border_group(case)
    _options(None, None, None, pipe=pipe, XM_K2_PPT=k2_ppt)
    _check(tb, frames, _expected(tb, frames), pipe_frames=0)


# ---- the entry's checks, and the handle afterwards ------------------------------------------------------------------------------
def test_the_entry_validates_its_arguments():
    tb, frames, _ = _border(4)
    with XMapsEngine(tb, n_slots=1) as eng:
        for bad in (frames[:0], np.concatenate([frames] * 17)[:65]):
            with pytest.raises(Exception):
                _group(eng, bad)
        d, _ = _group(eng, np.concatenate([frames] * 16))  # 64 frames: the most it takes
        assert np.array_equal(d[63], d[3]) and np.array_equal(d[60], d[0])
    with XMapsEngine(S.make_tables(S.C_TINY), camera_perspective=True, n_slots=1) as eng:
        with pytest.raises(Exception):
            eng.debug_k2_group_u16(np.zeros((1, eng.rect_h, eng.rect_w), np.uint16), None, None, None)


def test_the_handle_works_as_before_after_debug_calls():
    """the entry touches no slot's state, tag or frame: a group of event frames afterwards equals the oracle, the path counters,
    the fallback counter and the last frame's statistics are a fresh handle's"""
    xm_option("XM_K2_PIPE", "2")
    cfg, tb, frames, want = _writable("cols", 256)
    evs = [S.make_events(cfg, frame=70 + f, n=cfg.n_events + 3_000 * f) for f in range(3)]
    refs = []
    for e in evs:
        x, y, t, _ = S.to_soa(e)
        refs.append(O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t))

    def events(eng, reps):
        for _ in range(reps):
            out = eng.process_event_frames(evs)
            for f, (d, b) in enumerate(out):
                assert np.array_equal(d, refs[f]["depth"]) and np.array_equal(b, refs[f]["bgr"]), f
        return eng.path_counts(), eng.sorted_fallbacks(), eng.last_frame_stats()

    with XMapsEngine(tb, n_slots=3) as eng:
        fresh = events(eng, 2)
        assert eng.debug_k2_pipe_frames() == 6
    with XMapsEngine(tb, n_slots=3) as eng:
        events(eng, 1)
        for k in range(3):
            d, b = _group(eng, frames[k:], np.array([1, 0, 1] if k == 0 else [1] * (3 - k), np.uint8))  # (3, 2, 1 frames; one not run)
            assert np.array_equal(d[0], want[k][0]) and np.array_equal(b[0], want[k][1])
        used = events(eng, 1)
        assert eng.debug_k2_pipe_frames() == 6 + 3 + 2 + 1
    assert used == fresh and fresh[0]["cols"] == 6 and fresh[1] == 0
    st = used[2]
    assert (st.n_events, st.n_inliers, st.t_min, st.t_max) == (len(evs[2]), int(refs[2]["mask"].sum()), float(evs[2]["t"].min()), float(evs[2]["t"].max()))
