"""CPU: what the GPU tests of the pipelined K2 on arbitrary frames (tests/test_gpu_k2pipe_frames.py) rest on, pinned without a GPU
(tests/k2_frame_cases.py): the vectorised A4 reference equals the 49-tap loops on every border case those tests use; the frames
of the whole-table test sample every disparity 0 .. 65535; the chosen P03 / z_near / z_far put the clamp's and the u8's edges on
integer disparities that the value-range frames hold; the cells the oracle writes on the column rigs are a proper part of the frame;
the tile classifier of tests/test_gpu_k2_tiled_paths.py gives what was worked out by hand, and that test's shapes reach every loader."""
import numpy as np
import pytest

import k2_frame_cases as K
import xmaps_oracle as O


@pytest.mark.parametrize("case", K.BORDER_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_the_vectorised_reference_equals_the_49_taps_on_every_border_case(case):
    for tb, frames in (K.border_group(case), K.value_group(case)):
        pmap = tb["disp_proj_mapxy_i16"]
        inside = (pmap[..., 0] >= 0) & (pmap[..., 0] < tb["rect_w"]) & (pmap[..., 1] >= 0) & (pmap[..., 1] < tb["rect_h"])
        assert inside.any() and not inside.all()  # targets inside and outside the frame
        for rect in frames[:2] if tb["rect_w"] > 300 else frames:  # (the loops take 0.6 s per frame of the largest case)
            rect = rect.astype(np.float32)
            want = K.brute_dilate_remap(rect, pmap)
            assert np.array_equal(K.shifted_dilate_remap(rect, pmap), want)
            assert np.array_equal(O.remap_rectified_disp_map_to_proj(rect, pmap), want)  # the oracle too


def test_the_border_groups_hold_four_different_frames_with_values_on_every_edge():
    for case in K.BORDER_CASES:
        tb, frames = K.border_group(case)
        assert frames.shape == (4, case[1], case[0]) and frames.dtype == np.uint16 and case[1] % 8 == 0
        assert len({f.tobytes() for f in frames}) == 4
        for f in frames:
            assert f[0].all() and f[-1].all() and f[:, 0].all() and f[:, -1].all()


def test_the_table_frames_sample_every_disparity():
    """the first two (monotone) frames leave out exactly the disparities with a byte below 3 -- a larger neighbour sits in every
    window that holds their cell; the third frame carries those"""
    tb, frames = K.table_tables(), K.table_frames()
    assert frames.shape == (3, 256, 256) and np.array_equal(frames[1], 65535 - frames[0])
    assert np.array_equal(frames[0][7, 5], 5 * 256 + 7)  # v[col][row] = col * 256 + row
    seen = np.zeros(65536, bool)
    for k, rect in enumerate(frames):
        seen[K.shifted_dilate_remap(rect.astype(np.float32), tb["disp_proj_mapxy_i16"]).astype(np.int64).reshape(-1)] = True
        if k == 1:
            d = np.arange(65536)
            assert np.array_equal(~seen, ((d >> 8) < 3) | ((d & 255) < 3))
    assert seen.all()


def test_the_clamp_edges_fall_on_integer_disparities_the_value_frames_hold():
    d = np.arange(0, 1400).astype(np.float32)
    depth = O.disparity_to_depth_rectified(d, K.P03)
    assert depth[100] == np.float32(K.Z_FAR) and depth[1200] == np.float32(K.Z_NEAR) and depth[99] > depth[100] > depth[101]
    assert depth[1199] > depth[1200] > depth[1201]
    u8 = O.clip_normalize_uint8_depth_frame(depth, K.Z_NEAR, K.Z_FAR)
    # 255 up to the clamp, then 252: 253 and 254 lie between two integer disparities (k2_frame_cases.py); 1 down to d = 1150, then 0
    assert list(u8[[99, 100, 101]]) == [255, 255, 252] and list(u8[[1104, 1105, 1150, 1151, 1199, 1200, 1201]]) == [2, 1, 1, 0, 0, 0, 0]
    assert not np.isin(u8, (253, 254)).any()
    for case in K.BORDER_CASES:
        for nlds_max in (2048, 1, 24):
            tb, frames = K.value_group(case, nlds_max)
            n_lds = K.n_lds_of(tb, nlds_max)
            assert n_lds == min(300, nlds_max)
            disp = np.stack([K.shifted_dilate_remap(f.astype(np.float32), tb["disp_proj_mapxy_i16"]) for f in frames])
            want = set(int(v) for v in K.special_values(n_lds))
            if case[2] * case[3] >= 256:  # (the 4 x 5 and 16 x 9 projectors have fewer pixels than there are values)
                assert want <= set(int(v) for v in np.unique(disp)), (case, nlds_max, want - set(int(v) for v in np.unique(disp)))
            got = np.unique(np.concatenate([K.expected(tb, f)[1].reshape(-1, 3) for f in frames]), axis=0)
            u8s = np.unique(O.clip_normalize_uint8_depth_frame(O.disparity_to_depth_rectified(disp, tb["p03"]), tb["z_near"], tb["z_far"]))
            if case[2] * case[3] >= 256:
                assert {0, 1, 252, 255} <= set(int(v) for v in u8s), (case, u8s)
            assert len(got) > 1


def _map_tables(mx, my, rect_w, rect_h):
    return {"disp_proj_mapxy_i16": np.stack((mx, my), -1).astype(np.int16), "rect_w": rect_w, "rect_h": rect_h}


def test_the_tile_classifier_on_maps_worked_out_by_hand():
    """a 48 x 32 projector shifted by (8, 8) into a 64 x 48 frame: a 16-pixel tile's targets span 16 cells, + 3 of margin either
    side = 22 columns; rows 8 .. 23 - 3 start at 5 -> 0, end at 26 -> 32 rows"""
    vs, us = np.mgrid[0:32, 0:48]
    tb = _map_tables(us + 8, vs + 8, 64, 48)
    t1 = K.classify_tiles(tb, 1)
    assert len(t1) == 3 * 2
    assert t1[0] == {"kind": "interior", "cols": 22, "rows_p": 32, "loads64": 2, "loads16": 1}  # 352 pairs, 88 octets on 256 threads
    assert t1[3] == t1[0]  # rows 24 .. 39: 21 -> 16 .. 42 -> 48, the frame's last row
    t2 = K.classify_tiles(tb, 2)
    assert len(t2) == 2 * 2
    assert t2[0] == {"kind": "interior", "cols": 38, "rows_p": 32, "loads64": 3, "loads16": 1}  # 608 pairs
    assert t2[1]["cols"] == 22  # the projector's last 16 columns alone
    assert K.tiled_loader_paths(tb, 1) == {"u16_oct_le8", "key64_un2"} and K.tiled_loader_paths(tb, 2) == {"u16_oct_le8", "key64_un2", "key64_un3"}
    # one frame row less: the lower tiles' patches stick out; the upper ones no longer take the 16-byte u16 loads (47 % 4 != 0)
    low = K.classify_tiles(_map_tables(us + 8, vs + 8, 64, 47), 1)
    assert [t["kind"] for t in low] == ["interior"] * 3 + ["border"] * 3
    assert K.tiled_loader_paths(_map_tables(us + 8, vs + 8, 64, 47), 1) == {"border"}
    assert K.tiled_loader_paths(_map_tables(us + 8, vs + 8, 64, 52), 1) == {"u16_quad", "key64_un2"}
    # targets 8 cells apart: 15 * 8 + 7 = 127 columns; rows 128 .. 248 -> 120 .. 251 = 132 -> 136 rows: > 10240 cells, also where
    # the patch sticks out of the frame (the first tile).  A tile whose targets all lie outside is empty
    mx, my = us * 8, vs * 8
    mx[:16, 16:32] = -1
    wild = K.classify_tiles(_map_tables(mx, my, 512, 512), 1)
    assert [t["kind"] for t in wild] == ["too_large", "empty"] + ["too_large"] * 4
    assert wild[5] == {"kind": "too_large", "cols": 127, "rows_p": 136, "loads64": 34, "loads16": 9}
    assert wild[1] == {"kind": "empty", "cols": 0, "rows_p": 0, "loads64": 0, "loads16": 0}


@pytest.mark.parametrize("ppt", [1, 2])
def test_every_window_lies_inside_its_tiles_patch_and_the_path_cases_reach_every_loader(ppt):
    """what the classifier claims of tests/test_gpu_k2_tiled_paths.py's shapes, and that its patches hold what k_build_k2_tables'
    do: the 7 x 7 window of every target inside the frame, rows from a multiple of 8 in whole octets"""
    reached = set()
    for case in K.TILED_PATH_CASES:
        tb, _ = K.border_tables(*case, seed=case[0])
        tiles = K.classify_tiles(tb, ppt)
        assert len(tiles) == -(-case[2] // (16 * ppt)) * -(-case[3] // 16)
        for t in tiles:
            assert t["rows_p"] % 8 == 0 and (t["kind"] == "too_large") == (t["cols"] * t["rows_p"] > K.K2_TILE_MAX)
            if t["kind"] == "interior":
                assert t["cols"] >= 7 and t["rows_p"] >= 8 and t["cols"] <= case[0] and t["rows_p"] <= case[1]
                assert (t["loads64"] - 1) * 256 < t["cols"] * t["rows_p"] // 2 <= t["loads64"] * 256
                assert (t["loads16"] - 1) * 256 < t["cols"] * t["rows_p"] // 8 <= t["loads16"] * 256
        reached |= K.tiled_loader_paths(tb, ppt)
    assert K.TILED_PATHS_WANTED[ppt] <= reached, K.TILED_PATHS_WANTED[ppt] - reached


@pytest.mark.parametrize("kind,proj_w", [("cols", 256), ("cols", 250), ("steep", 256), ("tall", 256)])
def test_the_oracle_writes_a_proper_part_of_the_column_rigs_frames(kind, proj_w):
    cfg, tb = K.column_rig(kind, proj_w)
    cells = K.writable_cells(tb, cfg)
    assert cells.shape == (tb["rect_h"], tb["rect_w"])
    assert 0.05 < cells.mean() < 0.95, cells.mean()
    assert not cells[-1].any()  # the last rectified row is never written (xmd:23): the frames of the GPU test leave it empty too
