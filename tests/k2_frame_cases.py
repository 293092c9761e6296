"""Shared by the K2 tests: the 49-tap DEFINITION of A4 (cv2.dilate 7x7 o cv2.remap nearest, python/disp_to_depth.py:76-97;
semantics restated in tests/test_gpu_a4_bruteforce.py), border-heavy tables and frames, and what the tests of the pipelined K2
(x_maps_amd/csrc/xmaps_k2pipe.hpp) rest on when they hand the kernel arbitrary disparity frames through xm_debug_k2_group_u16:

* brute_dilate_remap / shifted_dilate_remap: the definition, as loops and vectorised (NumPy only);
* expected(tb, rect): depth and BGR of a rectified disparity frame through the oracle's A5 - A7;
* border_tables / sparse_frame (the a4 test's), pipe_tables: the same projector map on a rig that takes neither column nor
  owner tiles, with a chosen largest disparity (the pipelined kernel's LDS copy of the per-disparity table holds that many + 1);
* classify_tiles / tiled_loader_paths: k_build_k2_tables restated -- which patch loader of the tiled K2 each tile of a rig takes --
  and TILED_PATH_CASES, the shapes of tests/test_gpu_k2_tiled_paths.py that between them reach every one;
* table_tables / table_frames: the 256 x 256 identity rig and the frames that between them sample every disparity 0 .. 65535;
* steep_tables, every_pixel_frames, writable_cells: the column rigs' frames that put an event on every camera pixel in every time
  column, and the cells the ORACLE writes over them (never derived from host/xm_k2_live.hpp).

tests/test_k2_frame_cases_cpu.py pins these against each other without a GPU."""
import numpy as np

import xmaps_oracle as O
from x_maps_amd import synthetic as S


def brute_dilate_remap(rect: np.ndarray, pmap: np.ndarray) -> np.ndarray:
    """49 taps per output pixel, straight from the definition."""
    H, W = rect.shape
    ph, pw = pmap.shape[:2]
    out = np.zeros((ph, pw), np.float32)
    for v in range(ph):
        for u in range(pw):
            mx, my = int(pmap[v, u, 0]), int(pmap[v, u, 1])
            if not (0 <= mx < W and 0 <= my < H):
                continue  # BORDER_CONSTANT 0
            best = -np.inf
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    yy, xx = my + dy, mx + dx
                    if 0 <= yy < H and 0 <= xx < W:
                        best = max(best, float(rect[yy, xx]))
            out[v, u] = best
    return out


def shifted_dilate_remap(rect: np.ndarray, pmap: np.ndarray) -> np.ndarray:
    """The same definition, vectorised: the maximum over the 49 shifted views of the frame padded with -inf (cells outside the
    image never win), then the nearest remap with constant 0 outside."""
    H, W = rect.shape
    pad = np.full((H + 6, W + 6), -np.inf, np.float32)
    pad[3:H + 3, 3:W + 3] = rect
    dil = np.full((H, W), -np.inf, np.float32)
    for dy in range(7):
        for dx in range(7):
            np.maximum(dil, pad[dy:dy + H, dx:dx + W], out=dil)
    mx, my = pmap[..., 0].astype(np.int64), pmap[..., 1].astype(np.int64)
    inside = (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
    out = np.zeros(pmap.shape[:2], np.float32)
    out[inside] = dil[my[inside], mx[inside]]
    return out


def expected(tb, rect):
    """(depth, bgr) of a rectified disparity frame [rect_h][rect_w]: the definition, then the oracle's A5, A6, A7"""
    disp = shifted_dilate_remap(np.asarray(rect, np.float32), tb["disp_proj_mapxy_i16"])
    depth = O.disparity_to_depth_rectified(disp, tb["p03"])
    u8 = O.clip_normalize_uint8_depth_frame(depth, tb["z_near"], tb["z_far"])
    return depth, O.generate_color_map(u8)


def border_tables(rect_w, rect_h, proj_w, proj_h, seed):
    """Tables whose projector map sweeps from 6 px outside the rectified frame on one side to 6 px outside on the other,
    with every pixel's target jittered -- so targets sit 0,1,2,3 px from each edge and beyond it."""
    rng = np.random.default_rng(seed)
    tb = S.make_tables(S.C_TINY)
    vs, us = np.mgrid[0:proj_h, 0:proj_w].astype(np.float64)
    mx = np.rint(-6 + us * (rect_w + 12) / max(proj_w - 1, 1) + rng.integers(-2, 3, us.shape))
    my = np.rint(-6 + vs * (rect_h + 12) / max(proj_h - 1, 1) + rng.integers(-2, 3, vs.shape))
    # pin a few targets exactly onto the corners / edges
    mx[0, :4] = [0, 1, 2, 3]
    my[0, :4] = [0, 0, 0, 0]
    mx[-1, -4:] = [rect_w - 4, rect_w - 3, rect_w - 2, rect_w - 1]
    my[-1, -4:] = rect_h - 1
    mx[1, :3] = [-1, rect_w, 5]
    my[1, :3] = [5, 5, rect_h]
    tb.update({"rect_w": rect_w, "rect_h": rect_h, "proj_w": proj_w, "proj_h": proj_h,
               "disp_proj_mapxy_i16": np.ascontiguousarray(np.stack((mx, my), -1).astype(np.int16)),
               "proj_x_map": np.zeros((rect_h, tb["proj_x_map"].shape[1]), np.int16)})
    return tb, rng


def sparse_frame(rng, rect_w, rect_h, fill):
    rect = rng.integers(1, 900, (rect_h, rect_w)).astype(np.float32)
    rect[rng.random(rect.shape) >= fill] = 0
    # make sure the border cells themselves carry values (they decide the edge cases)
    rect[0, :] = rng.integers(1, 900, rect_w)
    rect[-1, :] = rng.integers(1, 900, rect_w)
    rect[:, 0] = rng.integers(1, 900, rect_h)
    rect[:, -1] = rng.integers(1, 900, rect_h)
    return rect


# ---- which loader of the tiled K2 a tile takes ----------------------------------------------------------------------------------
K2_TX, K2_TY, K2_TILE_MAX = 16, 16, 10240  # xmaps_geometry.hpp: a block is 16 x 16 threads, a patch at most 10240 cells of LDS


def classify_tiles(tb, ppt):
    """k_build_k2_tables restated: per tile of 16 * ppt x 16 projector pixels (row-major list of dicts) its `kind` -- 'empty' (no
    pixel maps into the frame), 'too_large' (the patch does not fit in LDS: the kernel reads the frame per pixel), 'interior'
    (the patch lies inside the frame) or 'border' --, the patch's `cols` and `rows_p`, and the 16-byte loads per thread that
    carry it: `loads64` of two 64-bit keys, `loads16` of eight u16 disparities."""
    pmap = tb["disp_proj_mapxy_i16"].astype(np.int64)
    rect_w, rect_h, tw = tb["rect_w"], tb["rect_h"], K2_TX * ppt
    out = []
    for v0 in range(0, pmap.shape[0], K2_TY):
        for u0 in range(0, pmap.shape[1], tw):
            mx, my = pmap[v0:v0 + K2_TY, u0:u0 + tw, 0], pmap[v0:v0 + K2_TY, u0:u0 + tw, 1]
            valid = (mx >= 0) & (mx < rect_w) & (my >= 0) & (my < rect_h)
            if not valid.any():
                out.append({"kind": "empty", "cols": 0, "rows_p": 0, "loads64": 0, "loads16": 0})
                continue
            bx, by = int(mx[valid].min()) - 3, (int(my[valid].min()) - 3) & ~7  # (3 cells of dilate margin; rows start on a multiple of 8)
            cols = int(mx[valid].max()) + 3 - bx + 1
            rows_p = (int(my[valid].max()) + 3 - by + 1 + 7) & ~7
            if cols * rows_p > K2_TILE_MAX:
                kind = "too_large"
            elif bx >= 0 and by >= 0 and bx + cols <= rect_w and by + rows_p <= rect_h:
                kind = "interior"
            else:
                kind = "border"
            nt = K2_TX * K2_TY
            out.append({"kind": kind, "cols": cols, "rows_p": rows_p, "loads64": -(-(cols * rows_p // 2) // nt),
                        "loads16": -(-(cols * rows_p // 8) // nt)})
    return out


def tiled_loader_paths(tb, ppt):
    """The patch loaders of frame_proj_tiled_body (xmaps_k2.hpp) that the rig's tiles take at `ppt` pixels per thread, as names:
    'too_large' (both formats read the frame per pixel), 'border' (both: cell by cell, or the clamped 64-bit pairs), and for
    interior patches 'u16_oct_gt8' / 'u16_oct_le8' (rect_h % 8 == 0: 16-byte loads, patches of more / at most 64 rows),
    'u16_quad' (rect_h % 8 == 4: 8-byte loads) and 'key64_un2' / '_un3' / '_un4' / '_un8' (rect_h even: the unroll the 16-byte
    loads per thread select)."""
    rect_h, names = tb["rect_h"], set()
    for t in classify_tiles(tb, ppt):
        if t["kind"] != "interior":
            names.add(t["kind"])
            continue
        if rect_h % 8 == 0:
            names.add("u16_oct_gt8" if t["rows_p"] > 64 else "u16_oct_le8")
        elif rect_h % 4 == 0:
            names.add("u16_quad")
        if rect_h % 2 == 0:
            names.add("key64_un%d" % (t["loads64"] if t["loads64"] in (3, 4) else 2 if t["loads64"] <= 2 else 8))
    return names


# (rect_w, rect_h, proj_w, proj_h) of tests/test_gpu_k2_tiled_paths.py, tables from border_tables(..., seed=rect_w): interior patches
# of 96 and 104 rows; one tile whose patch exceeds LDS; interior patches of 24 and 32 rows in 2, 3 and 4 loads per thread; interior
# tiles of a frame whose height is 4 mod 8
TILED_PATH_CASES = [(128, 256, 128, 48), (120, 104, 8, 8), (256, 64, 256, 128), (320, 64, 256, 128), (176, 132, 128, 48)]
# what they have to reach between them, per pixels-per-thread setting: every u16 loader at both, the 64-bit loader's four unroll
# variants between the two (the 24- and 32-row patches are 2 loads per thread for 16-pixel tiles, 3 and 4 for 32-pixel ones)
TILED_PATHS_WANTED = {1: {"too_large", "border", "u16_oct_gt8", "u16_oct_le8", "u16_quad", "key64_un2", "key64_un8"},
                      2: {"too_large", "border", "u16_oct_gt8", "u16_oct_le8", "u16_quad", "key64_un3", "key64_un4", "key64_un8"}}


# ---- rigs for arbitrary frames through the group frame kernel -----------------------------------------------------------------
# the depth clamp's edges on integer disparities: depth = P03 / d is z_far = 1.2 at d = 100 and z_near = 0.1 at d = 1200
# (the u8 of A6 is 255 up to d = 100, 252 at d = 101 -- no integer disparity gives 253 or 254: they need a depth in
# [1.1914, 1.2), d in (100, 100.73) --, 1 for d = 1105 .. 1150 and 0, the white pixel, from d = 1151 on)
P03, Z_NEAR, Z_FAR = 120.0, 0.1, 1.2
CLAMP_EDGES = (99, 100, 101, 1199, 1200, 1201)
U8_EDGES = (1104, 1105, 1150, 1151)


def no_tiles_x_map(tb, max_disp):
    """An X-map for a rig whose frames come from the caller, not from K1.  One entry at the int16 minimum: the reference's int16
    wrap in disp = xp - xr - x_offset could trigger, so the rig takes neither column nor owner tiles (cols_info mode 'none')
    and the pipelined K2's live mask is all ones.  One entry `max_disp` above the LUT's smallest x: the largest disparity an
    event of the rig can have, i.e. n_lds - 1 of the pipelined kernel (before XM_K2_NLDS_MAX cuts it)."""
    xm = np.zeros((tb["rect_h"], tb["proj_x_map"].shape[1]), np.int16)
    xm[0, 0] = -32768
    xp = int(tb["cam_mapx_i16"].min()) + int(tb["x_offset"]) + int(max_disp)
    assert 0 <= xp <= 32767
    xm[0, 1] = xp
    return xm


def n_lds_of(tb, nlds_max=2048):
    """what xm_create keeps of the per-disparity table in the pipelined kernel's LDS (classify_rig, host/xm_create.hpp)"""
    xr_min, x_off = int(tb["cam_mapx_i16"].min()), int(tb["x_offset"])
    max_disp = max(max(int(tb["proj_x_map"].max()), 0) - xr_min - x_off, 0 - xr_min - x_off)
    return max(1, min(max_disp + 1, 65536, nlds_max))


def pipe_tables(rect_w, rect_h, proj_w, proj_h, seed, max_disp=299):
    """border_tables on a rig without column tiles, n_lds = max_disp + 1, and the clamp edges on integer disparities"""
    tb, rng = border_tables(rect_w, rect_h, proj_w, proj_h, seed)
    tb["proj_x_map"] = no_tiles_x_map(tb, max_disp)
    tb.update({"p03": P03, "z_near": Z_NEAR, "z_far": Z_FAR})
    return tb, rng


def special_values(n_lds):
    """the disparities at which the kernel's value paths change: the ends of the LDS copy of the per-disparity table, of the
    compact key's 12 bits, of int16 and of u16, and the edges of the depth clamp and of the u8"""
    return np.array(sorted({0, 1, max(n_lds - 1, 0), n_lds, n_lds + 1, 4095, 4096, 32767, 32768, 65534, 65535, *CLAMP_EDGES, *U8_EDGES}), np.int64)


def value_frames(rng, rect_w, rect_h, n_lds):
    """u16 [4][rect_h][rect_w]: (0) the special values and random u16 mixed, 30 % of the cells, every border cell special;
    (1) the same at 5 %; (2) the special values alone on a lattice of every fourth cell, zeros between -- a window centred on a
    lattice cell holds no other one, so every special value IS some window's maximum wherever a pixel targets its cell;
    (3) half the cells with disparities up to 1300, the range in which depth and colour change with every step"""
    special = special_values(n_lds)
    shape = (rect_h, rect_w)
    out = []
    for fill in (0.3, 0.05):
        rect = np.where(rng.random(shape) < 0.5, special[rng.integers(0, len(special), shape)], rng.integers(0, 65536, shape))
        rect[rng.random(shape) >= fill] = 0
        for edge in (rect[0, :], rect[-1, :], rect[:, 0], rect[:, -1]):  # (views)
            edge[:] = special[rng.integers(0, len(special), edge.shape)]
        out.append(rect)
    lat = np.zeros(shape, np.int64)
    ys, xs = np.mgrid[0:rect_h:4, 0:rect_w:4]
    lat[::4, ::4] = special[(xs // 4 + 5 * (ys // 4)) % len(special)]
    out.append(lat)
    low = np.where(rng.random(shape) < 0.3, special[special <= 1300][rng.integers(0, int((special <= 1300).sum()), shape)],
                   rng.integers(1, 1301, shape))
    low[rng.random(shape) >= 0.5] = 0
    out.append(low)
    return np.stack(out).astype(np.uint16)


# (rect_w, rect_h, proj_w, proj_h, fill): the a4 test's shapes with rect_h a multiple of 8 (the pipelined loader's rule).  Targets
# 0 - 3 px from every edge and outside on all four sides; one-tile projectors (16 x 9, 4 x 5: gx == 1, the kernel's plain division);
# a 96 x 5 projector over 48 rows: patches that stick out of the frame above and below; a last tile of 1, 2, 3 and 18 pixels
BORDER_CASES = [(176, 136, 64, 48, 0.05), (152, 104, 50, 37, 0.3), (96, 64, 33, 70, 0.02), (40, 24, 19, 17, 0.5),
                (64, 48, 16, 9, 0.3), (64, 40, 17, 16, 0.3), (88, 48, 32, 16, 0.2), (88, 48, 96, 5, 0.1),
                (32, 24, 4, 5, 0.5), (352, 264, 128, 96, 0.4)]


def border_group(case, max_disp=299):
    """(tables, u16 [4][rect_h][rect_w]): four different sparse frames (values 1 .. 899, as the a4 test's) of a border case"""
    rect_w, rect_h, proj_w, proj_h, fill = case
    tb, rng = pipe_tables(rect_w, rect_h, proj_w, proj_h, seed=3000 + rect_w, max_disp=max_disp)
    frames = [sparse_frame(rng, rect_w, rect_h, f) for f in (fill, 0.5 * fill, min(2.0 * fill, 1.0), 0.02)]
    return tb, np.stack(frames).astype(np.uint16)


def value_group(case, nlds_max=2048, max_disp=299):
    """(tables, u16 [4][rect_h][rect_w]): the same rig with cells over the whole u16 range and at the value paths' edges"""
    rect_w, rect_h, proj_w, proj_h, fill = case
    tb, rng = pipe_tables(rect_w, rect_h, proj_w, proj_h, seed=4000 + rect_w, max_disp=max_disp)
    return tb, value_frames(rng, rect_w, rect_h, n_lds_of(tb, nlds_max))


# ---- the whole per-disparity table ------------------------------------------------------------------------------------------------
TABLE_N = 256


def table_tables(max_disp=2047):
    """a 256 x 256 rectified frame under an identity projector map (projector 256 x 256), no column tiles"""
    tb = S.make_tables(S.C_TINY)
    vs, us = np.mgrid[0:TABLE_N, 0:TABLE_N]
    tb.update({"rect_w": TABLE_N, "rect_h": TABLE_N, "proj_w": TABLE_N, "proj_h": TABLE_N,
               "disp_proj_mapxy_i16": np.ascontiguousarray(np.stack((us, vs), -1).astype(np.int16)),
               "proj_x_map": np.zeros((TABLE_N, tb["proj_x_map"].shape[1]), np.int16)})
    tb["proj_x_map"] = no_tiles_x_map(tb, max_disp)
    tb.update({"p03": P03, "z_near": Z_NEAR, "z_far": Z_FAR})
    return tb


def table_frames():
    """[3][rect_h][rect_w] u16.  The two monotone frames v[col][row] = col * 256 + row and 65535 - v: the 7 x 7 maximum is a
    corner of the window, so the value of every cell at least 3 cells from the two edges the values fall towards is some pixel's
    maximum.  A cell nearer to those edges never is (a larger neighbour sits in every window that holds it), and in BOTH frames
    these are the values with a byte below 3: 0 .. 767 and every x * 256 + {0, 1, 2}.  The third frame carries exactly those, each
    alone on a lattice of every fourth cell with zeros between: a window centred on a lattice cell holds no other one."""
    row, col = np.mgrid[0:TABLE_N, 0:TABLE_N].astype(np.int64)
    v = col * 256 + row
    missing = np.array([d for d in range(65536) if (d >> 8) < 3 or (d & 255) < 3], np.int64)
    assert len(missing) <= (TABLE_N // 4) ** 2
    third = np.zeros((TABLE_N, TABLE_N), np.int64)
    lattice = np.zeros((TABLE_N // 4) ** 2, np.int64)
    lattice[:len(missing)] = missing
    third[::4, ::4] = lattice.reshape(TABLE_N // 4, TABLE_N // 4)
    return np.stack((v, 65535 - v, third)).astype(np.uint16)


# ---- the column rigs: what the oracle itself writes ---------------------------------------------------------------------------
def steep_tables(cfg):
    """One frame column per 3 rows, the 64 time columns 4 frame columns apart: a frame column's live rows come in runs of 3
    every 12 rows, so many 8-row octets hold exactly one live cell, at their row 0 or their row 7.  The camera LUT follows the
    X-map (disparities around 30)."""
    tb = S.make_tables(cfg)
    rh, n_cols = cfg.rect_h, 64
    yr, tc = np.mgrid[0:rh, 0:n_cols].astype(np.int64)
    xmap = (S.X_OFFSET + 60 + 4 * tc + yr // 3).astype(np.int16)
    xmap[:, 0] = 0
    xmap[:6, :] = 0
    xmap[rh - 5:, :] = 0
    assert xmap.max() - S.X_OFFSET < cfg.rect_w
    ys, xs = np.mgrid[0:cfg.cam_h, 0:cfg.cam_w].astype(np.float64)
    rows = tb["cam_mapy_i16"].astype(np.float64)
    tb["cam_mapx_i16"] = np.ascontiguousarray(np.rint(30.0 + 4.0 * n_cols * (xs / cfg.cam_w) + np.floor(np.clip(rows, 0, rh) / 3.0)).astype(np.int16))
    tb["proj_x_map"] = np.ascontiguousarray(xmap)
    tb["x_map_width"], tb["t_px_scale"] = n_cols, n_cols - 1
    return tb


def every_pixel_frames(tb, cfg):
    """8 frames: frame k carries one event per time column for every camera pixel with x = k mod 8 (2 560 events per time
    column on the 160 x 128 camera: under 65 527 per tile at any tile width)"""
    n_cols = tb["proj_x_map"].shape[1]
    frames = []
    for k in range(8):
        ys, xs = np.mgrid[0:cfg.cam_h, k:cfg.cam_w:8]
        px = xs.size
        e = np.zeros(n_cols * px, dtype=S.EVENT_CD_DTYPE)
        e["x"] = np.tile(xs.reshape(-1), n_cols)
        e["y"] = np.tile(ys.reshape(-1), n_cols)
        e["t"] = 5_000_000 + np.repeat(np.arange(n_cols, dtype=np.int64), px) * 1_000  # column c exactly: (t - t0) / span * (n_cols - 1) = c
        e["p"] = 1
        frames.append(e)
    return frames


def writable_cells(tb, cfg):
    """bool [rect_h][rect_w]: the cells the oracle writes over the eight exhaustive frames (the union of the non-zero cells of its
    disp_map).  An under-approximation of 'a K1 store can reach it', from the reference's side."""
    cells = np.zeros((tb["rect_h"], tb["rect_w"]), bool)
    for e in every_pixel_frames(tb, cfg):
        x, y, t, _ = S.to_soa(e)
        cells |= O.process_ev_frame(tb, x.astype(np.int64), y.astype(np.int64), t, want_bgr=False)["disp_map"] != 0
    return cells


def column_rig(kind, proj_w):
    """(cfg, tables) of the column rigs of tests/test_gpu_k2_live.py"""
    if kind == "tall":  # patches of 9 - 10 row octets
        cfg = S.RigConfig("k2l-tall", 160, 128, proj_w, 96, 60_000)
        return cfg, S.make_tables(cfg)
    if kind == "steep":
        cfg = S.RigConfig("k2l-steep", 160, 128, proj_w, 128, 60_000)
        return cfg, steep_tables(cfg)
    cfg = S.RigConfig("k2l-cols", 160, 128, proj_w, 128, 60_000)
    return cfg, S.make_tables(cfg)
