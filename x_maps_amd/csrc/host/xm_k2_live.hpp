// xm_k2_live.hpp -- which 16-byte quads of the column tiles' u16 disparity frame can EVER be written, and, from that, one bit
// per loader slot of the pipelined K2 (xmaps_k2pipe.hpp): "this slot's quad is live".  Plain C++ (no HIP types: xm_create
// includes it, and so does the stand-alone CPU test tests/c_host/k2_live_host.cpp).
//
// The column tiles' flush stores a frame cell only through cell(row, time column) (xmaps_k1cols.hpp, step 5), for the rows
// r < xmap_h - 1 and the pairs that are live (xp - x_offset >= xr_min); every other cell of the frame is 0 from xm_create on
// and stays 0.  Which cells those are depends on the calibration alone -- the X-map, x_offset, xr_min, the frame's size and
// shear -- so it is decided once per handle, here.  A quad is 8 consecutive cells of one frame column (16 bytes, aligned:
// rect_h % 8 == 0); it is live iff it holds a live cell.  A slot whose quad is dead holds zeros whether it is loaded or not.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../xmaps_geometry.hpp"  // K2_TX, K2_TY, K2P_UN

namespace xm {

constexpr int K2L_THREADS = K2_TX * K2_TY;  // threads of a K2 block
constexpr int K2L_UN = K2P_UN;              // loader slots per thread, slot s = tid + j * K2L_THREADS
constexpr int K2L_WAVE = 64;
constexpr int K2L_WORDS = K2L_THREADS / K2L_WAVE * K2L_UN * 2;  // dwords per tile: [wave][j] a 64-bit lane mask {lo, hi}

struct K2LiveRig {
  const int16_t* xmap;  // [xmap_h][xmap_w], row-major, as the configuration holds it (xm_config.proj_x_map)
  int xmap_w, xmap_h;
  int x_offset, xr_min;  // xr_min: the smallest rectified x of the LUT (xm_handle::cols_xr_min)
  int rect_w, rect_h;
  int shear_m, shear_bias, shear_extra;  // the frame holds cell (x, row) in column x + shear_bias + ((row >> 3) * shear_m >> 12)
};

struct K2LiveTile {  // a record of k2_tiles: the tile's patch rectangle of the frame
  int bx, by, cols, rows;
};

// the flush's rule (cols_cell, xmaps_k1cols.hpp; its lean form is this one with xr_min >= 0 and rect_h >= xmap_h - 1, where
// neither the wrap nor the row test can trigger): frame column of the pair, one negative wrap like NumPy; false = never stored
inline bool k2_live_cell_column(const K2LiveRig& g, int xp, int r, int& fc) {
  const int fu = xp - g.x_offset;
  if (fu < g.xr_min) return false;
  fc = (int)(short)fu;
  if (fc < 0) fc += g.rect_w;
  return fc >= 0 && fc < g.rect_w && r < g.rect_h;
}

// frame column that holds cell (x, row) (frame16_col, xmaps_common.hpp)
inline int k2_live_frame_col(const K2LiveRig& g, int x, int row) { return x + g.shear_bias + (((row >> 3) * g.shear_m) >> 12); }

// Can the quads be told apart at all?  (whole quads only; the tiles' patches start on a multiple of 8 rows.  A frame of at most
// 32768 columns: there a live fu is its own int16 value, so cols_cell's cast and the lean flush, which stores at fu as it
// is, name the same column -- xm_create refuses wider frames anyway)
inline bool k2_live_rig_ok(const K2LiveRig& g, const K2LiveTile* tiles, size_t n_tiles) {
  if (!g.xmap || g.xmap_w <= 0 || g.xmap_h <= 0 || g.rect_w <= 0 || g.rect_h <= 0 || (g.rect_h & 7) != 0 || g.rect_w > 32768 || g.shear_extra < 0) return false;
  for (size_t i = 0; i < n_tiles; ++i)
    if (tiles[i].cols > 0 && tiles[i].rows > 0 && ((tiles[i].by & 7) != 0 || (tiles[i].rows & 7) != 0)) return false;
  return true;
}

// one byte per quad of the frame ((rect_w + shear_extra) * rect_h / 8 of them, in memory order): 1 = some pair stores into it
inline std::vector<uint8_t> k2_live_quads(const K2LiveRig& g) {
  const size_t qpc = (size_t)g.rect_h >> 3, n_cols = (size_t)(g.rect_w + g.shear_extra);
  std::vector<uint8_t> live(n_cols * qpc, 0);
  for (int r = 0; r < g.xmap_h - 1; ++r)
    for (int c = 0; c < g.xmap_w; ++c) {
      int fc;
      if (!k2_live_cell_column(g, (int)g.xmap[(size_t)r * g.xmap_w + c], r, fc)) continue;
      const int col = k2_live_frame_col(g, fc, r);
      if (col < 0 || (size_t)col >= n_cols) continue;  // (a store outside the frame's allocation: no rig has one)
      live[(size_t)col * qpc + ((size_t)r >> 3)] = 1;
    }
  return live;
}

// The loader's view: for every tile, wave and j the lanes whose slot s = wave * 64 + lane + j * 256 must be loaded.  The slot's
// quad is the one issue() (xmaps_k2pipe.hpp) addresses: patch column s / oct, row octet s % oct (oct = rows / 8), frame column
// bx + column + shear_bias + (((by >> 3) + octet) * shear_m >> 12), rows by + 8 * octet .. + 7.  Slots the loader refuses
// anyway (behind the patch's last, outside the frame) carry 0.  out: n_tiles * K2L_WORDS dwords.
inline void k2_live_mask(const K2LiveRig& g, const K2LiveTile* tiles, size_t n_tiles, std::vector<uint32_t>& out) {
  out.assign(n_tiles * (size_t)K2L_WORDS, 0u);
  if (!k2_live_rig_ok(g, tiles, n_tiles)) {  // nothing known: every slot is loaded
    out.assign(n_tiles * (size_t)K2L_WORDS, ~0u);
    return;
  }
  const std::vector<uint8_t> live = k2_live_quads(g);
  const size_t qpc = (size_t)g.rect_h >> 3;
  const int n_cols = g.rect_w + g.shear_extra;
  for (size_t t = 0; t < n_tiles; ++t) {
    const K2LiveTile& rec = tiles[t];
    if (rec.cols <= 0 || rec.rows <= 0) continue;
    const int oct = rec.rows >> 3, nslot = rec.cols * oct, g0 = rec.by >> 3;
    for (int s = 0; s < nslot && s < K2L_THREADS * K2L_UN; ++s) {
      const int c = s / oct, ro = s - c * oct;
      const int gx = rec.bx + c, gy = rec.by + 8 * ro;
      if (gx < 0 || gx >= g.rect_w || gy < 0 || gy >= g.rect_h) continue;
      const int col = gx + g.shear_bias + (((g0 + ro) * g.shear_m) >> 12);
      const bool on = col < 0 || col >= n_cols || live[(size_t)col * qpc + ((size_t)gy >> 3)] != 0;
      if (!on) continue;
      const int j = s / K2L_THREADS, tid = s - j * K2L_THREADS, wave = tid / K2L_WAVE, lane = tid - wave * K2L_WAVE;
      out[t * (size_t)K2L_WORDS + (size_t)((wave * K2L_UN + j) * 2 + (lane >> 5))] |= 1u << (lane & 31);
    }
  }
}

struct K2LiveStats {
  double cells, quads, lines;        // live fractions of the frame's cells, 16-byte quads and 128-byte lines
  double slot_quads, slot_lines;     // of the quads / distinct lines per tile the loader's slots address: the share it still loads
};

inline K2LiveStats k2_live_stats(const K2LiveRig& g, const K2LiveTile* tiles, size_t n_tiles) {
  K2LiveStats st = {1.0, 1.0, 1.0, 1.0, 1.0};
  if (!k2_live_rig_ok(g, tiles, n_tiles)) return st;
  const std::vector<uint8_t> live = k2_live_quads(g);
  const size_t qpc = (size_t)g.rect_h >> 3, n_cols = (size_t)(g.rect_w + g.shear_extra);
  {
    std::vector<uint8_t> cell(n_cols * (size_t)g.rect_h, 0);
    size_t n_cell = 0, n_quad = 0, n_line = 0, lines = (live.size() + 7) / 8;
    for (int r = 0; r < g.xmap_h - 1; ++r)
      for (int c = 0; c < g.xmap_w; ++c) {
        int fc;
        if (!k2_live_cell_column(g, (int)g.xmap[(size_t)r * g.xmap_w + c], r, fc)) continue;
        const int col = k2_live_frame_col(g, fc, r);
        if (col < 0 || (size_t)col >= n_cols) continue;
        uint8_t& b = cell[(size_t)col * g.rect_h + r];
        n_cell += b ? 0 : 1;
        b = 1;
      }
    for (size_t q = 0; q < live.size(); ++q) n_quad += live[q];
    for (size_t l = 0; l < lines; ++l) {
      bool any = false;
      for (size_t q = l * 8; q < std::min(live.size(), l * 8 + 8); ++q) any = any || live[q];
      n_line += any ? 1 : 0;
    }
    st.cells = (double)n_cell / (double)cell.size();
    st.quads = (double)n_quad / (double)live.size();
    st.lines = (double)n_line / (double)lines;
  }
  size_t sq = 0, sq_live = 0, sl = 0, sl_live = 0;
  std::vector<size_t> all_l, live_l;
  const int nc = (int)n_cols;
  for (size_t t = 0; t < n_tiles; ++t) {
    const K2LiveTile& rec = tiles[t];
    if (rec.cols <= 0 || rec.rows <= 0) continue;
    const int oct = rec.rows >> 3, nslot = rec.cols * oct, g0 = rec.by >> 3;
    all_l.clear();
    live_l.clear();
    for (int s = 0; s < nslot && s < K2L_THREADS * K2L_UN; ++s) {
      const int c = s / oct, ro = s - c * oct, gx = rec.bx + c, gy = rec.by + 8 * ro;
      if (gx < 0 || gx >= g.rect_w || gy < 0 || gy >= g.rect_h) continue;
      const int col = gx + g.shear_bias + (((g0 + ro) * g.shear_m) >> 12);
      if (col < 0 || col >= nc) continue;
      const size_t q = (size_t)col * qpc + ((size_t)gy >> 3);
      sq += 1;
      all_l.push_back(q >> 3);
      if (live[q]) {
        sq_live += 1;
        live_l.push_back(q >> 3);
      }
    }
    // (slots walk the patch in memory order, column by column: equal lines are neighbours)
    for (size_t i = 0; i < all_l.size(); ++i) sl += i == 0 || all_l[i] != all_l[i - 1];
    for (size_t i = 0; i < live_l.size(); ++i) sl_live += i == 0 || live_l[i] != live_l[i - 1];
  }
  if (sq) st.slot_quads = (double)sq_live / (double)sq;
  if (sl) st.slot_lines = (double)sl_live / (double)sl;
  return st;
}

}  // namespace xm
