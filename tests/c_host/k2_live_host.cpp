// k2_live_host.cpp -- the pipelined K2's live-slot masks (x_maps_amd/csrc/host/xm_k2_live.hpp) against a brute-force enumeration
// written another way: a std::vector<bool> over the CELLS of the frame, filled pair by pair, then every slot of every tile
// looked up cell by cell.  Hand-built rigs; stand-alone (its own main, no HIP, no GPU): tests/test_k2_live_host_cpu.py builds it
// with -fsanitize=address,undefined and runs it.  Prints "ok", or what differs and exits 1.
#include "../../x_maps_amd/csrc/host/xm_k2_live.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>

using namespace xm;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_failed < 20) {                                 \
        fprintf(stderr, "FAILED %s: ", #cond);             \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
      g_failed += 1;                                       \
    }                                                      \
  } while (0)

struct Rig {
  std::string name;
  std::vector<int16_t> xmap;
  K2LiveRig g{};
  std::vector<K2LiveTile> tiles;
};

Rig make_rig(const char* name, int xmap_w, int xmap_h, int rect_w, int rect_h, int x_offset, int xr_min,
             const std::function<int(int, int)>& frame_col_of /* (row, time column) -> xp - x_offset */) {
  Rig R;
  R.name = name;
  R.xmap.resize((size_t)xmap_w * xmap_h);
  for (int r = 0; r < xmap_h; ++r)
    for (int c = 0; c < xmap_w; ++c) R.xmap[(size_t)r * xmap_w + c] = (int16_t)(frame_col_of(r, c) + x_offset);
  R.g.xmap = nullptr;  // (set by use(): the vector may move)
  R.g.xmap_w = xmap_w; R.g.xmap_h = xmap_h; R.g.x_offset = x_offset; R.g.xr_min = xr_min;
  R.g.rect_w = rect_w; R.g.rect_h = rect_h; R.g.shear_m = R.g.shear_bias = R.g.shear_extra = 0;
  return R;
}

// a grid of patches over the frame and beyond it on all four sides: every tile's rows a multiple of 8, by a multiple of 8
void grid_tiles(Rig& R, int cols, int rows, int step_x, int step_y) {
  for (int by = -rows + 8; by < R.g.rect_h + 8; by += step_y)
    for (int bx = -cols + 3; bx < R.g.rect_w + 3; bx += step_x) R.tiles.push_back(K2LiveTile{bx, by, cols, rows});
  R.tiles.push_back(K2LiveTile{0, 0, 0, 0});    // a tile without a patch
  R.tiles.push_back(K2LiveTile{5, 8, -1, 16});  // ... and the table builder's "does not fit" mark
}

// ---- the other way round: cells first ----------------------------------------------------------------------------------
std::vector<bool> brute_cells(const K2LiveRig& g) {
  const long n_cols = (long)g.rect_w + g.shear_extra;
  std::vector<bool> cells((size_t)n_cols * (size_t)g.rect_h, false);
  for (int c = 0; c < g.xmap_w; ++c)
    for (int r = 0; r + 1 < g.xmap_h; ++r) {
      const long fu = (long)g.xmap[(size_t)r * g.xmap_w + c] - (long)g.x_offset;
      if (!(fu >= (long)g.xr_min)) continue;  // dead: no LUT entry gives disp >= 0
      long fc = ((fu + 32768L) % 65536L + 65536L) % 65536L - 32768L;  // int16, as the frame index of the reference
      if (fc < 0) fc += g.rect_w;                                     // NumPy's one wrap
      if (fc < 0 || fc >= g.rect_w || r >= g.rect_h) continue;        // (an IndexError in the reference)
      long sh = (long)(r / 8) * g.shear_m;
      sh = sh >= 0 ? sh / 4096 : -((-sh + 4095) / 4096);  // floor
      const long col = fc + g.shear_bias + sh;
      if (col < 0 || col >= n_cols) continue;
      cells[(size_t)col * (size_t)g.rect_h + (size_t)r] = true;
    }
  return cells;
}

struct Tally {
  long slots = 0, live = 0, single_row0 = 0, single_row7 = 0, dead_tiles = 0, full_tiles = 0, outside = 0;
};

Tally check_rig(Rig& R) {
  R.g.xmap = R.xmap.data();
  Tally T;
  std::vector<uint32_t> mask;
  k2_live_mask(R.g, R.tiles.data(), R.tiles.size(), mask);
  CHECK(mask.size() == R.tiles.size() * (size_t)K2L_WORDS, "%s: %zu words", R.name.c_str(), mask.size());
  if (mask.size() != R.tiles.size() * (size_t)K2L_WORDS) return T;
  const std::vector<bool> cells = brute_cells(R.g);
  const long n_cols = (long)R.g.rect_w + R.g.shear_extra;
  for (size_t t = 0; t < R.tiles.size(); ++t) {
    const K2LiveTile& rec = R.tiles[t];
    const int oct = rec.rows / 8;
    long tile_slots = 0, tile_live = 0;
    for (int j = 0; j < K2L_UN; ++j)
      for (int tid = 0; tid < K2L_THREADS; ++tid) {
        const int s = tid + j * K2L_THREADS;
        const uint32_t word = mask[t * (size_t)K2L_WORDS + (size_t)(((tid / 64) * K2L_UN + j) * 2 + (tid % 64) / 32)];
        const bool bit = (word >> (tid % 32)) & 1u;
        if (rec.cols <= 0 || oct <= 0 || s >= rec.cols * oct) continue;  // the loader refuses the slot: either value
        const int pc = s / oct, po = s % oct;                            // patch column, row octet
        const long gx = (long)rec.bx + pc, gy = (long)rec.by + 8L * po;
        if (gx < 0 || gx >= R.g.rect_w || gy < 0 || gy >= R.g.rect_h) {  // outside the frame: either value
          T.outside += 1;
          continue;
        }
        // the address issue() loads from (xmaps_k2pipe.hpp): 8 cells from there on
        const long col = gx + R.g.shear_bias + ((((long)(rec.by >> 3) + po) * R.g.shear_m) >> 12);
        CHECK(col >= 0 && col < n_cols, "%s: tile %zu slot %d reads column %ld", R.name.c_str(), t, s, col);
        if (col < 0 || col >= n_cols) continue;
        const size_t addr = (size_t)col * (size_t)R.g.rect_h + (size_t)gy;
        int n = 0, which = -1;
        for (int k = 0; k < 8; ++k)
          if (cells[addr + (size_t)k]) {
            n += 1;
            which = k;
          }
        CHECK(bit == (n > 0), "%s: tile %zu (bx %d by %d cols %d rows %d) slot %d (column %d octet %d): mask %d, %d live cells",
              R.name.c_str(), t, rec.bx, rec.by, rec.cols, rec.rows, s, pc, po, (int)bit, n);
        T.slots += 1;
        tile_slots += 1;
        if (n > 0) {
          T.live += 1;
          tile_live += 1;
        }
        if (n == 1 && which == 0) T.single_row0 += 1;
        if (n == 1 && which == 7) T.single_row7 += 1;
      }
    if (tile_slots > 0 && tile_live == 0) T.dead_tiles += 1;
    if (tile_slots > 0 && tile_live == tile_slots) T.full_tiles += 1;
  }
  // the frame's own statistics agree with the cells
  const K2LiveStats st = k2_live_stats(R.g, R.tiles.data(), R.tiles.size());
  size_t n_cell = 0;
  for (size_t i = 0; i < cells.size(); ++i) n_cell += cells[i] ? 1 : 0;
  CHECK(std::abs(st.cells - (double)n_cell / (double)cells.size()) < 1e-12, "%s: cell fraction %f", R.name.c_str(), st.cells);
  if (T.slots) CHECK(std::abs(st.slot_quads - (double)T.live / (double)T.slots) < 1e-12, "%s: slot fraction %f", R.name.c_str(), st.slot_quads);
  CHECK(st.quads >= st.cells && st.lines >= st.quads, "%s: %f %f %f", R.name.c_str(), st.cells, st.quads, st.lines);
  return T;
}

}  // namespace

int main() {
  // 1. a drift of one frame column per 3 rows, time columns 4 frame columns apart: a frame column's live rows are runs of 3 every
  //    12 rows, so octets hold exactly one live cell at their row 0 (rows 6, 7 | 8) and at their row 7 (rows 15 | 16, 17)
  {
    Rig R = make_rig("drift", 40, 97, 173, 96, 100, 0, [](int r, int c) { return 5 + 4 * c + r / 3; });
    grid_tiles(R, 37, 40, 29, 24);  // 5 octets per column: a thread's slots change column inside a wave
    grid_tiles(R, 9, 104, 11, 56);  // 13 octets, 117 slots; patches taller than the frame
    grid_tiles(R, 64, 128, 50, 64); // 16 octets, 1024 slots: all four loader registers, every wave
    const Tally T = check_rig(R);
    CHECK(T.single_row0 > 0 && T.single_row7 > 0, "drift: %ld / %ld octets with one live cell at row 0 / 7", T.single_row0, T.single_row7);
    CHECK(T.outside > 0 && T.live > 0 && T.live < T.slots, "drift: %ld of %ld slots live, %ld outside", T.live, T.slots, T.outside);
  }
  // 2. the first tiles entirely dead (nothing maps left of frame column 90), and a rig that is entirely live
  {
    Rig R = make_rig("dead-left", 30, 65, 176, 64, 7, 0, [](int r, int c) { return 90 + 2 * c + (r >> 4); });
    for (int bx = 0; bx < 176; bx += 16) R.tiles.push_back(K2LiveTile{bx, 0, 16, 64});
    const Tally T = check_rig(R);
    CHECK(T.dead_tiles >= 5 && T.dead_tiles < (long)R.tiles.size(), "dead-left: %ld dead tiles", T.dead_tiles);
    Rig L = make_rig("all-live", 50, 41, 50, 40, 0, 0, [](int, int c) { return c; });
    grid_tiles(L, 20, 24, 13, 16);
    const Tally U = check_rig(L);
    CHECK(U.live == U.slots && U.slots > 0 && U.full_tiles > 0, "all-live: %ld of %ld", U.live, U.slots);
  }
  // 3. xr_min equal to a reachable column: the pair that maps to it is live, the one a column to its left is not
  {
    Rig R = make_rig("xr-min", 2, 9, 64, 8, 11, 20, [](int, int c) { return 19 + c; });
    R.tiles.push_back(K2LiveTile{16, 0, 8, 8});
    const Tally T = check_rig(R);
    CHECK(T.live == 1 && T.slots == 8, "xr-min: %ld of %ld slots live", T.live, T.slots);
    R.g.xmap = R.xmap.data();
    const std::vector<uint8_t> q = k2_live_quads(R.g);
    CHECK(q[20] == 1 && q[19] == 0, "xr-min: quads of columns 19 / 20: %d / %d", (int)q[19], (int)q[20]);
  }
  // 4. a sheared frame (half a column per octet of rows, bias 3), odd width
  {
    Rig R = make_rig("shear", 33, 81, 131, 80, 40, 0, [](int r, int c) { return 2 + 3 * c + r / 5; });
    R.g.shear_m = 2048; R.g.shear_bias = 3; R.g.shear_extra = 3 + ((80 / 8 * 2048) >> 12) + 1;
    grid_tiles(R, 21, 48, 17, 32);
    const Tally T = check_rig(R);
    CHECK(T.live > 0 && T.live < T.slots && T.single_row0 + T.single_row7 > 0, "shear: %ld of %ld", T.live, T.slots);
    Rig N = make_rig("shear-negative", 33, 81, 131, 80, 40, 0, [](int r, int c) { return 2 + 3 * c + r / 5; });
    N.g.shear_m = -1365; N.g.shear_bias = 6; N.g.shear_extra = 8;
    grid_tiles(N, 21, 48, 17, 32);
    const Tally V = check_rig(N);
    CHECK(V.live > 0 && V.live < V.slots, "shear-negative: %ld of %ld", V.live, V.slots);
  }
  // 5. a negative frame column with NumPy's one wrap (xr_min < 0), and X-map cells that are dead (below xr_min)
  {
    Rig R = make_rig("wrap", 24, 49, 101, 48, 30, -6, [](int r, int c) { return -9 + c * 2 + (r & 1); });
    grid_tiles(R, 30, 16, 25, 8);
    const Tally T = check_rig(R);
    R.g.xmap = R.xmap.data();
    const std::vector<uint8_t> q = k2_live_quads(R.g);
    const size_t qpc = 48 / 8;
    CHECK(q[(size_t)(101 - 6) * qpc] == 1 && q[(size_t)(101 - 7) * qpc] == 0 && q[(size_t)(101 - 1) * qpc] == 1, "wrap: columns -6 / -7 / -1");
    CHECK(T.live > 0 && T.live < T.slots, "wrap: %ld of %ld", T.live, T.slots);
  }
  // 6. rows of the X-map beyond the frame (rect_h < xmap_h - 1) are never stored; the last X-map row never holds a winner
  {
    Rig R = make_rig("short-frame", 20, 60, 77, 40, 3, -1, [](int r, int c) { return r < 58 ? 70 : c; });
    R.xmap[(size_t)59 * 20 + 4] = (int16_t)(10 + 3);  // the last row alone maps to column 10: not live
    grid_tiles(R, 12, 24, 10, 16);
    const Tally T = check_rig(R);
    R.g.xmap = R.xmap.data();
    const std::vector<uint8_t> q = k2_live_quads(R.g);
    size_t n = 0;
    for (uint8_t b : q) n += b;
    CHECK(n == 40 / 8, "short-frame: %zu live quads", n);
    CHECK(T.live > 0, "short-frame: %ld", T.live);
  }
  // 7. a patch that does not start on a multiple of 8 rows: nothing is derived, every slot is loaded
  {
    Rig R = make_rig("unaligned", 8, 17, 32, 16, 0, 0, [](int, int c) { return c; });
    R.tiles.push_back(K2LiveTile{0, 4, 8, 8});
    R.g.xmap = R.xmap.data();
    std::vector<uint32_t> mask;
    k2_live_mask(R.g, R.tiles.data(), R.tiles.size(), mask);
    bool ones = mask.size() == (size_t)K2L_WORDS;
    for (uint32_t w : mask) ones = ones && w == ~0u;
    CHECK(ones, "unaligned: not all ones");
  }
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  puts("ok");
  return 0;
}
