// xm_plan.hpp -- what xm_create decides about a rig (RigPlan), and every rule that picks a frame's kernels and their launch
// shapes from it: which path a frame or a group takes (frame_path), and the grid, block and dynamic LDS of K0 / K0b, K1 and K2.
// Plain C++ (no HIP types: the library's one translation unit includes it, and so does the stand-alone CPU test
// tests/c_host/plan_host.cpp).  The rules take a const RigPlan& and, where the answer depends on the moment, a PathNow;
// they return values and touch nothing.  The launchers (xm_launch.hpp, xm_enqueue.hpp) choose the template instance and pass
// the arguments; every number of a launch comes from here.
//
// The kernels' constants and LDS layouts the rules need are the kernels' own: ../xmaps_geometry.hpp defines each once, for both.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../../include/xmaps.h"
#include "../xmaps_geometry.hpp"

namespace xm {

constexpr int OWN_PLANS = 3;  // owner tiles: up to three plans by falling tile width (xm_own_plan.hpp)

// ---- what xm_create decided about the rig: written by its stages (xm_create.hpp), read-only from create_slots on ---------------
struct RigPlan {
  struct Dims {
    int cam_w = 0, cam_h = 0, proj_w = 0, proj_h = 0, rect_w = 0, rect_h = 0, xmap_w = 0, xmap_h = 0, x_offset = 0;
    bool projector = true;  // cfg.view == XM_VIEW_PROJECTOR
    size_t key_cells = 0;   // cells of the fused path's key frame (rect or camera frame)
    int out_w = 0, out_h = 0;
    int n_cus = 256;        // CUs of the device
    bool has_pmap = false;  // the rig came with a projector map (d_pmap)
  } dims;
  struct Modes {
    bool time_sorted = false;  // XM_FLAG_TIME_SORTED
    bool try_sorted = false;   // XM_FLAG_TRY_SORTED
    bool k1_direct = false;    // "XM_K1_DIRECT", or tables too tall for LDS: every event takes the direct path
    bool k2_direct = false;    // "XM_K2_DIRECT"
    bool k2_flags = false;     // "XM_K2_FLAGS"=1: K1 marks dirty 128-byte lines of the key frame, K2 skips clean ones.
                               // Measured: K2 fetches 37 % fewer bytes but is not faster (it is latency, not bandwidth bound)
  } modes;
  // K1 tiling: LDS windows (time columns / camera columns) and the dynamic LDS they need; 0 = direct kernel
  struct K1 {
    int w_ts = 0, w_x = 0;
    size_t lds = 0;
  } k1;
  struct Compact {
    bool key32_ok = false;  // the rig qualifies for the compact key frame (projector view, rect_h % 4 == 0, disparities < 4096)
  } compact;
  // column-tile K1 (xmaps_k1cols.hpp): the rig qualifies (projector view, cell(row, column) injective, no int16 wrap in the
  // disparity arithmetic), smallest rectified x of the LUT, widest tile the LDS budget allows, events a tile should hold
  struct Cols {
    bool ok = false;
    bool single = false;  // XM_COLS=2: also for single-frame calls (default: groups of frames only -- a single frame's third
                          // launch, the boundary pass, costs the pipelined one-frame-per-call path more than the tiles save)
    int xr_min = 0, w_max = 0, target = 3700;
    int xr_max = 0;   // largest rectified x of the LUT (xr_min: its smallest): the ingest's FirstEventPerYT cell map is this + 1 wide
    int lds_pad = 0;  // "XM_COLS_LDS_PAD" (experiments): bytes of dynamic LDS a column-tile block asks for beyond its carve-up
    int flags = 0;    // COLS_F_ALL_IN_FRAME when no live (row, column) pair of the rig maps outside the frame
    // owner tiles (xmaps_k1own.hpp): the rig's (row, column) -> cell map is not injective (the reference's own calibration), but
    // every cell's columns lie within a few (<= 7) columns of its first one: ok with own_mode set; tile widths and halos per plan
    bool own_mode = false;
    int own_ept_forced = 0;  // "XM_OWN_EPT" (experiments): 4 = four events per thread where a tile then fits one pass
  } cols;
  // the owner tiles' plans (own_setup), by falling tile width: ownership per 8-row group on tiles of 20 and of 16 columns -- frames
  // whose tiles fit one event pass of a block --, then ownership per row on tiles of 8 -- denser frames, and rigs whose slant
  // rules the first two out.  All write the same frame (every cell a pair maps to, every frame), so consecutive frames of a slot
  // may take different plans.  (Their device tables: xm_handle::own[i].)
  struct Own {
    bool ok = false, all_in = false;
    int w = 0, halo = 0, extras = 0;
    int r_lo = 0, hr = 0, hrp = 0, rp = 0, grouped = 0, nxs_max = 0, extra_max = 0;
  } own[OWN_PLANS];
  struct K2 {
    bool has_tables = false;  // the tiled frame kernel's per-tile / per-pixel tables exist (a projector map: d_k2_tiles)
    int tile_cap[3] = {K2_TILE_MAX, K2_TILE_MAX, K2_TILE_MAX};  // cells of the largest K2 patch (multiple of 8), per geometry
    int patch_cols_max = 0;  // widest patch of the 16 x 16 / 32 x 16 tiles (-1: some patch does not fit LDS)
    int force_ppt = 0;       // "XM_K2_PPT"=1/2: experiments
  } k2;
  // pipelined K2 of the group launches (xmaps_k2pipe.hpp)
  struct K2Pipe {
    bool on = true;          // "XM_K2_PIPE"=0: off
    bool force = false;      // "XM_K2_PIPE"=2 (tests): also for groups too small for the pipeline to matter
    bool rig_ok = false;     // every tile's patch fits the pipelined loader, rect_h % 8 == 0
    int g = 1;               // its geometry: tiles of 16 << g pixels x 16 rows (2 / 4 pixels per thread)
    int nlds = 0;            // entries of the per-disparity table kept in LDS
    int per_cu_max = 8;      // "XM_K2_PER_CU": its blocks per CU at most (what it leaves, the next group's K1 can take)
    int blocks_cap = 0;      // "XM_K2_PIPE_BLOCKS" (tests): at most this many persistent blocks, so that each walks several items; 0 = no cap
    int consec = -1;         // k_frame_proj_pipe<PPT, true>: PPT consecutive pixels per thread; -1 = where it measured faster (PPT = 4), "XM_K2_CONSEC"=0|1 forces
    bool has_pix16[3] = {false, false, false};  // the kernel's u16 copy of the pixel table exists (d_k2_pix16[g])
    int pix_stride = 0;      // its row stride
    // "XM_K2_CHAIN": the pipelined K2 launches of different groups (different streams) wait for each other -- one K2 at a time, at
    // per_cu_max blocks per CU, and the following groups' boundary pass and K1 in what it leaves (profiles/r05_own_tiles.md)
    bool chain = false;
    bool live = true;          // "XM_K2_LIVE"=0: all-ones live-slot masks (the same kernel, for tests and A/B runs)
    bool live_report = false;  // "XM_K2_LIVE"=2: the derived masks, and their live fractions on stderr (profiles)
  } k2pipe;
};

// what a path rule may know about the moment besides the rig
struct PathNow {
  bool capturing = false;       // inside xm_graph_create's stream capture (no host-side redo possible there)
  bool compact_paused = false;  // the compact paths are switched off for a while (they kept failing: sparse / noisy stream)
};

struct EventsView {
  const uint16_t* x = nullptr;
  const uint16_t* y = nullptr;
  const void* t = nullptr;
  const int16_t* p = nullptr;
  const void* aos = nullptr;
  size_t n = 0;
  int t_dtype = XM_T_INT64;
  bool use_p = false;
};

inline unsigned grid_for(uint64_t items, unsigned per_block) {
  uint64_t g = (items + per_block - 1) / per_block;
  return (unsigned)(g ? g : 1);
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// SoA columns that take 16-byte loads
inline bool ev_vec16(const EventsView& ev) {
  return !ev.aos && aligned(ev.x, 16) && aligned(ev.y, 16) && aligned(ev.t, 16) && (!ev.use_p || aligned(ev.p, 16));
}

// ---- K0 (extrema) ---------------------------------------------------------------------------------------------------------------
// blocks per frame: ~2048 events per thread-block iteration keeps every CU busy without drowning the 32 atomic slots (VEC2: K0_UN
// loads x 2 events per thread per sweep); a grid-stride kernel, so the grid is capped
inline unsigned k0_blocks(uint64_t n, bool vec2, unsigned cap) {
  const unsigned g = grid_for(n, BLOCK * (vec2 ? 2 * K0_UN : 4));
  return g > cap ? cap : g;
}
// VEC2 (16-byte loads of int64 SoA time stamps): a lone frame needs its t (and p) aligned (a group: every column of every frame)
inline bool k0_vec2(const EventsView& ev) { return aligned(ev.t, 16) && (!ev.use_p || aligned(ev.p, 4)); }

// ---- K1 (scatter): tiled, or one thread per event --------------------------------------------------------------------------------
// The tiled kernel pays a fixed price per block (copy the bands, clear + scan w_ts * xmap_h slots), so it needs blocks of >= 1024
// events whose time slice still fits the LDS window of w_ts X-map columns.  A frame of n events spreads over xmap_w columns: a
// block of E events spans about E * xmap_w / n of them.  Dense frames (C-1M: 1 M events / 640 columns) get 4096-event blocks;
// sparse ones (ESL-like: 150 K events / 1080 columns, < 1 event per slot, nothing to de-duplicate) go to the one-thread-per-event
// kernel, whose cost is proportional to n.
inline double k1_block_events(const RigPlan& p, uint64_t n) {  // the most events a block of a frame of n events may take
  return p.dims.xmap_w > 0 ? (p.k1.w_ts - 1.5) * (double)n / (double)p.dims.xmap_w : 0.0;
}
inline bool tiled_path(const RigPlan& p, uint64_t n) {  // dense enough for the tiled K1?
  return !p.modes.k1_direct && p.k1.w_ts > 0 && p.k1.w_x > 0 && k1_block_events(p, n) >= 1024.0;
}
inline unsigned k1_threads(const RigPlan& p, uint64_t n) {  // the tiled K1's block for frames of n events
  const double max_ev = k1_block_events(p, n);
  unsigned threads = TILE_THREADS;
  while (threads > 1024 / TILE_EPT && (double)(threads * TILE_EPT) > max_ev) threads >>= 1;  // smallest block: 1024 events
  return threads;
}
// the tiled K1's launch: block size from the mean frame (a sparser frame of a group only sends more of its events down the direct
// path in the kernel), blocks for the largest; redo: the redo node of a captured group, at most 32 blocks per frame
struct K1TiledShape {
  unsigned threads, gx;
  size_t lds;
};
inline K1TiledShape k1_tiled_shape(const RigPlan& p, uint64_t n_max, uint64_t n_mean, bool redo) {
  K1TiledShape s;
  s.threads = k1_threads(p, n_mean);
  s.gx = grid_for(n_max, s.threads * TILE_EPT);
  if (redo) s.gx = std::min(s.gx, 32u);
  s.lds = p.k1.lds;
  return s;
}
// the one-thread-per-event K1: blocks of a frame of n events (vec4: the lone frame's kernel that takes four events per thread)
inline unsigned k1_direct_blocks(uint64_t n, bool vec4) { return grid_for(n, vec4 ? BLOCK * 4 : BLOCK); }

// ---- column / owner tiles ------------------------------------------------------------------------------------------------------------
// owner tiles: the plan a frame of n events takes -- the default plan (wide tiles) while a tile's own + halo columns fit ONE event
// pass of a block (8 events x 512 threads: past that a tile looks its events up again for every row pass); denser frames take
// the next plan's narrower tiles
inline int own_pick(const RigPlan& p, uint64_t n) {
  const double per_col = (double)n / (double)p.dims.xmap_w;
  int pick = 0;  // (the mean tile: measured on the ESL-like frames at 94 % of a block's events, the fuller tiles' second pass included)
  while (pick + 1 < OWN_PLANS && p.own[pick + 1].ok &&
         per_col * (p.own[pick].w + p.own[pick].halo) > (double)(COLS_EPT * COLS_MAX_THREADS))
    pick += 1;
  return pick;
}

// time columns per tile for frames of n events: about cols.target events per tile, within the LDS budget; 0 = not this path
inline int cols_width(const RigPlan& p, uint64_t n) {
  if (p.cols.ok && p.cols.own_mode) {  // owner tiles: the widths the ownership tables are built for; not for nearly empty frames
    const RigPlan::Own& os = p.own[own_pick(p, n)];
    const uint64_t tiles = grid_for(p.dims.xmap_w, os.w);
    return n >= tiles * 128 && n < (1ull << 28) ? os.w : 0;
  }
  if (!p.cols.ok || p.cols.w_max < 1 || p.dims.xmap_w < 1 || n == 0 || n >= (1ull << 28)) return 0;
  const double per_col = (double)n / (double)p.dims.xmap_w;
  int W = (int)((double)p.cols.target / per_col);
  W = std::max(1, std::min(W, p.cols.w_max));
  if (per_col * W < 1024.0) return 0;  // sparse frames: the band copies and the slot scan would dominate (direct kernel instead)
  return W;
}

// the plan whose tiles are W columns wide (cols_width picked it): its index in RigPlan::own / xm_handle::own
inline int own_index(const RigPlan& p, int W) {
  for (int i = 1; i < OWN_PLANS; ++i)
    if (p.own[i].ok && p.own[i].w == W) return i;
  return 0;
}

// owner tiles: events per thread -- eight; four (twice the waves at half the registers for the same tile: xmaps_k1own.hpp) measured
// the same within the noise (profiles/r05_own_tiles.md) and is kept as an experiment switch ("XM_OWN_EPT" = 4; not for 16-byte SoA loads)
inline int own_ept(const RigPlan& p, uint64_t n, int W, bool vec16) {
  if (vec16 || p.cols.own_ept_forced != 4) return 8;
  const double per = (double)n / (double)p.dims.xmap_w * (W + p.own[own_index(p, W)].halo);
  return per * 1.12 <= 4.0 * COLS_MAX_THREADS ? 4 : 8;
}

inline unsigned cols_threads(const RigPlan& p, uint64_t n, int W, int ept = COLS_EPT) {
  if (p.cols.own_mode) {  // own + halo columns in one pass where 512 threads hold them
    const double per = (double)n / (double)p.dims.xmap_w * (W + p.own[own_index(p, W)].halo);
    const unsigned t = ((unsigned)(per * 1.12 / ept) + 63u) / 64u * 64u;
    return std::max(128u, std::min(t, (unsigned)COLS_MAX_THREADS));
  }
  const double per_tile = (double)n / (double)p.dims.xmap_w * W;
  // one pass for a tile 12 % above the mean (Poisson spread of an evenly filled scan); fuller tiles take a second pass.
  // Tiles of more than 2048 events get the full 512 threads even when 448 would hold them: three blocks per CU are then
  // 24 waves = every wave slot the kernel's 80 VGPRs allow (measured at C-1M, 3125 events per tile: 4.35 instead of 4.63 us
  // per frame at full occupancy; 384 threads = two passes: 5.9 us)
  unsigned t = ((unsigned)(per_tile * 1.12 / COLS_EPT) + 63u) / 64u * 64u;
  if (t > 256u) t = COLS_MAX_THREADS;
  return std::max(128u, std::min(t, (unsigned)COLS_MAX_THREADS));
}

// dynamic LDS of a column-tile block and of an owner-tile block: the pieces the kernels carve (xmaps_geometry.hpp), summed
inline size_t cols_lds_bytes_at(int w_x, int cam_h, int xmap_h, int W) {
  return 16 * ((size_t)band_lut_q(w_x, cam_h) + (size_t)band_xm_q(W, xmap_h) + (size_t)cols_slot_q(W, xmap_h));
}
inline size_t cols_lds_bytes(const RigPlan& p, int W) { return cols_lds_bytes_at(p.k1.w_x, p.dims.cam_h, p.dims.xmap_h, W); }

inline size_t own_plan_lds_bytes(int nxs_max, int rp, int hrp, int extra_max, bool grouped) {
  return 4 * ((size_t)own_band_words(nxs_max, rp) + (size_t)own_extra_words(extra_max) + (size_t)own_tab_words(hrp, grouped));
}
inline size_t own_lds_bytes(const RigPlan::Own& os) {
  return own_plan_lds_bytes(os.nxs_max, os.rp, os.hrp, os.extra_max, os.grouped != 0);
}

// K0b: the tile boundaries + column thresholds of the frame(s), left behind the u16 frame.  Column tiles: one boundary per tile, 16
// lanes each on tiles of <= 16 columns, else 32 (cols_bounds_per_block); owner tiles: two per tile (its first column, the end of its
// halo behind it), 32 lanes.  own: the owner tiles' plan (-1: column tiles)
struct BoundsShape {
  int own, split;  // split: the plan's halo (0: column tiles)
  unsigned nb;     // boundaries
  int lanes;       // 16 / 32 per boundary
  unsigned gx;     // blocks of 256 threads (per frame)
};
inline BoundsShape cols_bounds_shape(const RigPlan& p, int W) {
  BoundsShape s;
  s.own = p.cols.own_mode ? own_index(p, W) : -1;
  s.split = s.own >= 0 ? p.own[s.own].halo : 0;
  s.nb = (s.split ? 2u : 1u) * grid_for(p.dims.xmap_w, W);
  s.lanes = !s.split && W <= 16 ? 16 : 32;
  s.gx = grid_for(s.nb + 1, cols_bounds_per_block(s.lanes));
  return s;
}

// K1 on the column tiles or the owner tiles: grid = tiles (x frames), block from the mean frame (cols_threads).  lds_pad: extra
// dynamic LDS of a column-tile block ("XM_COLS_LDS_PAD": the groups' launch only)
struct TilesK1Shape {
  int own;  // the owner tiles' plan (-1: column tiles)
  int halo, ept;
  unsigned gx, threads;
  size_t lds;
  int flags;  // the rig's own (cols.flags) on top of the caller's
};
inline TilesK1Shape tiles_k1_shape(const RigPlan& p, uint64_t n_mean, int W, bool v16, int flags, size_t lds_pad) {
  TilesK1Shape s;
  s.gx = grid_for(p.dims.xmap_w, W);
  s.flags = flags | p.cols.flags;
  if (p.cols.own_mode) {
    s.own = own_index(p, W);
    s.halo = p.own[s.own].halo;
    s.ept = own_ept(p, n_mean, W, v16);
    s.lds = own_lds_bytes(p.own[s.own]);
    s.threads = cols_threads(p, n_mean, W, s.ept);
  } else {
    s.own = -1;
    s.halo = 0;
    s.ept = COLS_EPT;
    s.lds = cols_lds_bytes(p, W) + lds_pad;
    s.threads = cols_threads(p, n_mean, W);
  }
  return s;
}

// ---- which path a frame or a group takes -----------------------------------------------------------------------------------------
inline bool sorted_path(const RigPlan& p, PathNow now, const EventsView& ev) {
  // the verified (t[0], t[n-1]) shortcut: both K1 kernels take it (tiled, and one thread per event for sparse frames)
  return (p.modes.time_sorted || (p.modes.try_sorted && !now.capturing)) && !ev.use_p && ev.n > 0;
}

// may this (sorted-path) frame use the compact key frame?  Needs the automatic redo (try-sorted mode, not inside a capture)
inline bool key32_path(const RigPlan& p, PathNow now, const EventsView& ev, bool sorted) {
  if (!sorted || !p.compact.key32_ok || !p.modes.try_sorted || now.capturing || now.compact_paused || p.modes.k2_direct ||
      p.modes.k2_flags || !tiled_path(p, ev.n))
    return false;
  if (!p.dims.projector) return ev.n <= (uint64_t)CAM32_MAX_EVENTS;  // the key's order field is the event index
  return ev.n / (uint64_t)(1024 / TILE_EPT * TILE_EPT) < (1ull << KEY32_TILE_BITS);  // tiles of >= 1024 events
}

// the column tiles' conditions on a frame: int64 time stamps, no polarity column, dense enough for a tile width of its own
inline bool cols_events(const RigPlan& p, const EventsView& ev) {
  return !ev.use_p && (ev.aos || ev.t_dtype == XM_T_INT64) && cols_width(p, ev.n) != 0;
}

// can this group of frames go through the multi-frame kernels?  (dense enough for the tiled K1, tiled K2 available)
inline bool batch_path(const RigPlan& p, uint64_t n_mean) {
  return tiled_path(p, n_mean) && !(p.dims.projector && p.modes.k2_direct) && !p.modes.k2_flags;
}

// kmode of a frame: 0 = 64-bit key frame (general), 1 = compact 32-bit key frame, 2 = column tiles + plain u16 frame
enum { KM_KEY64 = 0, KM_KEY32 = 1, KM_COLS = 2 };

struct FramePath {
  bool per_frame = false;  // a group without a multi-frame path (untiled K2): frame by frame through enqueue_frame
  bool sorted = false;     // the verified (t[0], t[n-1]) shortcut: no K0
  bool direct = false;     // a group too sparse for the tiles: the one-thread-per-event K1 between the multi-frame K0 and K2
  int cols_w = 0;          // column / owner tiles of this width (0: none)
  bool dev_redo = false;   // a captured group on the column tiles: the redo decided on the device (launch_group)
  bool key32 = false;      // the compact key frame
  uint64_t n_max = 0, n_mean = 0;
  bool vec16 = true;       // every SoA frame's columns 16-byte aligned
  int kmode() const { return cols_w ? KM_COLS : key32 ? KM_KEY32 : KM_KEY64; }
  int counter() const { return cols_w ? 3 : key32 ? 2 : sorted ? 1 : 0; }  // index into xm_handle::path_counts
};

// The path of a lone frame (group = false) or of a group of n frames.  A group adds its own conditions on top of a lone frame's:
// the multi-frame kernels, or the one-thread-per-event K1 (>= 2 frames), or none; one tile width for all its frames (from the mean
// frame) and one layout (AoS / SoA); and while it is being captured (can_redo: descriptors for the redo at hand, >= 2 frames --
// a lone frame's seven launches, four of them returning at once, take longer than K0 -> K1 -> K2) the column tiles with the
// redo decided on the device.  A lone frame takes the column tiles only under cols.single.
inline FramePath frame_path(const RigPlan& rp, PathNow now, const EventsView* evs, int n, bool allow_sorted, bool group = false,
                            bool can_redo = false) {
  FramePath p;
  uint64_t n_sum = 0;
  bool one_layout = true;
  p.sorted = allow_sorted && n > 0;
  for (int f = 0; f < n; ++f) {
    const EventsView& ev = evs[f];
    p.n_max = std::max<uint64_t>(p.n_max, ev.n);
    n_sum += ev.n;
    if (!ev.aos) p.vec16 = p.vec16 && ev_vec16(ev);
    p.sorted = p.sorted && sorted_path(rp, now, ev);
    one_layout = one_layout && (ev.aos != nullptr) == (evs[0].aos != nullptr);
  }
  p.n_mean = n ? n_sum / (uint64_t)n : 0;
  const bool k2_untiled = rp.modes.k2_direct || rp.modes.k2_flags;
  if (group) {
    // frames too sparse for the tiled K1 (the reference's own recordings: ~150 k events over 1080 time columns): the multi-frame
    // K0 and K2 with the one-thread-per-event K1 in between -- three launches per group instead of three per frame
    const bool tiled = batch_path(rp, p.n_mean);
    p.direct = !tiled && !(rp.dims.projector && (rp.modes.k2_direct || !rp.k2.has_tables)) && !rp.modes.k2_flags && n >= 2 &&
               p.n_max < (1ull << 31);
    p.per_frame = !tiled && !p.direct;
    if (p.per_frame) return p;
  }
  auto tile_width = [&] {
    int W = one_layout ? cols_width(rp, p.n_mean) : 0;
    for (int f = 0; f < n && W; ++f)
      if (!cols_events(rp, evs[f])) W = 0;
    return W;
  };
  // the column tiles need the automatic redo at hand on the host, as the compact key frame does
  if (p.sorted && (group || rp.cols.single) && rp.cols.ok && rp.modes.try_sorted && !now.capturing && !now.compact_paused && !k2_untiled)
    p.cols_w = tile_width();
  else if (group && can_redo && n >= 2 && now.capturing && !p.direct && rp.cols.ok && !k2_untiled)
    p.dev_redo = (p.cols_w = tile_width()) != 0;
  p.key32 = p.sorted && !p.cols_w && !p.direct;
  for (int f = 0; f < n && p.key32; ++f) p.key32 = key32_path(rp, now, evs[f], p.sorted);
  return p;
}

// ---- K2 (tiled frame kernel, projector view) ------------------------------------------------------------------------------------
// Pixels per thread of a launch over n_frames frames: two (32 x 16-pixel tiles) when the launch fills the chip several times
// over -- a K2 wave is a chain of dependent round trips, what it costs there is resident waves x lifetime, so each wave carries
// two pixels through the chain --, one (16 x 16) for a lone small frame, where the chain's length IS the kernel's duration and
// twice the blocks start at once (C-1M, one frame: 7.3 us with one pixel per thread, 12.3 with two).
inline int k2_ppt(const RigPlan& p, int n_frames) {
  if (p.k2.force_ppt == 1 || p.k2.force_ppt == 2) return p.k2.force_ppt;
  const uint64_t blocks2 = (uint64_t)grid_for(p.dims.proj_w, 2 * K2_TX) * grid_for(p.dims.proj_h, K2_TY) * (uint64_t)std::max(n_frames, 1);
  // measured at C-1M (600 blocks of 32 x 16 pixels per frame, tools/ppt_threshold.sh), K2 us per launch with one / two pixels per
  // thread: 1 frame 5.3 / 7.2, 2 frames 8.7 / 8.6, 3: 11.1 / 10.6, 8: 23.4 / 21.3, 16: 47.5 / 41.1 -- the crossover is at about
  // four blocks per CU
  return blocks2 >= 1024 ? 2 : 1;
}

// K2's dynamic LDS: the tile's patch of u16 disparities (the row maxima replace it in place) + the overrun of its last read
inline size_t k2_lds_bytes(const RigPlan& p, int ppt) { return (size_t)k2_patch_hw(p.k2.tile_cap[ppt - 1]) * sizeof(uint16_t); }

// the tiled K2's launch over n_frames frames (a lone frame: 1): blocks of K2_TX * K2_TY threads.  redo: the redo node of a captured
// group -- a few blocks per frame walk its tiles
struct K2TiledShape {
  int ppt, tile_cap;
  unsigned gx, gy, gz;
  unsigned threads;
  size_t lds;
};
inline K2TiledShape k2_tiled_shape(const RigPlan& p, int n_frames, bool redo = false) {
  K2TiledShape s;
  s.ppt = k2_ppt(p, n_frames);
  s.tile_cap = p.k2.tile_cap[s.ppt - 1];
  s.gx = grid_for(p.dims.proj_w, K2_TX * s.ppt);
  s.gy = grid_for(p.dims.proj_h, K2_TY);
  s.gz = (unsigned)n_frames;
  if (redo) s.gx = std::min(s.gx * s.gy, 32u), s.gy = 1;
  s.threads = K2_TX * K2_TY;
  s.lds = k2_lds_bytes(p, s.ppt);
  return s;
}

// the software-pipelined K2 (persistent blocks walking (frame, tile) items): groups on the plain u16 frame
inline size_t k2_pipe_lds_bytes(const RigPlan& p, int g) {
  return (size_t)k2p_dlut_off_hw(p.k2.tile_cap[g]) * sizeof(uint16_t) + (size_t)p.k2pipe.nlds * K2P_DLUT_ENTRY_BYTES;
}

// does a group of n_frames take the pipelined K2, and in which shape?  (use = false: the tiled K2, one block per tile)
struct K2PipeShape {
  bool use = false;
  int g = 0, ppt = 0;
  uint32_t gx = 0, gy = 0;
  unsigned blocks = 0;
  size_t lds = 0;
  uint32_t gx_magic = 0;     // divmod(tile, gx) by a multiply in the kernel: exact while tile * gx < 2^32; 0 = divide
  bool consecutive = false;  // consecutive pixels per thread (default: on the 64 x 16 tiles)
};
inline K2PipeShape k2_pipe_shape(const RigPlan& p, int n_frames) {
  K2PipeShape s;
  const RigPlan::K2Pipe& k = p.k2pipe;
  if (!k.on || !k.rig_ok || k.nlds < 1 || (k2_ppt(p, n_frames) != 2 && !k.force)) return s;
  s.g = k.g, s.ppt = 1 << s.g;
  s.gx = grid_for(p.dims.proj_w, K2_TX * s.ppt), s.gy = grid_for(p.dims.proj_h, K2_TY);
  const uint64_t total = (uint64_t)s.gx * s.gy * (uint64_t)n_frames;
  s.lds = k2_pipe_lds_bytes(p, s.g);
  const unsigned per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)k.per_cu_max, (160 * 1024) / (s.lds + 2048)));
  s.blocks = (unsigned)p.dims.n_cus * per_cu / 8 * 8;
  if (total < 3ull * s.blocks && !k.force) return s;  // too few items per block for the pipeline to matter: one block per tile
  s.blocks = (unsigned)std::min<uint64_t>(s.blocks, std::max<uint64_t>(total, 1));
  if (k.blocks_cap > 0) s.blocks = std::min(s.blocks, (unsigned)k.blocks_cap);  // (tests: any grid is legal -- items are (f, b) with stride gridDim.x)
  s.gx_magic = s.gx > 1 && (uint64_t)s.gx * s.gy * s.gx < (1ull << 32) ? (uint32_t)(((1ull << 32) + s.gx - 1) / s.gx) : 0u;
  s.consecutive = (k.consec < 0 ? s.g >= 2 : k.consec != 0) && k.has_pix16[s.g];
  s.use = true;
  return s;
}

// ---- the frame kernels without tiles ------------------------------------------------------------------------------------------------
// camera view on the compact key frame: blocks of CAM32_T x CAM32_T pixels
inline unsigned cam32_gx(const RigPlan& p) { return grid_for(p.dims.cam_w, CAM32_T); }
inline unsigned cam32_gy(const RigPlan& p) { return grid_for(p.dims.cam_h, CAM32_T); }
// one thread per pixel: camera view on the 64-bit keys, projector view under "XM_K2_DIRECT"
inline uint64_t cam_pixels(const RigPlan& p) { return (uint64_t)p.dims.cam_w * p.dims.cam_h; }
inline unsigned pixel_blocks(uint64_t px) { return grid_for(px, BLOCK); }

// ---- xm_create's arithmetic ---------------------------------------------------------------------------------------------------------
// smallest / largest entry of the LUT's rectified x and of the X-map
struct TableExtrema {
  int xr_min = 32767, xr_max = -32768, xp_min = 32767, xp_max = -32768;
};
inline TableExtrema table_extrema(const int16_t* cam_mapx, size_t cam_px, const int16_t* proj_x_map, size_t xm_cells) {
  TableExtrema e;
  for (size_t i = 0; i < cam_px; ++i) {
    e.xr_min = std::min<int>(e.xr_min, cam_mapx[i]);
    e.xr_max = std::max<int>(e.xr_max, cam_mapx[i]);
  }
  for (size_t i = 0; i < xm_cells; ++i) {
    e.xp_min = std::min<int>(e.xp_min, proj_x_map[i]);
    e.xp_max = std::max<int>(e.xp_max, proj_x_map[i]);
  }
  return e;
}

// What the tables' extrema allow.  key32_ok: the compact (32-bit) key frame's arithmetic conditions (see key32_tag in
// xmaps_common.hpp; camera view: (event index + 1) << 12 | disparity on the camera frame -- only the disparity range matters);
// xm_create adds the switch and, in projector view, the injective X-map.  no_wrap: the reference's int16 wrap-around in
// disp = xp - xr - x_offset (xmd:27) never triggers on this rig: then disp >= 0 <=> xp - x_offset >= xr, which is what makes "dead"
// X-map cells recognisable.  k2_pipe_nlds: the pipelined K2 keeps the per-disparity table in LDS: every disparity an event of
// this rig can have, at most nlds_max entries (2048 = 16 KB: with the patch and the staging rows a block then stays under 27 KB
// of LDS, six blocks per CU; a larger disparity -- the reference's ESL calibration allows 3808 through LUT entries far outside
// the frame, no rendered frame comes near -- reads the global table)
struct RigClass {
  long max_disp;  // the projector's largest x, never taken below 0, against the LUT's smallest
  bool key32_ok, no_wrap;
  int k2_pipe_nlds;
};
inline RigClass classify_tables(const TableExtrema& e, int x_offset, bool projector, int rect_h, int nlds_max) {
  RigClass c;
  c.max_disp = std::max<long>((long)std::max(e.xp_max, 0) - e.xr_min - x_offset, (long)0 - e.xr_min - x_offset);
  c.key32_ok = (!projector || (rect_h & 3) == 0) && c.max_disp < (1l << KEY32_DISP_BITS);
  c.k2_pipe_nlds = (int)std::max<long>(1, std::min<long>(std::min<long>(c.max_disp + 1, 65536), nlds_max));
  c.no_wrap = (long)e.xp_max - e.xr_min - x_offset <= 32767 && (long)e.xp_min - e.xr_max - x_offset >= -32768;
  return c;
}

// K1 LDS windows (w_ts X-map columns, w_x camera columns) within the LDS budget, and the widest column tile.  k1_wx: the LUT
// band's width to start from ("XM_K1_WX", 16).  Reads dims, cols.ok and cols.own_mode; xm_create copies the result into the plan.
struct K1Windows {
  int w_ts = 0, w_x = 0;
  size_t lds = 0;
  bool k1_direct = false;  // tables too tall for LDS: every event takes the direct path
  int cols_w_max = 0;
  bool cols_ok = false;    // what is left of cols.ok
};
inline K1Windows size_k1_windows(const RigPlan& p, int k1_wx) {
  K1Windows r;
  const int xmap_h = p.dims.xmap_h, cam_h = p.dims.cam_h;
  // C-1M needs 44 KB (w_ts = 5, w_x = 16): three blocks per CU beside K2's 12 KB blocks
  const size_t budget = 76 * 1024;
  int w_ts = 5, w_x = k1_wx;  // 5 time columns, 16 camera columns: 70 KB at C-1M
  auto need = [&](int wt, int wx) {  // the pieces k_scatter_tiled carves (xmaps_geometry.hpp), summed
    const int head_q = tiled_head_q(tiled_win_q(p.dims.projector, wt, wx, cam_h, xmap_h), band_lut_q(wx, cam_h));
    return 16 * ((size_t)head_q + (size_t)band_xm_q(wt, xmap_h) + (size_t)tiled_dump_q());
  };
  while (need(w_ts, w_x) > budget && (w_ts > 1 || w_x > 1)) {
    if (w_ts * xmap_h * 6 >= w_x * cam_h * 4 && w_ts > 1) w_ts -= 1;
    else if (w_x > 1) w_x /= 2;
    else w_ts -= 1;
  }
  r.k1_direct = p.modes.k1_direct;
  if (need(w_ts, w_x) <= budget && w_ts >= 1 && w_x >= 1) {
    r.w_ts = w_ts;
    r.w_x = w_x;
    r.lds = need(w_ts, w_x);
  } else {
    r.k1_direct = true;
  }
  // column tiles: the widest tile whose bands + slots fit the same budget (the LUT band is the tiled kernel's)
  r.cols_ok = p.cols.ok;
  if (r.cols_ok && !r.k1_direct && r.w_x > 0) {
    int wm = 0;
    while (wm < 16 && cols_lds_bytes_at(r.w_x, cam_h, xmap_h, wm + 1) <= budget) wm += 1;
    r.cols_w_max = wm;
  }
  if (r.cols_w_max < 1 && !p.cols.own_mode) r.cols_ok = false;
  return r;
}

}  // namespace xm
