// xmaps_geometry.hpp -- the numbers the kernels and the host's plan both read, defined once: block shapes, events per thread,
// key-frame fields, flags, and the dynamic-LDS layout of every kernel whose LDS the host sizes.  Standard C++ only (no HIP
// types): the device headers include it, and so do host/xm_plan.hpp, host/xm_k2_live.hpp and host/xm_own_plan.hpp and, through
// them, the stand-alone CPU programs under tests/c_host.  A kernel carves its LDS pointers from the *_q / *_words / *_hw
// functions below and the host's *_lds_bytes (host/xm_plan.hpp) are sums of the very same functions, so a layout has one text.
// Compile knobs only a kernel reads (XM_OWN_WAVES, XM_COLS_WAVES_PER_EU, XM_K1_WAVES_PER_EU, ...) stay in that kernel's header.
#pragma once

#if defined(__HIPCC__)
#define XM_HD __host__ __device__
#else
#define XM_HD
#endif

namespace xm {

// ---- block shapes and events per thread --------------------------------------------------------------------------------------
constexpr int BLOCK = 256;  // threads of every one-item-per-thread kernel (K0, direct K1, boundary pass, untiled frame kernels)

#ifndef XM_K0_UN
#define XM_K0_UN 8
#endif
constexpr int K0_UN = XM_K0_UN;  // K0: 16-byte loads of t in flight per thread (vector path)

#ifndef XM_TILE_THREADS
#define XM_TILE_THREADS 512
#endif
constexpr int TILE_THREADS = XM_TILE_THREADS;  // tiled K1: 512 x 8 or 1024 x 4 events: same LDS tile, different latency/issue trade
#ifdef XM_TILE_EPT  // experiments: events per thread decoupled from the block size (smaller tiles)
constexpr int TILE_EPT = XM_TILE_EPT;
#else
constexpr int TILE_EPT = 4096 / XM_TILE_THREADS;
#endif
constexpr int TILE_EVENTS = TILE_THREADS * TILE_EPT;  // largest block: 4096 events (the LDS slots hold (local idx + 1) << 16)

constexpr int COLS_EPT = 8;  // column / owner tiles: events per thread and pass
#ifndef XM_COLS_MAX_THREADS
#define XM_COLS_MAX_THREADS 512
#endif
constexpr int COLS_MAX_THREADS = XM_COLS_MAX_THREADS;  // ... their largest block
// flags of the column / owner tile kernels (what each means: scatter_cols_body, xmaps_k1cols.hpp)
enum { COLS_F_DEVICE_REDO = 1, COLS_F_ALL_IN_FRAME = 2, COLS_F_EXT_EXTREMA = 4 };
// boundary pass (k_cols_bounds): boundaries a block of 256 threads finds at G lanes per boundary
XM_HD constexpr int cols_bounds_per_block(int G) { return 256 / G; }

constexpr int OWN_BW = 4;  // owner tiles: tile widths are multiples of it (K0b finds two boundaries per tile: its first column and the end of its halo)

#ifndef XM_K2_TILE_MAX
#define XM_K2_TILE_MAX 10240
#endif
#ifndef XM_K2_TX
#define XM_K2_TX 16
#define XM_K2_TY 16
#endif
// K2: a block is K2_TX x K2_TY threads, its tile K2_TX * PPT x K2_TY pixels (PPT pixels per thread: template parameter of the K2
// kernels); a patch holds at most K2_TILE_MAX cells = 20 KB of u16 (the rig's largest patch sizes the dynamic LDS: 10.5 KB at C-1M)
constexpr int K2_TX = XM_K2_TX, K2_TY = XM_K2_TY, K2_TILE_MAX = XM_K2_TILE_MAX;
// pipelined K2: 16-byte patch loads per thread kept in registers: thread slot s = tid + j * K2_TX * K2_TY holds quad s of the patch
// in memory order, so a patch of q quads needs ceil(q / 256) of them: four cover 8192 cells
constexpr int K2P_UN = 4;
constexpr int K2P_DLUT_ENTRY_BYTES = 8;  // ... an entry of its per-disparity table in LDS: {f32 depth bits, BGR word}

constexpr int CAM32_T = 32;  // camera view on the compact key frame: blocks of CAM32_T x CAM32_T pixels
// the compact (32-bit) key frame's fields (key32_tag, xmaps_common.hpp) and the largest frame its camera-view form orders exactly
constexpr unsigned KEY32_DISP_BITS = 12, KEY32_TILE_BITS = 16, CAM32_MAX_EVENTS = (1u << 20) - 1u;

// MC3D baseline (xmaps_mc3d.hpp): a wave takes MC3D_FW camera pixels of a row, a block MC3D_FR rows; MC3D_N_CNT counts per block
constexpr int MC3D_FW = 64, MC3D_FR = BLOCK / 64, MC3D_N_CNT = 7;
#ifndef XM_MC3D_GL
#define XM_MC3D_GL 16
#endif
constexpr unsigned MC3D_GL = XM_MC3D_GL;  // ... lanes of a wave that share one pixel's window (a power of two, 2 .. 64)
static_assert(MC3D_GL >= 2 && MC3D_GL <= 64 && (MC3D_GL & (MC3D_GL - 1)) == 0, "XM_MC3D_GL");
#ifndef XM_MC3D_UN
#define XM_MC3D_UN 16
#endif
constexpr unsigned MC3D_UN = XM_MC3D_UN;  // ... window entries a lane has in flight per trip
// ... its int32 maps: MC3D_POISON marks a NaN / +-inf entry, finite entries saturate at +-MC3D_SAT (== XM_MC3D_POISON, xmaps.h)
constexpr int MC3D_POISON = -2147483647 - 1, MC3D_SAT = 1 << 30;
constexpr unsigned MC3D_NO_BLUR = 1;  // == XM_MC3D_NO_BLUR

// ESL filters (xmaps_eslfilter.hpp).  Bilateral filter: a block takes ESLF_BW x ESLF_BH pixels with a halo of ESLF_HALO (d <= 5);
// ESLF_BINS colour-table bins (+ 2 entries); extrema: ESLF_RED_CHUNK pixels per block.  TV denoiser: a surface's flat vector is cut
// into tiles of ESLF_TILE pixels -- the unit of every partial sum, so it fixes the summation order: results move with it.
constexpr int ESLF_BW = 32, ESLF_BH = BLOCK / ESLF_BW, ESLF_HALO = 2, ESLF_MAX_TAPS = 25, ESLF_BINS = 4096;
constexpr int ESLF_RED_CHUNK = BLOCK * 8, ESLF_TILE = BLOCK * 4;
constexpr unsigned ESLF_NO_BILATERAL = 1, ESLF_NO_TV = 2;  // == XM_ESL_FILTER_*
// Evaluation table (xmaps_evaltable.hpp).  The streams are cut into flat tiles of EVT_TILE pixels: a thread takes EVT_UN quads of
// four consecutive pixels (16-byte loads where the maps allow them).  The tile is the unit of every partial sum, so it fixes the
// summation order: the last bits of a margin or an RMSE move with it.  Median: a block takes EVT_MW x EVT_MH pixels.
constexpr int EVT_UN = 4, EVT_TILE = BLOCK * 4 * EVT_UN;
constexpr int EVT_MW = 32, EVT_MH = BLOCK / EVT_MW;
constexpr int EVT_MAX_METHODS = 8, EVT_MAX_ROWS = 2 * EVT_MAX_METHODS, EVT_MAX_STACKS = 1 + EVT_MAX_METHODS;  // every method may add a "1 sec" row
// ... its search key: 1 + (min(cost, max_row_diff + 1) << pos_bits | position in a window of `span` entries), 0 = poison, in 32 bits
XM_HD constexpr unsigned mc3d_pos_bits(unsigned span) {
  unsigned b = 0;
  while (b < 32 && (1ull << b) < span) ++b;
  return b;
}
XM_HD constexpr bool mc3d_key_fits(unsigned max_row_diff, unsigned span) {  // (the largest key is (max_row_diff + 2) << pos_bits)
  return (((unsigned long long)max_row_diff + 2ull) << mc3d_pos_bits(span)) < (1ull << 32);
}

// ---- dynamic LDS layouts: every piece one function of plain ints ---------------------------------------------------------------
// Units: _q = 16-byte quads, _words = 4 bytes, _hw = 2 bytes.  Plain int arithmetic, as the kernels do it: a table's height
// fits int16 indices and a window is at most 64 columns wide, so no product comes near 2^31; the host sums the pieces in size_t.
// LDS-direct band loads write whole waves (64 lanes x 16 B): a band keeps one wave of quads behind it for its last, partial wave
constexpr int LDS_WAVE_SLACK_Q = 64;

// The two bands of the tiled K1 and of the column tiles: w_x camera columns of the LUT (u32 per pixel), w time columns of the
// X-map (int16 per cell), each copied with its global misalignment: one quad of slack in front, the wave of slack behind
XM_HD constexpr int band_lut_q(int w_x, int cam_h) { return ((w_x * cam_h + 3) >> 2) + 1 + LDS_WAVE_SLACK_Q; }
XM_HD constexpr int band_xm_q(int w, int xmap_h) { return ((w * xmap_h + 7) >> 3) + 1 + LDS_WAVE_SLACK_Q; }

// k_scatter_cols*:  LUT band (w_x) | X-map band (W) | winner slots, one u32 per (time column, row) of the tile
XM_HD constexpr int cols_slot_q(int W, int xmap_h) { return (W * xmap_h + 3) >> 2; }

// k_scatter_tiled*:  max(winner slots, LUT band) | X-map band (w_ts) | dump area.  Slots and LUT band share a region (the band is
// only read by the first gather, the slots only written after it); a slot per (time column, row) of the window in projector
// view, per pixel of the LUT window in camera view.  Waves entirely past the end of a band dump their load behind the X-map band
XM_HD constexpr int tiled_win_words(bool projector, int w_ts, int w_x, int cam_h, int xmap_h) { return projector ? w_ts * xmap_h : w_x * cam_h; }
XM_HD constexpr int tiled_win_q(bool projector, int w_ts, int w_x, int cam_h, int xmap_h) { return (tiled_win_words(projector, w_ts, w_x, cam_h, xmap_h) + 3) >> 2; }
XM_HD constexpr int tiled_head_q(int win_q, int lut_q) { return win_q > lut_q ? win_q : lut_q; }
XM_HD constexpr int tiled_dump_q() { return 1 + LDS_WAVE_SLACK_Q; }

// k_scatter_own*:  band slots [nxs_max][rp] | extra slots [extra_max] | the tile's band table (own_bm, own_setup): a u32 per row
// -- or, with ownership per 8-row group, two per group --, padded to 16 bytes
XM_HD constexpr int own_band_words(int nxs_max, int rp) { return nxs_max * rp; }
XM_HD constexpr int own_extra_words(int extra_max) { return extra_max; }
XM_HD constexpr int own_tab_words(int hrp, bool grouped) { return ((grouped ? (hrp >> 3) * 2 : hrp) + 3) & ~3; }

// k_frame_proj_tiled*:  the tile's patch of u16 disparities (tile_cap cells; the row maxima replace it in place) and the overrun
// of its last 16-byte reads.  k_frame_proj_pipe:  the same patch | from the next 16-byte boundary, n_lds entries of the
// per-disparity table
XM_HD constexpr int k2_patch_hw(int tile_cap) { return tile_cap + 32; }
XM_HD constexpr int k2p_dlut_off_hw(int tile_cap) { return (k2_patch_hw(tile_cap) + 7) & ~7; }

}  // namespace xm
