// xmaps_common.hpp -- what every device header of the X-maps hot path shares: the device ABI (DevTables, SlotState, FrameDesc, the
// packed-key layouts), the order-preserving time codecs, the time normalisation (x_maps_disparity.py:16-19), the per-event
// arithmetic of K1 (event_disparity*, event_cell: cam_proj_calibration.py:277-281 / 299-303, x_maps_disparity.py:23-29), the XCD
// work orders, the wave reductions, and the XM_ABLATE experiment globals.  (gfx950 / MI355X)
//
// Needs xmaps_geometry.hpp only (standard C++: what the kernels share with the host's plan); every other xmaps_*.hpp includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "xmaps_geometry.hpp"  // BLOCK, the KEY32 fields, every constant and LDS layout the host's plan reads too

namespace xm {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int KEY_IDX_SHIFT = 16;
constexpr int KEY_TAG_SHIFT = 44;
constexpr u32 KEY_MAX_TAG = (1u << 19) - 1;
constexpr int MM_SLOTS = 32;   // spread the min/max atomics over 32 addresses: one contended word retires only
                               // ~88 atomics/us on this chip (8 slots measured +3 us on K0)
constexpr int CNT_SLOTS = 64;  // same for the counters

enum { CNT_USED = 0, CNT_INLIER = 1, CNT_OOB = 2, CNT_UNSORTED = 3, CNT_STRIDE = 4 };

// HBM layouts (built once in xm_create).  The scan axis is the SLOW axis of every table an event touches:
// events arrive time-sorted and the projector scans x-slow, so the events of one thread block sit in a band of
// a few camera columns / a few X-map time columns / a few frame columns.  Column-major tables make that band a
// handful of contiguous runs -> coalesced tile loads into LDS and coalesced flushes out of it.
struct DevTables {
  const u32* lut;       // [cam_w][cam_h]   TRANSPOSED  (u16(yr) << 16) | u16(xr)
  const int16_t* xmap;  // [xmap_w][xmap_h] TRANSPOSED  X-map, time column major
  const u32* pmap;      // [proj_h][proj_w] row-major   (u16(my) << 16) | u16(mx)
  const uint2* dlut;    // [65536] per integer disparity: {f32 bits of depth, BGR word} = disparity_pixel(d) (A5-A7)
  const int4* k2_tiles; // [tiles_y][tiles_x] {bx, by, cols, rows_p} of every K2 tile's key-frame patch (cols = 0: none of
                        //   its pixels maps into the frame; cols < 0: patch too large for LDS -> generic path), precomputed
  const u32* k2_pix;    // [proj_h][proj_w] offset of the pixel's 7-tap column run inside its tile's LDS patch, ~0u = the
                        //   pixel maps outside the frame (BORDER_CONSTANT 0)
  const int4* k2_tiles1;  // the same two tables for K2's one-pixel-per-thread geometry (16 x 16 tiles: lone frames, whose
  const u32* k2_pix1;     //   launch is too small to fill the chip with 32 x 16 tiles; see frame_proj_tiled_body)
  int cam_w, cam_h, proj_w, proj_h, rect_w, rect_h, xmap_w, xmap_h;
  int x_offset, t_px_scale;
  double p03;
  float z_near, z_far;
  // owner tiles (xmaps_k1own.hpp; rigs whose (row, time column) -> cell map is not injective): the X-map once more with the
  // distance to the cell's owner column in the top bits; per tile {columns of its cell band, first extra, extras}; per (tile,
  // row) the band's first frame column and the mask of the band cells the tile owns (one u32); cells outside the
  // band ("extras") have a slot index in xmap_extra (at their owner pair) and their frame cell in own_extra_cells.  The rows
  // the rectify LUT can reach: own_hr rows from own_r_lo (a multiple of 8) on, padded to own_hrp (a multiple of 8)
  const uint16_t* xmap_own;     // [xmap_w][xmap_h]  xp | delta << 13, 0 = undefined
  const uint16_t* xmap_extra;   // [xmap_w][xmap_h]  extra slot + 1 at the owner pair of a cell outside its tile's band, else 0
  const int4* own_tiles;        // [tiles] {band columns, first extra, extras, 0}
  const u32* own_bm;            // [tiles][own_tab_words]  the tile's band table (own_setup): band positions and ownership per row / per 8-row group
  const u32* own_extra_cells;   // [extras] cell index in the (sheared) u16 frame
  int own_r_lo, own_hr, own_hrp, own_nxs_max, own_extra_max;
  int own_grouped;  // 1: a tile owns whole 8-row pieces of a frame column (own_plan), 0: any cells of a row
  int own_rp;  // rows per pass of a tile's LDS slots (a multiple of 8; own_hrp = one pass): see scatter_own_body
  // the plain u16 disparity frame of the column / owner tiles is sheared by whole columns per 8-row group: cell (x, row) lives
  // in frame column x + shear_bias + ((row >> 3) * shear_m >> 12); the frame has rect_w + shear_extra columns.  All 0 unless
  // the rig's X-map is slanted (xm_create fits shear_m)
  int shear_m, shear_bias, shear_extra;
};

__host__ __device__ inline size_t frame16_cells(const DevTables& tb) { return (size_t)(tb.rect_w + tb.shear_extra) * (size_t)tb.rect_h; }
// column of cell (x, row) in the u16 frame
__host__ __device__ inline int frame16_col(const DevTables& tb, int x, int row) { return x + tb.shear_bias + (((row >> 3) * tb.shear_m) >> 12); }

// Per-slot device state.  tag_a is written by K0 (block 0) and read by K1/K2; tag_b is written by K1
// (block 0) and read by K0 -- so no kernel reads a word that one of its own blocks is writing.
struct SlotState {
  u32 tag_a;
  u32 tag_b;
  u32 pad[2];
  u64 mm[2][MM_SLOTS][2];               // [parity][slot]{min, max} in order-preserving u64 encoding
  u32 cnt[2][CNT_SLOTS][CNT_STRIDE];    // [parity][slot]{used, inliers, index errors, events outside [t[0], t[n-1]]}
  u32 unsorted_sticky;                  // time-sorted mode: frames whose declaration did not hold (read by xm_sync)
  u32 pad2;
  // XM_FLAG_TRY_SORTED: two words of pinned host memory the kernels report to without a host round trip --
  // [0] = tag of the last frame whose (t[0], t[n-1]) shortcut did NOT hold (written by K1), [1] = tag of the last frame whose
  // K2 has started, i.e. whose K1 verdict is final.  NULL when the mode is off.
  u32* host_flags;
};
static_assert(sizeof(SlotState) % 16 == 0, "SlotState array stride");

// One frame of a MULTI-FRAME launch (grid = frames x tiles), in device memory.  Written by the host (xm_process_batch, the
// hipGraph batch) or by the ingest kernels (device-side frame segmentation: the frame's event range never visits the
// host).  valid == 0: every kernel of the frame exits at once (no frame was cut).  n == 0 with valid != 0: a defined
// empty frame (tags advance, outputs are written empty).
struct FrameDesc {
  const uint16_t* x;
  const uint16_t* y;
  const void* t;
  const int16_t* p;
  const uint4* aos;
  u64 n;
  u64* key_frame;
  SlotState* st;
  float* depth;
  uint8_t* bgr;
  u32 valid;
  u32 pad;
};
static_assert(sizeof(FrameDesc) == 88, "FrameDesc layout");

// Conditional frames of a captured batch (hipGraph): no host is at hand there to redo a frame whose column-tile attempt
// failed (xmaps_k1cols.hpp), so the graph carries BOTH paths and the kernels decide per frame on the device.  A failing
// tile leaves the frame's tag in SlotState.pad[1]; COND = 1 kernels run a frame only if its attempt failed, COND = 2 only
// if it held, COND = 0 always.  (tag_a holds the frame's tag from the attempt's K1 on, and K0 of the redo recomputes the
// very same value from tag_b, which only a K2 advances.)
__device__ inline bool frame_attempt_failed(const SlotState* st) { return st->pad[1] == st->tag_a; }
template <int COND> __device__ inline bool frame_skipped(const SlotState* st) {
  if constexpr (COND == 0) return false;
  else return frame_attempt_failed(st) != (COND == 1);
}

// device -> pinned host memory, visible to the host when the kernel has finished
__device__ inline void host_flag_store(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// ---- order-preserving u64 encodings so that one pair of unsigned atomics serves every t dtype ------
template <typename T> struct TimeCodec;
template <> struct TimeCodec<long long> {
  static __host__ __device__ u64 enc(long long v) { return (u64)v ^ 0x8000000000000000ull; }
  static __host__ __device__ long long dec(u64 u) { return (long long)(u ^ 0x8000000000000000ull); }
};
template <> struct TimeCodec<double> {
  static __host__ __device__ u64 enc(double v) {
    u64 b;
    __builtin_memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  }
  static __host__ __device__ double dec(u64 u) {
    u64 b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
  }
};
template <> struct TimeCodec<float> {  // f32 -> f64 is exact and monotone
  static __host__ __device__ u64 enc(float v) { return TimeCodec<double>::enc((double)v); }
  static __host__ __device__ float dec(u64 u) { return (float)TimeCodec<double>::dec(u); }
};

// Dirty-line flags of the projector-view key frame: one byte per 128-byte line (16 cells).  K1 stores the frame's tag
// byte for every line it writes a key into; K2 only fetches lines whose flag carries the current tag byte (at C-1M only
// 46 % of the lines are dirty, so K2 skips half of its 34 MB read).  Plain idempotent stores, no clearing: a stale flag
// (tags repeat every 255 frames) is only a false positive -- the line is fetched and its keys' full tags decide.
__host__ __device__ inline unsigned char dirty_byte(u32 tag) { return (unsigned char)(tag % 255u + 1u); }

// ---- compact (32-bit) key frame of the verified-sorted projector-view path ------------------------------------------------
//   tag4:4 | tile:16 | disparity:12        (tag4 = tag % 15 + 1; 0 = cleared cell)
// Half the bytes per cell means twice as many winners per 64-byte L2 atomic request and half of K2's key-frame read: K1
// at full occupancy is bound by the chip's L2 atomic rate (~23 G requests/s measured: profiles/r02*_pmc.md), K2 by the
// read.  The order field is the TILE index, not the event index: inside a tile the last writer is resolved exactly in LDS
// (slot value = local index | disparity), across tiles a higher tile = later events.  That is exact as long as EVERY
// event of the tile goes through the LDS slots: an event whose time column falls outside the tile's LDS window cannot, so it
// marks the frame as failed -- the same flag, and the same automatic redo on the 64-bit general path, as an event outside
// [t[0], t[n-1]].  Events outside the LUT window only (x noise) fetch their LUT entry from global memory and then use
// the slots like everybody else.  Preconditions checked by the host (xm_create): projector view, rect_h % 4 == 0, every
// possible disparity < 4096, tiles per frame < 65536; the 4-bit tag is kept unambiguous by clearing the frame at least
// every 15 frames of the slot (9.3 MB memset per 15 frames at C-1M).
// Camera view (VIEW == 1 with KEY32): the cell is the event's own pixel, written by events of ANY tile, so the order field is the
// event itself: key = (event index + 1) << 12 | disparity -- exact for every frame of < 2^20 events whatever their order, strays
// included; no tag: the frame kernel, which reads every pixel of the 1.2 MB frame exactly once, zeroes what it has read.
// (KEY32_DISP_BITS, KEY32_TILE_BITS, CAM32_MAX_EVENTS: xmaps_geometry.hpp)
__host__ __device__ inline u32 key32_tag(u32 tag) { return (tag % 15u + 1u) << 28; }
__device__ inline uint16_t key_disp32(u32 k, u32 tag4) { return (k & 0xf0000000u) == tag4 ? (uint16_t)(k & 0xfffu) : (uint16_t)0; }

constexpr u64 MM_INIT_MIN = ~0ull;
constexpr u64 MM_INIT_MAX = 0ull;

// ---- t -> X-map column, bit-exact with NumPy (x_maps_disparity.py:16-19) ---------------------------
// int64: (t - tmin) and (tmax - tmin) are exact int64, both converted to f64, IEEE divide, multiply by
// S, round-half-even.  Compiled with -ffp-contract=off so nothing is fused.
template <typename T> struct TimeNorm;
template <> struct TimeNorm<long long> {
  long long tmin;
  double den, scale, rs;
  bool degenerate, fast_frame;
  __device__ TimeNorm(long long lo, long long hi, int S)
      : tmin(lo), den((double)(hi - lo)), scale((double)S), degenerate(hi == lo) {
    // a frame spans microseconds: (hi - lo) < 2^32 always holds in practice; everything else takes the exact path
    fast_frame = (u64)(hi - lo) <= 0xffffffffull && !degenerate;
    rs = (1.0 / den) * scale;
  }
  // Reference: rint(fl(fl(a / den) * S)), a = t - tmin.  Fast value: e = fl(a * fl(fl(1/den) * S)) differs from the
  // reference's product by < 4 ulp (< 2e-12 for columns <= 32767); whenever e is further than 1e-6 from a rounding
  // boundary (x.5) both round to the same integer, so rint(e) IS the reference result.  Closer than that (exact ties such
  // as golden g1d_rint_ties land here) the IEEE divide of column_exact decides.
  // Branch-free and built from full-rate FP64 adds only (K1 as a single launch is bound by this dependent chain; the
  // conversions and v_rndne_f64 are quarter rate): u32 -> double and double -> nearest-even integer both go through the
  // 2^52 trick -- bits(2^52) | a IS 2^52 + a, and the low word of fl(e + 2^52) IS rint(e) for 0 <= e < 2^32.
  // `ok` = the value may be used; callers OR the failures of a batch together and take ONE rare branch.
  __device__ int column_fast(long long t, bool& ok) const {
    constexpr double M = 4503599627370496.0;  // 2^52
    const u64 a = (u64)(t - tmin);
    const double ad = __hiloint2double(0x43300000, (int)(u32)a) - M;  // (double)(u32)a, exact
    const double e = ad * rs;
    const double m = e + M;  // low word = rint(e), ties to even
    const double d = e - (m - M);  // e - rint(e), exact (Sterbenz)
    ok = ((u32)(a >> 32) == 0u) & (fabs(d) < 0.5 - 1e-6);
    return (int)(short)__double2loint(m);
  }
  __device__ int column_exact(long long t) const {
    if (degenerate) return 0;  // 0/0 = NaN -> int16 cast = 0 (what NumPy yields on x86-64)
    const double tn = (double)(t - tmin) / den;
    return (int)(short)(int)rint(tn * scale);
  }
  __device__ int column(long long t) const {
    bool ok;
    const int c = column_fast(t, ok);
    return __builtin_expect(ok && fast_frame, 1) ? c : column_exact(t);
  }
  // N columns at once: straight-line fast values (N independent chains for the scheduler to interleave), one rare branch
  template <int N> __device__ void columns(const long long (&t)[N], int (&col)[N]) const {
    u32 redo = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      bool ok;
      col[k] = column_fast(t[k], ok);
      redo |= ok ? 0u : (1u << k);
    }
    if (!fast_frame) redo = (1u << N) - 1;
    if (__builtin_expect(redo != 0, 0)) {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if ((redo >> k) & 1) col[k] = column_exact(t[k]);
    }
  }
};
template <> struct TimeNorm<double> {
  double tmin, den, scale;
  bool degenerate;
  __device__ TimeNorm(double lo, double hi, int S) : tmin(lo), den(hi - lo), scale((double)S), degenerate(hi == lo) {}
  __device__ int column(double t) const {
    if (degenerate) return 0;
    double tn = (t - tmin) / den;
    return (int)(short)(int)rint(tn * scale);
  }
  template <int N> __device__ void columns(const double (&t)[N], int (&col)[N]) const {
#pragma unroll
    for (int k = 0; k < N; ++k) col[k] = column(t[k]);
  }
};
template <> struct TimeNorm<float> {  // eval caller with an f32 time surface: NumPy stays in f32
  float tmin, den, scale;
  bool degenerate;
  __device__ TimeNorm(float lo, float hi, int S) : tmin(lo), den(hi - lo), scale((float)S), degenerate(hi == lo) {}
  __device__ int column(float t) const {
    if (degenerate) return 0;
    float tn = (t - tmin) / den;
    return (int)(short)(int)rintf(tn * scale);
  }
  template <int N> __device__ void columns(const float (&t)[N], int (&col)[N]) const {
#pragma unroll
    for (int k = 0; k < N; ++k) col[k] = column(t[k]);
  }
};

// blockIdx -> work item such that the blocks that land on one XCD (blockIdx % 8 under round-robin dispatch) own a
// contiguous range of items.  Bijective for any grid size.
constexpr u32 N_XCD = 8;
__device__ inline u32 xcd_contiguous(u32 b, u32 nb) {
  const u32 xcd = b % N_XCD, j = b / N_XCD, q = nb / N_XCD, r = nb % N_XCD;
  return xcd * q + (xcd < r ? xcd : r) + j;
}

// The same for frame `frame` of a (nb, frames) grid: workgroups are dealt to the XCDs in LINEAR order, so the frame's block b sits on
// XCD (frame * nb + b) % 8 -- with nb % 8 != 0 every frame starts on another XCD, and xcd_contiguous(b, nb) would hand every XCD
// every table slice over the frames of a group.  XCD x takes the x-th contiguous run of the frame's items, whatever the phase
// (the runs' lengths move by one item between frames).  Bijective.
__device__ inline u32 xcd_contiguous_in_frame(u32 b, u32 nb, u32 frame) {
  const u32 s = (frame * nb) % N_XCD, bv = b + s, xcd = bv % N_XCD, end = nb + s;  // the frame's blocks: virtual indices [s, end)
  u32 start = 0;
  for (u32 x = 0; x < xcd; ++x) {
    const u32 first = s + ((x + N_XCD - s) % N_XCD);
    start += first < end ? (end - 1 - first) / N_XCD + 1 : 0;
  }
  const u32 first = s + ((xcd + N_XCD - s) % N_XCD);
  return start + (bv - first) / N_XCD;
}

// ---- wave helpers (wave = 64 lanes) ------------------------------------------------------------------
__device__ inline u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    u64 w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ inline u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ inline double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ inline double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ inline u32 wave_sum_u32(u32 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline u32 wave_max_u32(u32 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u32 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// frame extrema as written by K0: every wave reduces the MM_SLOTS partials itself (128 B, L2-hot) and broadcasts
// the result through SGPRs (readfirstlane), so everything derived from it is wave-uniform
__device__ inline u64 uniform_u64(u64 v) {
  const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
  return ((u64)hi << 32) | lo;
}
__device__ inline void load_frame_minmax(const SlotState* st, u32 parity, u64& lo, u64& hi) {
  const int lane = threadIdx.x & 63;
  u64 a = MM_INIT_MIN, b = MM_INIT_MAX;
  if (lane < MM_SLOTS) {
    a = st->mm[parity][lane][0];
    b = st->mm[parity][lane][1];
  }
#pragma unroll
  for (int o = MM_SLOTS / 2; o > 0; o >>= 1) {
    const u64 a2 = __shfl_xor(a, o, 64), b2 = __shfl_xor(b, o, 64);
    a = a2 < a ? a2 : a;
    b = b2 > b ? b2 : b;
  }
  lo = uniform_u64(a);
  hi = uniform_u64(b);
}

// ---- slot bookkeeping every K1 does.  The pointer types are template parameters: the column and owner tiles pass pointers that
//      carry the global address space in their type (xmaps_k1cols.hpp), and a generic parameter here would make their stores flat.
// Block 0 re-arms the OTHER parity's min/max slots for the next frame on this slot; the calling threads take the slots
// first, first + step, ...
template <typename State>
__device__ __forceinline__ void rearm_minmax(State st, u32 parity, int first, int step) {
  for (int i = first; i < MM_SLOTS; i += step) {
    st->mm[parity ^ 1][i][0] = MM_INIT_MIN;
    st->mm[parity ^ 1][i][1] = MM_INIT_MAX;
  }
}

// Block end (one thread): the block's inlier and index-error counts into the frame's counters, spread over CNT_SLOTS addresses.
// The counts are LDS words: taken by reference, each is read where it is used (by value both are read up front, which moved
// the tail of every K1); the site hands in the row itself, c = st->cnt[parity][blk % CNT_SLOTS], so that its address is formed
// where it was.
template <typename Counters>
__device__ __forceinline__ void flush_counts(Counters c, const u32& n_in, const u32& n_oob) {
  if (n_in) __hip_atomic_fetch_add(&c[CNT_INLIER], n_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (n_oob) __hip_atomic_fetch_add(&c[CNT_OOB], n_oob, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sharded frames: the FRAME's extrema from the 16-byte device buffer the ranks MIN-all-reduce -- {tmin, -tmax}, int64 for int64 t,
// f64 for float t (k_minmax_export) -- as the encoded lo / hi.  Uniform loads.
template <typename T>
__device__ __forceinline__ ulonglong2 ext_minmax(const void* __restrict__ mm_ext) {
  if constexpr (std::is_same<T, long long>::value) {
    const long long* m = static_cast<const long long*>(mm_ext);
    return make_ulonglong2(TimeCodec<T>::enc(m[0]), TimeCodec<T>::enc(-m[1]));
  } else {
    const double* m = static_cast<const double*>(mm_ext);
    return make_ulonglong2(TimeCodec<T>::enc((T)m[0]), TimeCodec<T>::enc((T)(-m[1])));
  }
}

// ---- EventCD records (AoS input): {x | y << 16, p, t low word, t high word} ----------------------------------------------
// (three sites keep the decode spelled out because their kernels' assembly moved with the call: k_cols_bounds' probe loop and
// k_pause_flags; profiles/device_split_identity.md)
template <typename T = long long>
__host__ __device__ __forceinline__ T rec_t(const uint4& r) { return (T)(long long)(((u64)r.w << 32) | r.z); }
__host__ __device__ __forceinline__ u32 rec_x(const uint4& r) { return r.x & 0xffff; }
__host__ __device__ __forceinline__ u32 rec_y(const uint4& r) { return r.x >> 16; }

// ---- the per-event arithmetic every K1 and the stage kernels share -----------------------------------------------------------
struct EventResult {
  int xr, yr, ts, disp;
  bool inlier;
};

// A1 + A2 for one event whose time column is already known.  Sets oob when NumPy would raise IndexError.
__device__ inline EventResult event_disparity_col(const DevTables& tb, int column, u32 x, u32 y, bool& oob) {
  EventResult r{0, 0, column, 0, false};
  oob = false;
  if (x >= (u32)tb.cam_w || y >= (u32)tb.cam_h) {  // map[y, x] IndexError (calib:279-280)
    oob = true;
    return r;
  }
  const u32 l = tb.lut[x * (u32)tb.cam_h + y];
  r.xr = (int)(short)(l & 0xffff);
  r.yr = (int)(short)(l >> 16);
  const bool y_ok = r.yr >= 0 && r.yr < tb.xmap_h - 1;  // xmd:23 (last X-map row excluded)
  if (!y_ok) return r;
  if ((u32)r.ts >= (u32)tb.xmap_w) {  // only reachable when a caller hands in extrema that do not bound t
    oob = true;
    return r;
  }
  const int xp = (int)tb.xmap[r.ts * tb.xmap_h + r.yr];                // xmd:25
  r.disp = (int)(short)(xp - r.xr - tb.x_offset);                      // int16 wrap-around (xmd:27)
  r.inlier = r.disp >= 0;                                              // xmd:29
  return r;
}

// A1 + A2 for one event.  `used` = belongs to the frame (polarity).
template <typename T>
__device__ inline EventResult event_disparity(const DevTables& tb, const TimeNorm<T>& tn, u32 x, u32 y, T t,
                                              bool used, bool& oob) {
  oob = false;
  if (!used) return EventResult{0, 0, 0, 0, false};
  return event_disparity_col(tb, tn.column(t), x, y, oob);
}

// cell of the disparity frame an inlier event writes; false = NumPy IndexError
template <int VIEW>
__device__ inline bool event_cell(const DevTables& tb, const EventResult& r, u32 x, u32 y, u32& cell) {
  if constexpr (VIEW == 0) {
    int col = (int)(short)(r.xr + r.disp);  // calib:300: int16 add (= xp - x_offset), rint is a no-op
    if (col < 0) col += tb.rect_w;          // NumPy negative index wraps once
    if (col < 0 || col >= tb.rect_w || r.yr >= tb.rect_h) return false;
    cell = (u32)col * (u32)tb.rect_h + (u32)r.yr;  // projector-view key frame is column-major [col][row]
  } else {
    cell = y * (u32)tb.cam_w + x;  // camera-view key frame is row-major; bounds checked by the LUT gather
  }
  return true;
}

// ---- experiment build (-DXM_ABLATE): switches and time stamps that kernels of several files use ----------------------------
#ifdef XM_ABLATE
__device__ int g_ablate = 0;  // bit0: no flush atomics, bit1: no LDS slot atomics, bit2: no band loads, bit3: no time divide
#define XM_ABL(bit) (g_ablate & (1 << (bit)))  // bit 2 (band loads) no longer wired
__device__ unsigned long long g_timeline[64][16];  // [block][phase] s_memtime stamps of thread 0 (experiments only)
#define XM_STAMP(ph) do { if ((threadIdx.x == 0) && blockIdx.x < 64) g_timeline[blockIdx.x][ph] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define XM_ABL(bit) 0
#define XM_STAMP(ph) do { } while (0)
#endif

}  // namespace xm
