// xmaps_k1tiles.hpp -- K1 on event tiles: the per-event work of xmaps_k1direct.hpp (same reference lines) for runs of up to 4096
// consecutive events, with the tables' bands and the last-writer-wins resolution in LDS.  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp only (events outside a tile's windows go through event_disparity_col / event_cell).
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// =====================================================================================================
// K1 (tiled): the same per-event work, restructured around what the chip charges for.
//
// Measured on MI355X (profiles/r01_ubench_atomics.md): a lane-divergent atomic costs ~39 ps of chip time per
// lane whatever its width/scope, a divergent load ~13 ps, but the same operations coalesced cost 6-10x less:
// the price is per (lane -> distinct cache line) request.  The direct kernel issues 3 such requests per event
// (LUT gather, X-map gather, atomic).  Here one block owns TILE_EVENTS consecutive events = one thin time slice:
//   * its LUT band  (w_x camera columns around the slice's mean x)   -> LDS, coalesced (column-major table)
//   * its X-map band (w_ts time columns around the slice's mean column) -> LDS, coalesced
//   * last-writer-wins is resolved in LDS first: one u32 slot per (time column, rectified row) -- events of
//     the same slot hit the same frame cell because cell = (yr, X[yr, ts]) -- holding max((local idx+1)<<16 | disp)
//   * winners are flushed with lanes walking consecutive rows of one time column; the key frame is
//     column-major, so a wave's atomics fall into a few cache lines instead of 64.
// Events outside the windows (unsorted / raster-ordered input, noise) take the direct global path inside
// the same kernel: always correct, only slower.  Camera view: slot = (row, x - x_lo), frame row-major.
// =====================================================================================================

// (TILE_THREADS, TILE_EPT, TILE_EVENTS: xmaps_geometry.hpp)
// VEC: SoA columns 16-byte aligned -> each thread loads TILE_EPT consecutive events with 8/16-byte loads.  A compile-time
// switch, not a per-block branch: with both load paths in one kernel the compiler's wait-count bookkeeping at the join
// put full vmcnt waits in front of the event loads and of the extrema reduction (seen in the ISA).
#ifdef XM_K1_WAVES_PER_EU  // experiments: cap the VGPRs so that this many waves fit a SIMD (HIP's 2nd launch-bounds argument)
#define XM_K1_BOUNDS __launch_bounds__(TILE_THREADS, XM_K1_WAVES_PER_EU)
#else
#define XM_K1_BOUNDS __launch_bounds__(TILE_THREADS)
#endif
// blk / nblk = this block's index among the frame's blocks / their number (blockIdx.x, gridDim.x of a single-frame launch).
// mm_ext (sharded mode, tag_override != 0): the FRAME's extrema in device memory as {tmin, -tmax} (int64 for int64 t, f64
// for float t) -- the buffer the ranks MIN-all-reduce -- read here so that no host round trip sits between the collective
// and this kernel; NULL: mm_lo / mm_hi carry the encoded extrema.
template <typename T, bool AOS, bool HAS_P, int VIEW, bool VEC, bool KEY32 = false>
__device__ __forceinline__ void scatter_tiled_body(
    const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const T* __restrict__ ts,
    const int16_t* __restrict__ ps, const uint4* __restrict__ aos, u64 n, u64 idx_offset, const DevTables& tb, SlotState* st,
    u32 tag_override, u64 mm_lo, u64 mm_hi, const void* __restrict__ mm_ext, u64* __restrict__ frame,
    unsigned char* __restrict__ dirty, int w_ts, int w_x, int sorted_mode, const u32 blk, const u32 nblk) {
  static_assert(!(AOS && VEC), "AoS records are loaded one per lane");
  constexpr bool PROJ32 = KEY32 && VIEW == 0, CAM32 = KEY32 && VIEW == 1;  // (see KEY32_DISP_BITS)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // LDS carve-up (the pieces and their sizes: xmaps_geometry.hpp).  The LUT band and the winner slots SHARE one region: the
  // band is only read by the first gather of the fast path, the slots only written after it -- two extra barriers buy 26 KB
  // per block, i.e. a third resident block per CU (block residency is what bounds the pipelined frame rate:
  // tools/block_timeline.py).
  const int win_words = tiled_win_words(VIEW == 0, w_ts, w_x, tb.cam_h, tb.xmap_h);
  const int win_q = tiled_win_q(VIEW == 0, w_ts, w_x, tb.cam_h, tb.xmap_h);
  const int lut_q = band_lut_q(w_x, tb.cam_h);
  u32* win = reinterpret_cast<u32*>(smem);
  u32* lut_base = win;
  int16_t* xm_base = reinterpret_cast<int16_t*>(win + 4 * tiled_head_q(win_q, lut_q));
  __shared__ u32 s_in, s_oob;

  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;               // 64 .. 1024, chosen per frame by the host so that the block's
  const int ev_per_block = nthreads * TILE_EPT;  // time slice fits the LDS window (see launch_scatter)
  XM_STAMP(0);
  // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Neighbouring tiles share
  // almost all of their LUT band and a column of their X-map band, so XCD k takes the k-th CONTIGUOUS eighth of the
  // frame's tiles: the bands then come out of that XCD's L2 instead of being fetched over the fabric once per block.
  const u32 tile = xcd_contiguous(blk, nblk);
  const u64 block_base = (u64)tile * ev_per_block;  // < n: the host launches ceil(n / ev_per_block) blocks, n > 0

  // ---- 1. Every load that depends on nothing is ISSUED here, small ones first, and nothing is consumed before the
  //         last one is out: vector memory returns in order, so the few bytes that locate the tile (samples, frame
  //         extrema) can be waited for with the 48 KB of events still in flight behind them.
  // 1a. three sampled events (first / middle / last of the block) locate the time slice; t[0] and t[n-1] are the frame
  //     extrema of the time-sorted mode.  Uniform loads.
  int sx[3];
  T st_t[3];
  T t_first, t_last;
  {
    const u64 last = (block_base + ev_per_block <= n ? block_base + ev_per_block : n) - 1;
    const u64 si[3] = {block_base, block_base + ((last - block_base) >> 1), last};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if constexpr (AOS) {
        const uint4 r = aos[si[j]];
        sx[j] = (int)rec_x(r);
        st_t[j] = rec_t<T>(r);
      } else {
        sx[j] = (int)xs[si[j]];
        st_t[j] = ts[si[j]];
      }
    }
    if constexpr (AOS) {
      const uint4 a = aos[0], b = aos[n - 1];
      t_first = rec_t<T>(a);
      t_last = rec_t<T>(b);
    } else {
      t_first = ts[0];
      t_last = ts[n - 1];
    }
  }
  // 1b. frame extrema as K0 left them: BOTH parities (2 x 16 B in lanes < MM_SLOTS), selected once the tag is known --
  //     loading only the right one would put a scalar load (the tag) in front of this vector load.
  //     Lanes >= MM_SLOTS load a duplicate slot, which a min/max reduction does not notice.
  const ulonglong2 mm_p0 = *reinterpret_cast<const ulonglong2*>(&st->mm[0][tid & (MM_SLOTS - 1)][0]);
  const ulonglong2 mm_p1 = *reinterpret_cast<const ulonglong2*>(&st->mm[1][tid & (MM_SLOTS - 1)][0]);
  // 1c. this thread's events, kept PACKED (two 16-bit coordinates per register) until after the window is known
  u32 xw[TILE_EPT / 2], yw[TILE_EPT / 2], pw[TILE_EPT / 2];
  T tt[TILE_EPT];
  u32 inb = 0;  // bit k: event k of this thread exists (index < n)
#pragma unroll
  for (int q = 0; q < TILE_EPT / 2; ++q) xw[q] = yw[q] = pw[q] = 0;
#pragma unroll
  for (int k = 0; k < TILE_EPT; ++k) tt[k] = (T)0;
  if constexpr (AOS) {  // EventCD records: event k*nthreads + tid, one 16-byte load each, clamped (branch-free)
    {
#pragma unroll
      for (int k = 0; k < TILE_EPT; ++k) {
        const u64 i = block_base + (u32)k * nthreads + tid;
        const bool ok = i < n;
        const uint4 r = aos[ok ? i : block_base];
        inb |= ok ? 1u << k : 0u;
        if (k & 1) {
          xw[k >> 1] |= (r.x & 0xffff) << 16;
          yw[k >> 1] |= r.x & 0xffff0000u;
          pw[k >> 1] |= r.y << 16;
        } else {
          xw[k >> 1] = r.x & 0xffff;
          yw[k >> 1] = r.x >> 16;
          pw[k >> 1] = r.y & 0xffff;
        }
        tt[k] = rec_t<T>(r);
      }
    }
  } else if constexpr (VEC) {  // TILE_EPT consecutive events per thread: 8/16-byte loads of x / y / p, 16-byte loads of t
    // Ragged end of the frame, branch-free: a thread past the end re-reads the last group (its events are masked out);
    // the thread that straddles the end loads its whole aligned group -- an aligned 8/16-byte word whose first element
    // is valid cannot cross into another page -- and a t pair that starts past the end is redirected to the first pair.
    // 32-bit element indices (n <= 2^28) and byte offsets: the loads take the scalar-base + 32-bit-offset form
    const u32 n32 = (u32)n;
    const u32 base_true = (u32)block_base + (u32)tid * TILE_EPT;
    const u32 last_grp = (n32 - 1u) & ~(u32)(TILE_EPT - 1);
    const u32 base = base_true < last_grp ? base_true : last_grp;
    const char* xs_b = reinterpret_cast<const char*>(xs);
    const char* ys_b = reinterpret_cast<const char*>(ys);
    const char* ps_b = reinterpret_cast<const char*>(ps);
    const char* ts_b = reinterpret_cast<const char*>(ts);
    if constexpr (TILE_EPT == 8) {
      const uint4 xv = *reinterpret_cast<const uint4*>(xs_b + base * 2u);
      const uint4 yv = *reinterpret_cast<const uint4*>(ys_b + base * 2u);
      xw[0] = xv.x; xw[1] = xv.y; xw[2] = xv.z; xw[3] = xv.w;
      yw[0] = yv.x; yw[1] = yv.y; yw[2] = yv.z; yw[3] = yv.w;
      if constexpr (HAS_P) {
        const uint4 pv = *reinterpret_cast<const uint4*>(ps_b + base * 2u);
        pw[0] = pv.x; pw[1] = pv.y; pw[2] = pv.z; pw[3] = pv.w;
      }
    } else {
      const uint2 xv = *reinterpret_cast<const uint2*>(xs_b + base * 2u);
      const uint2 yv = *reinterpret_cast<const uint2*>(ys_b + base * 2u);
      xw[0] = xv.x; xw[1] = xv.y;
      yw[0] = yv.x; yw[1] = yv.y;
      if constexpr (HAS_P) {
        const uint2 pv = *reinterpret_cast<const uint2*>(ps_b + base * 2u);
        pw[0] = pv.x; pw[1] = pv.y;
      }
    }
    if constexpr (sizeof(T) == 8) {
#pragma unroll
      for (int q = 0; q < TILE_EPT / 2; ++q) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(ts_b + (base + 2 * q < n32 ? base + 2 * q : base) * 8u);
        __builtin_memcpy(&tt[2 * q], &a.x, 8);
        __builtin_memcpy(&tt[2 * q + 1], &a.y, 8);
      }
    } else {
#pragma unroll
      for (int q = 0; q < TILE_EPT / 4; ++q) {
        const float4 a = *reinterpret_cast<const float4*>(ts_b + (base + 4 * q < n32 ? base + 4 * q : base) * 4u);
        __builtin_memcpy(&tt[4 * q], &a.x, 4); __builtin_memcpy(&tt[4 * q + 1], &a.y, 4);
        __builtin_memcpy(&tt[4 * q + 2], &a.z, 4); __builtin_memcpy(&tt[4 * q + 3], &a.w, 4);
      }
    }
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) inb |= base_true + k < n32 ? 1u << k : 0u;
  } else {  // any alignment / ragged tail: event k*nthreads + tid, still coalesced across lanes, clamped
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) {
      const u64 i = block_base + (u32)k * nthreads + tid;
      const bool ok = i < n;
      const u64 ic = ok ? i : block_base;
      const u32 xv = xs[ic], yv = ys[ic];
      tt[k] = ts[ic];
      inb |= ok ? 1u << k : 0u;
      xw[k >> 1] |= xv << ((k & 1) * 16);
      yw[k >> 1] |= yv << ((k & 1) * 16);
      if constexpr (HAS_P) pw[k >> 1] |= (u32)(uint16_t)ps[ic] << ((k & 1) * 16);
    }
  }
  XM_STAMP(1);

  // ---- 2. frame extrema -> time normalisation.  General mode: written by K0.  Time-sorted mode (the caller declared
  //         the frame sorted by t, true for every frame the trigger finder emits): extrema = t[0], t[n-1], K0 is not
  //         launched at all, and the declaration is VERIFIED below (every event must lie inside [t[0], t[n-1]]).
  const u32 tag = tag_override ? tag_override : (sorted_mode ? st->tag_b + 1 : st->tag_a);
  const u32 parity = tag & 1;
  u64 lo, hi;
  if (tag_override) {  // sharded mode: the FRAME's extrema come from the all-reduce of the shards' extrema
    lo = mm_lo;
    hi = mm_hi;
    if (mm_ext) {  // {tmin, -tmax} left in device memory by the collective
      const ulonglong2 e = ext_minmax<T>(mm_ext);
      lo = e.x;
      hi = e.y;
    }
  } else {
    if (sorted_mode) {
      lo = TimeCodec<T>::enc(t_first);
      hi = TimeCodec<T>::enc(t_last);
      if (hi < lo) hi = lo;  // not sorted at all: keep the arithmetic defined; the verification flags the frame
    } else {
      u64 a = parity ? mm_p1.x : mm_p0.x, b = parity ? mm_p1.y : mm_p0.y;
#pragma unroll
      for (int o = MM_SLOTS / 2; o > 0; o >>= 1) {
        const u64 a2 = __shfl_xor(a, o, 64), b2 = __shfl_xor(b, o, 64);
        a = a2 < a ? a2 : a;
        b = b2 > b ? b2 : b;
      }
      lo = uniform_u64(a);
      hi = uniform_u64(b);
    }
    if (blk == 0) {
      if (tid == 0) {
        if (sorted_mode) {
          st->tag_a = tag;  // K2 reads tag_a and copies it to tag_b
          st->mm[parity][0][0] = lo;  // for xm_frame_stats.t_min / t_max
          st->mm[parity][0][1] = hi;
        } else {
          st->tag_b = tag;
        }
      }
      rearm_minmax(st, parity, tid, nthreads);
    }
  }
  const TimeNorm<T> tn(TimeCodec<T>::dec(lo), TimeCodec<T>::dec(hi), tb.t_px_scale);
  const u64 key_hi = (u64)tag << KEY_TAG_SHIFT;
  if (tid == 0) {
    s_in = 0;
    s_oob = 0;
  }
  XM_STAMP(2);

  // ---- 3. window = median of the samples.  A wrong guess (unsorted input, a noise event) only sends events down
  //         the direct path.
  int x_lo, ts_lo;
  {
    // the column is monotone in t: the median column is the column of the median time (one conversion, not three)
    const u64 e0 = TimeCodec<T>::enc(st_t[0]), e1 = TimeCodec<T>::enc(st_t[1]), e2 = TimeCodec<T>::enc(st_t[2]);
    const u64 lo01 = e0 < e1 ? e0 : e1, hi01 = e0 < e1 ? e1 : e0;
    const u64 m2 = hi01 < e2 ? hi01 : e2;
    const u64 em = lo01 > m2 ? lo01 : m2;
    const int mc = tn.column(TimeCodec<T>::dec(em));
    const int mx = max(min(sx[0], sx[1]), min(max(sx[0], sx[1]), sx[2]));
    x_lo = min(max(mx - w_x / 2, 0), max(tb.cam_w - w_x, 0));
    ts_lo = min(max(mc - w_ts / 2, 0), max(tb.xmap_w - w_ts, 0));
  }
  XM_STAMP(3);
  // The bands are contiguous runs of the column-major tables: [x_lo, x_lo + w_x) x cam_h words and
  // [ts_lo, ts_lo + w_ts) x xmap_h int16.  Aligned 16-byte loads over ONE index space (LUT quads, then X-map quads), so a
  // full-size block issues 3 (1024 threads) or 6 (512) loads per thread, all in flight at once; the LDS copies keep the global misalignment (a
  // few elements of slack in front).  Branch-free on purpose: loads use a clamped index and out-of-range lanes store into
  // a dummy LDS slot -- any predication here turns into one basic block per load with an s_waitcnt vmcnt(0) behind it
  // (seen in the ISA), i.e. serialized L2 round trips.
  const int wx_eff = min(w_x, tb.cam_w), wts_eff = min(w_ts, tb.xmap_w);
  const u32 lut_start = (u32)x_lo * (u32)tb.cam_h, lut_shift = lut_start & 3u;  // in words
  const u32 xm_start = (u32)ts_lo * (u32)tb.xmap_h, xm_shift = xm_start & 7u;   // in int16
  const u32* lut_t = lut_base + lut_shift;
  const int16_t* xm_t = xm_base + xm_shift;
  const uint4* g_lut = reinterpret_cast<const uint4*>(tb.lut + (lut_start - lut_shift));
  const int nq_lut = (int)((lut_shift + (u32)wx_eff * (u32)tb.cam_h + 3u) >> 2);
  const uint4* g_xm = reinterpret_cast<const uint4*>(tb.xmap + (xm_start - xm_shift));
  const int nq_xm = (int)((xm_shift + (u32)wts_eff * (u32)tb.xmap_h + 7u) >> 3);
  const int nq_all = nq_lut + nq_xm;
  uint4* l_lut = reinterpret_cast<uint4*>(lut_base);
  uint4* l_xm = reinterpret_cast<uint4*>(xm_base);
  // LDS-DIRECT loads (global_load_lds_dwordx4, gfx950): the bands go L2 -> LDS without passing through VGPRs -- no 24
  // registers of band data held across the event arithmetic, no ds_write_b128, nothing to wait for until the gathers.
  // Lane l of a wave writes 16 B at M0 + 16 l, so a wave's 64 quads land contiguously: LDS quad index == band quad index,
  // as before.  Waves entirely past the end of a band skip the load (wave-uniform branch); the last, partial wave of a
  // band re-reads the band's last quad for its surplus lanes and writes it into the wave of slack behind the band.
  // A FIXED number of loads per wave is issued here (enough for the C-1M bands), so that the wait for the thread's own
  // events further down can be a counted one (vmcnt(6)) and the bands stay in flight during the time-column arithmetic;
  // taller tables / smaller blocks fetch the rest after that arithmetic (dynamic trip count = full wait, seen in the ISA).
  // The compiler waits with vmcnt(0) before the first use of a register loaded BEFORE an LDS-direct load (seen in the ISA:
  // it does not count past them), i.e. the time-column arithmetic below would wait for the bands too.  Touch the event
  // registers here instead: the wait lands in front of the band loads, where only the events are outstanding (they were
  // issued ~1 us ago and the samples behind them have already arrived), and the bands then fly during the arithmetic.
#pragma unroll
  for (int q = 0; q < TILE_EPT / 2; ++q) asm volatile("" : "+v"(xw[q]), "+v"(yw[q]), "+v"(pw[q]));
#pragma unroll
  for (int k = 0; k < TILE_EPT; ++k) asm volatile("" : "+v"(tt[k]));
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  constexpr int UL_L = TILE_THREADS >= 1024 ? 2 : 4, UL_X = TILE_THREADS >= 1024 ? 1 : 2;
  const int dma_q0 = tid & ~63;  // first band quad of this wave in pass 0
  const int dma_lane = tid & 63;
  uint4* l_dmy = l_xm + band_xm_q(w_ts, tb.xmap_h);  // the dump area (tiled_dump_q): where waves past the end of a band dump their load
  {
#pragma unroll
    for (int k = 0; k < UL_L; ++k) {
      const int q0 = dma_q0 + k * nthreads;
      __builtin_amdgcn_global_load_lds((glb_void*)(g_lut + min(q0 + dma_lane, nq_lut - 1)),
                                       (lds_void*)(q0 < nq_lut ? l_lut + q0 : l_dmy), 16, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < UL_X; ++k) {
      const int q0 = dma_q0 + k * nthreads;
      __builtin_amdgcn_global_load_lds((glb_void*)(g_xm + min(q0 + dma_lane, nq_xm - 1)),
                                       (lds_void*)(q0 < nq_xm ? l_xm + q0 : l_dmy), 16, 0, 0);
    }
    (void)nq_all;
  }
  XM_STAMP(4);

  // ---- 4. with the bands in flight: unpack the events, their time columns (bit-exact with NumPy, see TimeNorm) ---------
  u32 x[TILE_EPT], y[TILE_EPT], lidx[TILE_EPT];
  bool used[TILE_EPT];
  int col[TILE_EPT];
#pragma unroll
  for (int k = 0; k < TILE_EPT; ++k) {
    x[k] = (xw[k >> 1] >> ((k & 1) * 16)) & 0xffff;
    y[k] = (yw[k >> 1] >> ((k & 1) * 16)) & 0xffff;
    used[k] = (inb >> k) & 1;
    if constexpr (HAS_P) used[k] = used[k] && (short)((pw[k >> 1] >> ((k & 1) * 16)) & 0xffff) == 1;
    lidx[k] = VEC ? (u32)tid * TILE_EPT + k : (u32)k * nthreads + tid;
  }
  tn.columns(tt, col);  // every lane; `used` masks the event below
  if (sorted_mode) {  // verify the time-sorted declaration: 2 compares per event
    bool bad = false;
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) {
      const u64 e = TimeCodec<T>::enc(tt[k]);
      bad = bad || (used[k] && (e < lo || e > hi));
    }
    if (__ballot(bad) && (tid & 63) == 0) {
      __hip_atomic_fetch_add(&st->cnt[parity][blk % CNT_SLOTS][CNT_UNSORTED], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&st->unsorted_sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (u32* hf = st->host_flags) host_flag_store(hf, tag);
    }
  }
  // Events outside the windows (unsorted / raster-ordered input, a noise event) take the global path -- the very functions
  // of the direct kernel -- in a compact loop: one pass handles every lane's next such event, so a wave with a single
  // stray event (the common case, 0.3 % of the events of a sorted frame but half of its waves) runs ~100 instructions, and
  // a wave without any skips the loop.  The block is issue-bound here (4 waves per SIMD), so the two dependent round
  // trips of a stray event are covered by the other waves' arithmetic; the band loads above are in flight meanwhile.
  int xl[TILE_EPT], tl[TILE_EPT];
  bool fast[TILE_EPT];
  u32 smask = 0;
#pragma unroll
  for (int k = 0; k < TILE_EPT; ++k) {
    xl[k] = (int)x[k] - x_lo;
    tl[k] = col[k] - ts_lo;
    fast[k] = used[k] && (u32)xl[k] < (u32)wx_eff && (u32)tl[k] < (u32)wts_eff && y[k] < (u32)tb.cam_h;
    smask |= used[k] && !fast[k] ? 1u << k : 0u;
  }
  u32 n_in = 0, n_oob = 0;
  u32 ovr = 0;  // PROJ32: bit k = event k's LUT entry was fetched from global memory and sits in xl[k]
  if constexpr (PROJ32) {
    // Every event must be resolved in the LDS slots (the key's order field is only the tile).  An event outside the LUT window
    // (x noise) but inside the time window fetches its LUT entry from global memory here and joins the fast path below; an
    // event outside the TIME window cannot use the slots: the frame is marked as failed and redone on the 64-bit path.
    bool bad = false;
    while (__ballot(smask != 0)) {
      const bool act = smask != 0;
      const int ks = act ? __builtin_ctz(smask) : 0;
      smask &= smask - 1;
      u32 ex = x[0], ey = y[0];
      int et = tl[0];
#pragma unroll
      for (int kk = 1; kk < TILE_EPT; ++kk) {
        const bool sel = ks == kk;
        ex = sel ? x[kk] : ex;
        ey = sel ? y[kk] : ey;
        et = sel ? tl[kk] : et;
      }
      bool oob = false;
      if (act) {
        if (ex >= (u32)tb.cam_w || ey >= (u32)tb.cam_h) {
          oob = true;  // map[y, x] IndexError (calib:279-280): dropped and counted, as on the other paths
        } else if ((u32)et >= (u32)wts_eff) {
          bad = true;
        } else {
          const u32 l = tb.lut[ex * (u32)tb.cam_h + ey];
#pragma unroll
          for (int kk = 0; kk < TILE_EPT; ++kk) xl[kk] = ks == kk ? (int)l : xl[kk];
          ovr |= 1u << ks;
        }
      }
      n_oob += __popcll(__ballot(oob));
    }
    if (__ballot(bad) && (tid & 63) == 0) {
      __hip_atomic_fetch_add(&st->cnt[parity][blk % CNT_SLOTS][CNT_UNSORTED], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (u32* hf = st->host_flags) host_flag_store(hf, tag);
    }
  } else
  while (__ballot(smask != 0)) {
    const bool act = smask != 0;
    const int ks = act ? __builtin_ctz(smask) : 0;
    smask &= smask - 1;
    u32 ex = x[0], ey = y[0], el = lidx[0];
    int ec = col[0];
#pragma unroll
    for (int kk = 1; kk < TILE_EPT; ++kk) {
      const bool sel = ks == kk;
      ex = sel ? x[kk] : ex;
      ey = sel ? y[kk] : ey;
      el = sel ? lidx[kk] : el;
      ec = sel ? col[kk] : ec;
    }
    bool oob = false, write = false;
    if (act) {
      const EventResult r = event_disparity_col(tb, ec, ex, ey, oob);
      u32 cell = 0;
      write = r.inlier;
      if (write && !event_cell<VIEW>(tb, r, ex, ey, cell)) {
        write = false;
        oob = true;
      }
      if (write) {
        if constexpr (CAM32) {
          cell = ex * (u32)tb.cam_h + ey;  // (the compact camera frame is column-major; event_cell has checked the pixel)
          __hip_atomic_fetch_max(reinterpret_cast<u32*>(frame) + cell,
                                 ((u32)(idx_offset + block_base + el + 1) << KEY32_DISP_BITS) | ((u32)r.disp & 0xfffu),
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          const u64 key = key_hi | ((idx_offset + block_base + el) << KEY_IDX_SHIFT) | (u64)(u32)r.disp;
          __hip_atomic_fetch_max(&frame[cell], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (VIEW == 0 && dirty) dirty[cell >> 4] = dirty_byte(tag);
        }
      }
    }
    n_in += __popcll(__ballot(write));
    n_oob += __popcll(__ballot(oob));
  }
  XM_STAMP(5);
  for (int q0 = dma_q0 + UL_L * nthreads; q0 < nq_lut; q0 += nthreads)  // taller tables / smaller blocks: the rest
    __builtin_amdgcn_global_load_lds((glb_void*)(g_lut + min(q0 + dma_lane, nq_lut - 1)), (lds_void*)(l_lut + q0), 16, 0, 0);
  for (int q0 = dma_q0 + UL_X * nthreads; q0 < nq_xm; q0 += nthreads)
    __builtin_amdgcn_global_load_lds((glb_void*)(g_xm + min(q0 + dma_lane, nq_xm - 1)), (lds_void*)(l_xm + q0), 16, 0, 0);
  // the LDS-direct loads are tracked by vmcnt like any vector load: all of them landed before the barrier
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  XM_STAMP(11);
  XM_STAMP(12);
  __syncthreads();  // bands visible
  XM_STAMP(6);

  // ---- 5. fast path, BRANCH-FREE so that the events' LDS round trips overlap: A1 + A2 out of the LDS bands with clamped
  //         addresses; then the LUT band's region becomes the slot array and collisions are resolved with ds_max_u32.
  bool wr[TILE_EPT];
  int slot[TILE_EPT];
  u32 val[TILE_EPT];
  {
    u32 l[TILE_EPT];
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) {
      const bool o_k = PROJ32 && ((ovr >> k) & 1u);
      l[k] = lut_t[fast[k] ? xl[k] * tb.cam_h + (int)y[k] : 0];
      if constexpr (PROJ32) {
        l[k] = o_k ? (u32)xl[k] : l[k];
        fast[k] = fast[k] || o_k;
      }
    }
    int xr[TILE_EPT], yr[TILE_EPT], xp[TILE_EPT];
    bool yok[TILE_EPT];
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) {
      xr[k] = (int)(short)(l[k] & 0xffff);
      yr[k] = (int)(short)(l[k] >> 16);
      yok[k] = fast[k] && yr[k] >= 0 && yr[k] < tb.xmap_h - 1;  // xmd:23
      xp[k] = (int)xm_t[yok[k] ? tl[k] * tb.xmap_h + yr[k] : 0];
    }
#pragma unroll
    for (int k = 0; k < TILE_EPT; ++k) {
      const int disp = (int)(short)(xp[k] - xr[k] - tb.x_offset);  // int16 wrap (xmd:27)
      bool write = yok[k] && disp >= 0;                               // xmd:29
      if constexpr (VIEW == 0) {
        int fc = (int)(short)(xr[k] + disp);  // = xp - x_offset (calib:300)
        if (fc < 0) fc += tb.rect_w;
        const bool in_frame = fc >= 0 && fc < tb.rect_w && yr[k] < tb.rect_h;
        n_oob += __popcll(__ballot(write && !in_frame));  // NumPy IndexError
        write = write && in_frame;
        slot[k] = tl[k] * tb.xmap_h + yr[k];
      } else if constexpr (CAM32) {
        slot[k] = xl[k] * tb.cam_h + (int)y[k];  // [window column][row], as the LUT band: the compact camera frame is column-major
      } else {
        slot[k] = (int)y[k] * w_x + xl[k];
      }
      wr[k] = write;
      val[k] = ((lidx[k] + 1) << 16) | (u32)disp;
      n_in += __popcll(__ballot(write));  // wavefront ballots instead of per-lane counters
    }
  }
  XM_STAMP(13);
  __syncthreads();  // every LUT gather has landed: the region can be reused
  {
    uint4* l_win = reinterpret_cast<uint4*>(win);
    for (int i = tid; i < win_q; i += nthreads) l_win[i] = make_uint4(0, 0, 0, 0);
  }
  __syncthreads();  // cleared slots visible
  XM_STAMP(14);
#pragma unroll
  for (int k = 0; k < TILE_EPT; ++k)
    if (wr[k] && !XM_ABL(1)) atomicMax(&win[slot[k]], val[k]);
  if ((tid & 63) == 0) {
    if (n_in) atomicAdd(&s_in, n_in);
    if (n_oob) atomicAdd(&s_oob, n_oob);
  }
  XM_STAMP(7);
  __syncthreads();
  XM_STAMP(8);

  // ---- 6. flush the winners: consecutive lanes -> consecutive slots = consecutive rows of one frame column (VIEW 0) /
  //         consecutive x of one row (VIEW 1).  One pass over the whole window (empty slots cost an LDS read, nothing
  //         else); all LDS reads of a thread are issued before its first atomic.
  {
    constexpr int FL = 4;
    static_assert(KEY_IDX_SHIFT == 16, "slot value ((local idx + 1) << 16 | disp) is added to the key as is");
    // key = tag | (global idx << 16) | disp, and the slot holds ((local idx + 1) << 16) | disp: one 64-bit add
    const u64 key_base = key_hi + ((idx_offset + block_base - 1) << KEY_IDX_SHIFT);
    const int per = VIEW == 0 ? tb.xmap_h : CAM32 ? tb.cam_h : w_x;  // slots per window column (VIEW 0, compact camera frame) / per camera row (VIEW 1)
    // (q, r) = divmod(slot, per), advanced incrementally: slot -> slot + nthreads is (q + dq, r + dr) with one carry
    const int dq = nthreads / per, dr = nthreads - dq * per;
    int q_i, r_i;
    {
      q_i = (int)((float)tid * (1.0f / (float)per));
      r_i = tid - q_i * per;
      if (r_i < 0) { q_i -= 1; r_i += per; }
      if (r_i >= per) { q_i += 1; r_i -= per; }
    }
    for (int i0 = tid; i0 < win_words; i0 += FL * nthreads) {
      u32 v[FL];
      int xv[FL], qs[FL], rs[FL];
#pragma unroll
      for (int j = 0; j < FL; ++j) {
        const int i = min(i0 + j * nthreads, win_words - 1);
        v[j] = win[i];
        xv[j] = VIEW == 0 ? (int)xm_t[i] : 0;
        qs[j] = q_i;
        rs[j] = r_i;
        q_i += dq;
        r_i += dr;
        if (r_i >= per) { r_i -= per; q_i += 1; }
      }
#pragma unroll
      for (int j = 0; j < FL; ++j) {
        const int i = i0 + j * nthreads;
        if (i < win_words && v[j]) {
          const int q = qs[j], r = rs[j];
          const u64 key = key_base + v[j];
          u32 cell;
          if constexpr (VIEW == 0) {  // q = window column, r = rectified row; the frame column comes from the X-map band
            int fc = (int)(short)(xv[j] - tb.x_offset);
            if (fc < 0) fc += tb.rect_w;
            cell = (u32)fc * (u32)tb.rect_h + (u32)r;
          } else if constexpr (CAM32) {  // q = window column, r = camera row: lanes walk consecutive rows of one column of the
            cell = (u32)(x_lo + q) * (u32)tb.cam_h + (u32)r;  // column-major frame (64 lanes = 256 contiguous bytes)
          } else {  // q = camera row, r = x - x_lo
            cell = (u32)q * (u32)tb.cam_w + (u32)(x_lo + r);
          }
          if constexpr (PROJ32) {  // tag4 | tile | disparity into the compact frame (see key32_tag)
            __hip_atomic_fetch_max(reinterpret_cast<u32*>(frame) + cell, key32_tag(tag) | (tile << KEY32_DISP_BITS) | (v[j] & 0xfffu),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else if constexpr (CAM32) {  // (event index + 1) | disparity; the slot holds ((local index + 1) << 16) | disparity
            __hip_atomic_fetch_max(reinterpret_cast<u32*>(frame) + cell,
                                   (((u32)(idx_offset + block_base) + (v[j] >> 16)) << KEY32_DISP_BITS) | (v[j] & 0xfffu),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            if (!XM_ABL(0)) __hip_atomic_fetch_max(&frame[cell], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (VIEW == 0 && dirty) dirty[cell >> 4] = dirty_byte(tag);  // consecutive lanes = consecutive rows
          }
        }
      }
    }
  }
  XM_STAMP(9);
  if (tid == 0) flush_counts(st->cnt[parity][blk % CNT_SLOTS], s_in, s_oob);
  XM_STAMP(10);
}

template <typename T, bool AOS, bool HAS_P, int VIEW, bool VEC, bool KEY32 = false>
__global__ XM_K1_BOUNDS void k_scatter_tiled(
    const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys, const T* __restrict__ ts,
    const int16_t* __restrict__ ps, const uint4* __restrict__ aos, u64 n, u64 idx_offset, DevTables tb, SlotState* st,
    u32 tag_override, u64 mm_lo, u64 mm_hi, const void* __restrict__ mm_ext, u64* __restrict__ frame,
    unsigned char* __restrict__ dirty, int w_ts, int w_x, int sorted_mode) {
  // All kernel arguments into SGPRs in ONE scalar-load round trip: a test that needs every one of them, placed first.
  // Left alone the compiler fetches them lazily, block by block -- eight dependent s_load -> s_waitcnt pairs along the
  // critical chain of every block (seen in the ISA).  (Inline asm would do it too, but makes every later uniform load a
  // vector load.)  Never true: sizes are non-negative and device addresses have bit 63 clear.
  {
    const u64 pp = (u64)xs | (u64)ys | (u64)ts | (u64)ps | (u64)aos | (u64)tb.lut | (u64)tb.xmap | (u64)st | (u64)frame |
                   (u64)dirty | (u64)mm_ext | n | idx_offset;
    const int pi = tb.cam_w | tb.cam_h | tb.xmap_w | tb.xmap_h | tb.t_px_scale | tb.x_offset | tb.rect_w | tb.rect_h |
                   (int)tag_override | w_ts | w_x | sorted_mode;
    if ((long long)(pp | (u64)(long long)pi) < 0) return;
  }
  scatter_tiled_body<T, AOS, HAS_P, VIEW, VEC, KEY32>(xs, ys, ts, ps, aos, n, idx_offset, tb, st, tag_override, mm_lo, mm_hi, mm_ext,
                                                      frame, dirty, w_ts, w_x, sorted_mode, blockIdx.x, gridDim.x);
}

// A frame without events inside a multi-frame launch: only the slot bookkeeping K1's block 0 does.
__device__ inline void scatter_empty_frame(SlotState* st, int sorted_mode) {
  const u32 tag = sorted_mode ? st->tag_b + 1 : st->tag_a;
  const u32 parity = tag & 1;
  if (threadIdx.x == 0) {
    if (sorted_mode) {
      st->tag_a = tag;
      st->mm[parity][0][0] = MM_INIT_MIN;
      st->mm[parity][0][1] = MM_INIT_MAX;
    } else {
      st->tag_b = tag;
    }
  }
  rearm_minmax(st, parity, threadIdx.x, blockDim.x);
}

// Multi-frame launch: grid = (tiles of the largest frame, frames).  One launch exposes frames x tiles blocks to the chip
// (60 frames: 14 700 blocks instead of 245): no per-frame launch ramp, the CUs always have a next block to pick up.  Every
// frame owns a key frame + state (FrameDesc), so blocks of different frames never meet.  The frame's size comes from
// device memory: the same launch serves frames cut out of a device-resident stream (ingest) whose length the host never saw.
template <typename T, bool AOS, bool HAS_P, int VIEW, bool VEC, bool KEY32 = false, int COND = 0>
__global__ XM_K1_BOUNDS void k_scatter_tiled_batch(const FrameDesc* __restrict__ descs, DevTables tb, int w_ts, int w_x,
                                                   int sorted_mode) {
  const FrameDesc d = descs[blockIdx.y];  // block-uniform: scalar loads
  if (!d.valid || frame_skipped<COND>(d.st)) return;
  const u32 evb = blockDim.x * TILE_EPT;
  const u32 nblk = (u32)((d.n + evb - 1) / evb);
  if constexpr (COND == 1) {
    // The redo node of a captured batch: launched with a FEW blocks per frame, which walk the frame's tiles when the frame's
    // attempt failed -- in the usual case (it held) the node costs a handful of blocks that read two words and return, not a
    // block per tile (each with the tiled kernel's LDS to allocate: 10 us per 60-frame replay)
    if (d.n == 0) {
      if (blockIdx.x == 0) scatter_empty_frame(d.st, sorted_mode);
      return;
    }
    for (u32 b = blockIdx.x; b < nblk; b += gridDim.x) {
      scatter_tiled_body<T, AOS, HAS_P, VIEW, VEC, KEY32>(d.x, d.y, (const T*)d.t, d.p, d.aos, d.n, 0ull, tb, d.st, 0u, 0ull, 0ull,
                                                          nullptr, d.key_frame, nullptr, w_ts, w_x, sorted_mode, b, nblk);
      __syncthreads();  // the next tile clears the LDS this one's flush has just read
    }
    return;
  }
  if (blockIdx.x >= nblk) {
    if (d.n == 0 && blockIdx.x == 0) scatter_empty_frame(d.st, sorted_mode);
    return;
  }
  scatter_tiled_body<T, AOS, HAS_P, VIEW, VEC, KEY32>(d.x, d.y, (const T*)d.t, d.p, d.aos, d.n, 0ull, tb, d.st, 0u, 0ull, 0ull,
                                                      nullptr, d.key_frame, nullptr, w_ts, w_x, sorted_mode, blockIdx.x, nblk);
}

}  // namespace xm
