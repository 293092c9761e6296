// xmaps_k1direct.hpp -- K1, one thread per event: rectify-LUT gather -> time column -> X-map gather -> disparity + inlier masks
// -> one 64-bit atomic max per inlier (cam_proj_calibration.py:277-281 / 299-317, x_maps_disparity.py:16-29).  The kernel of
// sparse frames (single, or cut by the device ingest) and of shards.  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp.  scatter_empty_frame is only declared here: xmaps_k1tiles.hpp defines it.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// =====================================================================================================
// K1: the fused per-event kernel.
// =====================================================================================================

// EPT = events per thread: 4 (vector loads: 8 B of x, 8 B of y, 2 x 16 B of t, 8 B of p per thread;
// needs 8/8/16/8-byte aligned columns) or 1 (any alignment).  AOS: one 16-B record per thread.
template <typename T, bool AOS, bool HAS_P, int EPT, int VIEW>
__device__ __forceinline__ void scatter_direct_body(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                    const T* __restrict__ ts, const int16_t* __restrict__ ps,
                                                    const uint4* __restrict__ aos, u64 n, u64 idx_offset,
                                                    const DevTables& tb, SlotState* st, u32 tag_override, u64 mm_lo,
                                                    u64 mm_hi, const void* __restrict__ mm_ext, u64* __restrict__ frame,
                                                    unsigned char* __restrict__ dirty, const u32 blk, const int sorted_mode = 0) {
  // sorted_mode (never with a polarity column): the caller expects the frame sorted by t -- extrema = t[0], t[n-1], K0 is not
  // launched, and every event is verified against them below exactly as k_scatter_tiled does (a failure marks the frame: it is
  // redone with K0).  The reference's own recordings are frames of this kind: ~150 k sorted events, too sparse for the tiles.
  const bool srt = sorted_mode != 0 && !tag_override && !HAS_P && n > 0;
  const u32 tag = tag_override ? tag_override : (srt ? st->tag_b + 1 : st->tag_a);
  const u32 parity = tag & 1;
  u64 lo, hi;
  if (tag_override) {  // sharded mode: the FRAME's extrema come from the all-reduce of the shards' extrema
    lo = mm_lo;
    hi = mm_hi;
    if (mm_ext) {  // {tmin, -tmax} in device memory
      const ulonglong2 e = ext_minmax<T>(mm_ext);
      lo = e.x;
      hi = e.y;
    }
  } else if (srt) {
    T t_first, t_last;
    if constexpr (AOS) {
      const uint4 a = aos[0], b = aos[n - 1];
      t_first = rec_t<T>(a);
      t_last = rec_t<T>(b);
    } else {
      t_first = ts[0];
      t_last = ts[n - 1];
    }
    lo = TimeCodec<T>::enc(t_first);
    hi = TimeCodec<T>::enc(t_last);
    if (hi < lo) hi = lo;  // not sorted at all: keep the arithmetic defined; the verification flags the frame
    if (blk == 0) {
      if (threadIdx.x == 0) {
        st->tag_a = tag;            // K2 reads tag_a and copies it to tag_b
        st->mm[parity][0][0] = lo;  // for xm_frame_stats.t_min / t_max
        st->mm[parity][0][1] = hi;
      }
      rearm_minmax(st, parity, threadIdx.x, BLOCK);
    }
  } else {
    load_frame_minmax(st, parity, lo, hi);
    if (blk == 0) {
      if (threadIdx.x == 0) st->tag_b = tag;
      rearm_minmax(st, parity, threadIdx.x, BLOCK);
    }
  }
  const TimeNorm<T> tn(TimeCodec<T>::dec(lo), TimeCodec<T>::dec(hi), tb.t_px_scale);
  const u64 key_hi = (u64)tag << KEY_TAG_SHIFT;

  u32 x[EPT], y[EPT];
  T t[EPT];
  bool used[EPT];
  const u64 base = ((u64)blk * BLOCK + threadIdx.x) * EPT;
  if constexpr (AOS) {
    static_assert(EPT == 1, "AoS: one record per thread");
    used[0] = base < n;
    if (used[0]) {
      uint4 r = aos[base];
      x[0] = rec_x(r);
      y[0] = rec_y(r);
      t[0] = rec_t<T>(r);
      if (HAS_P) used[0] = (short)(r.y & 0xffff) == 1;
    }
  } else if constexpr (EPT == 4) {
    if (base + 4 <= n) {
      const uint2 xv = *reinterpret_cast<const uint2*>(xs + base);
      const uint2 yv = *reinterpret_cast<const uint2*>(ys + base);
      x[0] = xv.x & 0xffff; x[1] = xv.x >> 16; x[2] = xv.y & 0xffff; x[3] = xv.y >> 16;
      y[0] = yv.x & 0xffff; y[1] = yv.x >> 16; y[2] = yv.y & 0xffff; y[3] = yv.y >> 16;
      if constexpr (sizeof(T) == 8) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(ts + base);
        const longlong2 b = *reinterpret_cast<const longlong2*>(ts + base + 2);
        __builtin_memcpy(&t[0], &a.x, 8); __builtin_memcpy(&t[1], &a.y, 8);
        __builtin_memcpy(&t[2], &b.x, 8); __builtin_memcpy(&t[3], &b.y, 8);
      } else {
        const float4 a = *reinterpret_cast<const float4*>(ts + base);
        __builtin_memcpy(&t[0], &a.x, 4); __builtin_memcpy(&t[1], &a.y, 4);
        __builtin_memcpy(&t[2], &a.z, 4); __builtin_memcpy(&t[3], &a.w, 4);
      }
      used[0] = used[1] = used[2] = used[3] = true;
      if constexpr (HAS_P) {
        const uint2 pv = *reinterpret_cast<const uint2*>(ps + base);
        used[0] = (short)(pv.x & 0xffff) == 1; used[1] = (short)(pv.x >> 16) == 1;
        used[2] = (short)(pv.y & 0xffff) == 1; used[3] = (short)(pv.y >> 16) == 1;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        used[k] = base + k < n;
        if (used[k]) {
          x[k] = xs[base + k];
          y[k] = ys[base + k];
          t[k] = ts[base + k];
          if (HAS_P) used[k] = ps[base + k] == 1;
        }
      }
    }
  } else {
    used[0] = base < n;
    if (used[0]) {
      x[0] = xs[base];
      y[0] = ys[base];
      t[0] = ts[base];
      if (HAS_P) used[0] = ps[base] == 1;
    }
  }

  if (srt) {  // verify the expectation: 2 compares per event
    bool bad = false;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      const u64 e = TimeCodec<T>::enc(used[k] ? t[k] : TimeCodec<T>::dec(lo));
      bad = bad || e < lo || e > hi;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) {
      __hip_atomic_fetch_add(&st->cnt[parity][blk % CNT_SLOTS][CNT_UNSORTED], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&st->unsorted_sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (u32* hf = st->host_flags) host_flag_store(hf, tag);
    }
  }
  u32 n_in = 0, n_oob = 0;
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    bool oob;
    const EventResult r = event_disparity<T>(tb, tn, x[k], y[k], t[k], used[k], oob);
    bool write = r.inlier;
    u32 cell = 0;
    if (write && !event_cell<VIEW>(tb, r, x[k], y[k], cell)) {
      write = false;
      oob = true;
    }
    if (write) {
      const u64 key = key_hi | ((idx_offset + base + k) << KEY_IDX_SHIFT) | (u64)(u32)r.disp;
      __hip_atomic_fetch_max(&frame[cell], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (VIEW == 0 && dirty) dirty[cell >> 4] = dirty_byte(tag);
    }
    // wavefront ballots: one popcount per wave instead of per-lane counters
    n_in += __popcll(__ballot(write));
    n_oob += __popcll(__ballot(oob));
  }
  __shared__ u32 s_in, s_oob;
  if (threadIdx.x == 0) {
    s_in = 0;
    s_oob = 0;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    if (n_in) atomicAdd(&s_in, n_in);
    if (n_oob) atomicAdd(&s_oob, n_oob);
  }
  __syncthreads();
  if (threadIdx.x == 0) flush_counts(st->cnt[parity][blk % CNT_SLOTS], s_in, s_oob);
}

template <typename T, bool AOS, bool HAS_P, int EPT, int VIEW>
__global__ __launch_bounds__(BLOCK) void k_scatter(const uint16_t* __restrict__ xs, const uint16_t* __restrict__ ys,
                                                   const T* __restrict__ ts, const int16_t* __restrict__ ps,
                                                   const uint4* __restrict__ aos, u64 n, u64 idx_offset,
                                                   DevTables tb, SlotState* st, u32 tag_override, u64 mm_lo,
                                                   u64 mm_hi, const void* __restrict__ mm_ext, u64* __restrict__ frame,
                                                   unsigned char* __restrict__ dirty, int sorted_mode) {
  scatter_direct_body<T, AOS, HAS_P, EPT, VIEW>(xs, ys, ts, ps, aos, n, idx_offset, tb, st, tag_override, mm_lo, mm_hi, mm_ext,
                                                frame, dirty, blockIdx.x, sorted_mode);
}

__device__ inline void scatter_empty_frame(SlotState* st, int sorted_mode);

// one thread per event, frame from a descriptor in device memory (sparse frames of a device-resident stream: ingest);
// grid = (blocks for the largest frame the host allows for, frames); a frame without events still does block 0's bookkeeping
template <typename T, bool AOS, bool HAS_P, int VIEW>
__global__ __launch_bounds__(BLOCK) void k_scatter_direct_batch(const FrameDesc* __restrict__ descs, DevTables tb, int sorted_mode) {
  const FrameDesc d = descs[blockIdx.y];
  if (!d.valid) return;
  if (blockIdx.x != 0 && (u64)blockIdx.x * BLOCK >= d.n) return;
  if (d.n == 0 && sorted_mode) {  // (only block 0 gets here) nothing to take the extrema from: what the tiled kernel does
    scatter_empty_frame(d.st, sorted_mode);
    return;
  }
  scatter_direct_body<T, AOS, HAS_P, 1, VIEW>(d.x, d.y, (const T*)d.t, d.p, d.aos, d.n, 0ull, tb, d.st, 0u, 0ull, 0ull, nullptr,
                                              d.key_frame, nullptr, blockIdx.x, sorted_mode);
}

}  // namespace xm
