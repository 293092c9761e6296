// xmaps_k0.hpp -- K0: the frame's extrema of t (x_maps_disparity.py:12-13) as a streaming reduction, for one frame, for the
// frames of a multi-frame launch, and their export for the all-reduce of a sharded frame.  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp only.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// =====================================================================================================
// K0: min / max of t over the frame's events (those with p == 1 when a polarity column is given).
//   SoA : t[n] (+ p[n]);  VEC = events per 16-byte load of int64 t (2) or scalar (1)
//   AoS : EventCD records, one 16-byte load per event
// Also: advances the slot's frame tag (block 0) and counts the used events.
// =====================================================================================================
// (K0_UN, 16-byte loads of t in flight per thread on the vector path: xmaps_geometry.hpp)
template <typename T, bool AOS, bool HAS_P, int VEC>
__device__ __forceinline__ void minmax_body(const T* __restrict__ t, const int16_t* __restrict__ p,
                                            const uint4* __restrict__ aos, u64 n, SlotState* st, u32 tag_override,
                                            const u32 blk, const u32 nblk) {
  // the frame tag is only needed for the final atomics: its load (kernarg -> st -> tag_b, a dependent scalar chain) must
  // not sit in front of the event loads
  u64 lo = MM_INIT_MIN, hi = MM_INIT_MAX;
  u32 used = 0;
  const u64 stride = (u64)nblk * BLOCK;
  if constexpr (AOS) {
    for (u64 i = (u64)blk * BLOCK + threadIdx.x; i < n; i += stride) {
      uint4 r = aos[i];
      bool ok = !HAS_P || (short)(r.y & 0xffff) == 1;
      if (ok) {
        u64 e = TimeCodec<long long>::enc(rec_t(r));
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
        ++used;
      }
    }
  } else if constexpr (VEC == 2) {
    const u64 n2 = n >> 1;
    const longlong2* t2 = reinterpret_cast<const longlong2*>(t);
    const u32* p2 = reinterpret_cast<const u32*>(p);
    // K0_UN independent 16-byte loads per thread per sweep: latency-bound otherwise (8 MB must be in flight at once)
    for (u64 i0 = (u64)blk * BLOCK + threadIdx.x; i0 < n2; i0 += K0_UN * stride) {
      longlong2 v[K0_UN];
      u32 pp[K0_UN];
      bool in[K0_UN];
#pragma unroll
      for (int j = 0; j < K0_UN; ++j) {
        const u64 i = i0 + (u64)j * stride;
        in[j] = i < n2;
        if (in[j]) {
          v[j] = t2[i];
          if constexpr (HAS_P) pp[j] = p2[i];
        }
      }
#pragma unroll
      for (int j = 0; j < K0_UN; ++j) {
        if (!in[j]) continue;
        bool ok0 = true, ok1 = true;
        if constexpr (HAS_P) {
          ok0 = (short)(pp[j] & 0xffff) == 1;
          ok1 = (short)(pp[j] >> 16) == 1;
        }
        if (ok0) {
          u64 e = TimeCodec<T>::enc((T)v[j].x);
          lo = e < lo ? e : lo;
          hi = e > hi ? e : hi;
          ++used;
        }
        if (ok1) {
          u64 e = TimeCodec<T>::enc((T)v[j].y);
          lo = e < lo ? e : lo;
          hi = e > hi ? e : hi;
          ++used;
        }
      }
    }
    if ((n & 1) && blk == 0 && threadIdx.x == 0) {
      u64 i = n - 1;
      if (!HAS_P || p[i] == 1) {
        u64 e = TimeCodec<T>::enc(t[i]);
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
        ++used;
      }
    }
  } else {
    for (u64 i = (u64)blk * BLOCK + threadIdx.x; i < n; i += stride) {
      if (!HAS_P || p[i] == 1) {
        u64 e = TimeCodec<T>::enc(t[i]);
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
        ++used;
      }
    }
  }

  const u32 tag = tag_override ? tag_override : st->tag_b + 1;
  const u32 parity = tag & 1;
  if (blk == 0 && threadIdx.x == 0) st->tag_a = tag;
  // wave -> block -> one pair of fire-and-forget atomics per block, spread over MM_SLOTS addresses.  The three wave
  // reductions advance together: 6 dependent cross-lane steps instead of 18.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 lo2 = __shfl_xor(lo, o, 64), hi2 = __shfl_xor(hi, o, 64);
    const u32 u2 = __shfl_xor(used, o, 64);
    lo = lo2 < lo ? lo2 : lo;
    hi = hi2 > hi ? hi2 : hi;
    used += u2;
  }
  __shared__ u64 s_lo[BLOCK / 64], s_hi[BLOCK / 64];
  __shared__ u32 s_used[BLOCK / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
    s_used[wave] = used;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 u = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
      u += s_used[w];
    }
    if (u) {
      const int slot = blk % MM_SLOTS;
      __hip_atomic_fetch_min(&st->mm[parity][slot][0], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(&st->mm[parity][slot][1], hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&st->cnt[parity][blk % CNT_SLOTS][CNT_USED], u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <typename T, bool AOS, bool HAS_P, int VEC>
__global__ __launch_bounds__(BLOCK) void k_minmax(const T* __restrict__ t, const int16_t* __restrict__ p,
                                                  const uint4* __restrict__ aos, u64 n, SlotState* st,
                                                  u32 tag_override) {
  // every kernel argument in one scalar round trip (see k_scatter_tiled); never true
  if ((long long)((u64)t | (u64)p | (u64)aos | (u64)st | n | (u64)tag_override) < 0) return;
  minmax_body<T, AOS, HAS_P, VEC>(t, p, aos, n, st, tag_override, blockIdx.x, gridDim.x);
}

// multi-frame launch: grid = (blocks per frame, frames); frame f = descs[f]
template <typename T, bool AOS, bool HAS_P, int VEC, int COND = 0>
__global__ __launch_bounds__(BLOCK) void k_minmax_batch(const FrameDesc* __restrict__ descs) {
  const FrameDesc d = descs[blockIdx.y];
  if (!d.valid || frame_skipped<COND>(d.st)) return;
  minmax_body<T, AOS, HAS_P, VEC>((const T*)d.t, d.p, d.aos, d.n, d.st, 0u, blockIdx.x, gridDim.x);
}

// Sharded frames: a shard's extrema as K0 left them (parity of `tag`) -> {tmin, -tmax} in a 16-byte device buffer of a
// reduction-friendly type (int64 for int64 t, f64 for float t: both exact), so that ONE MIN all-reduce of that buffer over
// the ranks yields the frame's extrema without any host round trip.  Empty shard -> {+max, +max} (neutral for MIN).
template <typename T>
__global__ __launch_bounds__(64) void k_minmax_export(const SlotState* __restrict__ st, u32 tag, void* __restrict__ out) {
  u64 lo, hi;
  load_frame_minmax(st, tag & 1, lo, hi);
  if (threadIdx.x != 0) return;
  const bool empty = lo == MM_INIT_MIN && hi == MM_INIT_MAX;
  if constexpr (std::is_same<T, long long>::value) {
    long long* o = static_cast<long long*>(out);
    const long long big = 0x7fffffffffffffffll;
    const long long tmax = TimeCodec<T>::dec(hi);
    o[0] = empty ? big : TimeCodec<T>::dec(lo);
    o[1] = empty || tmax == (-big - 1) ? big : -tmax;
  } else {
    double* o = static_cast<double*>(out);
    o[0] = empty ? __builtin_inf() : (double)TimeCodec<T>::dec(lo);
    o[1] = empty ? __builtin_inf() : -(double)TimeCodec<T>::dec(hi);
  }
}

}  // namespace xm
