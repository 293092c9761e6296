// xmaps_timecal.hpp -- gfx950 device code of the projector time-map calibration (xm_timecal_*): camera time surfaces of a white
// frame projected onto a plane -> the calibrated projector-space time map that build_tables(projector_time_map=) takes.
//
// The reference ships no code for this step.  The recipe is the paper's (section 3.3, "Time map calibration": several camera
// time maps normalised to (0, 1) and averaged, a binary map, the projected frame's corners, a projective warp to the projector's
// width x height, missing values interpolated linearly between actual lines); the arithmetic below is THIS BUILD'S DEFINITION,
// pinned bit for bit to the NumPy oracle of tests/time_cal_cases.py.  Float64 throughout, every expression in the order written,
// nothing fused (-ffp-contract=off).
//   T0 k_surf_extrema     (xmaps_surface.hpp, as it is) lo / hi / nnz over a surface's non-zero entries -> one partial per block
//   T1 k_tcal_accumulate  folds a surface's partials the way S1 does; a surface that is not surf_normalisable is skipped and
//                         counted; per pixel with v != 0: sum = sum + surf_norm(v), cnt += 1.  ONE thread owns a pixel and walks
//                         the group's surfaces in index order: no floating-point atomic, and the sums depend on the sequence of
//                         surfaces only, not on how they were grouped into calls
//   T2 k_tcal_mean        valid = cnt >= min_count; mean = valid ? sum / f64(cnt) : 0
//   T3 k_tcal_corners     core = valid on the whole 3 x 3 neighbourhood (never an image-border pixel); TL = argmin(x + y),
//                         TR = argmax(x - y), BR = argmax(x + y), BL = argmin(x - y) over the core pixels, ties to the smallest
//                         raster index: four packed keys (score << 32 | raster), one integer atomic min per block and key
//   T4 k_tcal_warp        per projector pixel (u, v): (X, Y, D) = h (u, v, 1), x = X / D, y = Y / D, the four taps (x0, y0),
//                         (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with the bilinear weights; a tap outside the image or not valid
//                         has weight 0; den / num summed in tap order; den > 0: num / den, present; else 0, missing
//   T5 k_tcal_fill        one block per projector row (a projector line is a column: the fill runs across the columns): the
//                         next present column by a backward min-scan, the previous one by a forward max-scan (wave scans + a
//                         cross-wave step in LDS, the running value carried across the chunks of a row); a missing pixel between
//                         two present ones gets m_l + (m_r - m_l) * ((u - u_l) / (u_r - u_l)), with one side only that side's
//                         value; a row without a present pixel stays 0 and is counted.  ONE cast to float32 at the store.
// No kernel waits for another block; every cross-block dependency is a kernel boundary.  Plain stores, except the integer atomics
// of T3's keys and of the four counters (integer min / add: the result does not depend on their order).
//
// x and y are compared as floats before an index is formed (NaN, +-inf from D = 0, or beyond the image: missing), as the rig-map
// kernels do.  NaN / +-inf surface entries are out of contract as in xmaps_surface.hpp.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_surface.hpp"  // k_surf_extrema, SurfPart1, surf_norm, surf_normalisable

namespace xm {

constexpr int TCAL_BATCH = 16;  // surfaces whose folded extrema a block holds in LDS at a time
constexpr u64 TCAL_NO_KEY = ~0ull;

struct TcalCounts {  // device side of the object's surface counters (one thread of one block adds to them, launches are ordered)
  u64 n_added, n_skipped;
};
struct TcalAcc {  // what T3 .. T5 reduce into; cleared by the host in front of them
  u64 key[4];     // TL, TR, BR, BL: score << 32 | raster index, integer min
  u32 n_valid, n_core, n_missing, n_unfilled;
};

// T1 ------------------------------------------------------------------------------------------------------------------------
// grid = the blocks of k_surf_extrema over one surface (nb): a thread owns SURF_RED_ITEMS pixels, base + k * BLOCK
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_tcal_accumulate(const T* __restrict__ surf, u32 n_px, u32 n_surf,
                                                            const SurfPart1* __restrict__ part1, double* __restrict__ sum,
                                                            u32* __restrict__ cnt, TcalCounts* __restrict__ counts) {
  __shared__ double s_lo[TCAL_BATCH], s_den[TCAL_BATCH];
  __shared__ u32 s_ok[TCAL_BATCH];
  const u32 nb = gridDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 base = blockIdx.x * (u32)SURF_RED_CHUNK + threadIdx.x;
  double acc[SURF_RED_ITEMS];
  u32 c[SURF_RED_ITEMS];
#pragma unroll
  for (int k = 0; k < SURF_RED_ITEMS; ++k) {
    const u32 i = base + (u32)k * BLOCK;
    acc[k] = i < n_px ? sum[i] : 0.0;
    c[k] = i < n_px ? cnt[i] : 0u;
  }
  u32 n_skipped = 0;
  for (u32 s0 = 0; s0 < n_surf; s0 += TCAL_BATCH) {
    const u32 nbatch = n_surf - s0 < (u32)TCAL_BATCH ? n_surf - s0 : (u32)TCAL_BATCH;
    for (u32 j = wave; j < nbatch; j += BLOCK / 64) {  // a wave folds a surface's S0 partials (a few KB, L2-hot)
      const SurfPart1* p1 = part1 + (size_t)(s0 + j) * nb;
      double lo = INFINITY, hi = -INFINITY;
      u32 nnz = 0;
      for (u32 i = lane; i < nb; i += 64) {
        const SurfPart1 p = p1[i];
        lo = p.lo < lo ? p.lo : lo;
        hi = p.hi > hi ? p.hi : hi;
        nnz += (u32)p.nnz;
      }
      lo = wave_min_f64(lo);
      hi = wave_max_f64(hi);
      nnz = wave_sum_u32(nnz);
      if (lane == 0) s_lo[j] = lo, s_den[j] = hi - lo, s_ok[j] = surf_normalisable(lo, hi, nnz) ? 1u : 0u;
    }
    __syncthreads();
    for (u32 j = 0; j < nbatch; ++j) {  // the group's surfaces in index order
      if (!s_ok[j]) {                  // (block-uniform)
        n_skipped += 1;
        continue;
      }
      const double lo = s_lo[j], den = s_den[j];
      const T* img = surf + (size_t)(s0 + j) * n_px;
      T v[SURF_RED_ITEMS];
#pragma unroll
      for (int k = 0; k < SURF_RED_ITEMS; ++k) {
        const u32 i = base + (u32)k * BLOCK;
        v[k] = i < n_px ? img[i] : (T)0;
      }
#pragma unroll
      for (int k = 0; k < SURF_RED_ITEMS; ++k) {
        if ((double)v[k] != 0.0) {
          acc[k] = acc[k] + surf_norm(v[k], lo, den);
          c[k] += 1;
        }
      }
    }
    __syncthreads();  // (the next batch overwrites the LDS words)
  }
#pragma unroll
  for (int k = 0; k < SURF_RED_ITEMS; ++k) {
    const u32 i = base + (u32)k * BLOCK;
    if (i < n_px) sum[i] = acc[k], cnt[i] = c[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts->n_added += n_surf;
    counts->n_skipped += n_skipped;
  }
}

// T2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_tcal_mean(const double* __restrict__ sum, const u32* __restrict__ cnt, u32 n_px, u32 min_count,
                                                      double* __restrict__ mean, uint8_t* __restrict__ valid) {
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n_px) return;
  const u32 c = cnt[i];
  const bool ok = c >= min_count;  // (min_count >= 1: c != 0)
  mean[i] = ok ? sum[i] / (double)c : 0.0;
  valid[i] = ok ? 1 : 0;
}

// T3 ------------------------------------------------------------------------------------------------------------------------
// one thread per pixel, raster order.  The four scores are turned so that every corner is a minimum and non-negative:
// x + y, w - (x - y), (w + h) - (x + y), h + (x - y) (all < 2^32: w * h < 2^31); the raster index below them breaks ties.
__global__ __launch_bounds__(BLOCK) void k_tcal_corners(const uint8_t* __restrict__ valid, int w, int h, TcalAcc* __restrict__ acc) {
  __shared__ u64 s_key[BLOCK / 64][4];
  __shared__ u32 s_n[BLOCK / 64][2];
  const u32 n_px = (u32)w * (u32)h, i = blockIdx.x * BLOCK + threadIdx.x;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool v = false, core = false;
  u32 x = 0, y = 0;
  if (i < n_px) {
    y = i / (u32)w, x = i - y * (u32)w;
    v = valid[i] != 0;
    if (v && x > 0 && y > 0 && x + 1 < (u32)w && y + 1 < (u32)h) {
      core = true;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) core = core && valid[(size_t)(y + dy) * (u32)w + (x + dx)] != 0;
    }
  }
  u64 key[4] = {TCAL_NO_KEY, TCAL_NO_KEY, TCAL_NO_KEY, TCAL_NO_KEY};
  if (core) {
    key[0] = ((u64)(x + y) << 32) | i;
    key[1] = ((u64)((u32)w - x + y) << 32) | i;
    key[2] = ((u64)((u32)w + (u32)h - x - y) << 32) | i;
    key[3] = ((u64)((u32)h + x - y) << 32) | i;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) key[k] = wave_min_u64(key[k]);
  const u32 nv = (u32)__popcll(__ballot(v)), nc = (u32)__popcll(__ballot(core));
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_key[wave][k] = key[k];
    s_n[wave][0] = nv, s_n[wave][1] = nc;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    u64 m = s_key[0][threadIdx.x];
#pragma unroll
    for (int wv = 1; wv < BLOCK / 64; ++wv) m = s_key[wv][threadIdx.x] < m ? s_key[wv][threadIdx.x] : m;
    if (m != TCAL_NO_KEY) __hip_atomic_fetch_min(&acc->key[threadIdx.x], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (threadIdx.x < 6) {
    const u32 which = threadIdx.x - 4;
    u32 n = 0;
#pragma unroll
    for (int wv = 0; wv < BLOCK / 64; ++wv) n += s_n[wv][which];
    if (n) __hip_atomic_fetch_add(which ? &acc->n_core : &acc->n_valid, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// T4 ------------------------------------------------------------------------------------------------------------------------
struct TcalWarpArgs {
  double h[9];  // projector pixel (u, v, 1) -> camera position, homogeneous
  int cam_w, cam_h, proj_w, proj_h;
  const double* mean;    // [cam_h][cam_w]
  const uint8_t* valid;
  double* value;         // [proj_h][proj_w]: the pre-fill map, 0 where missing
  uint8_t* present;
  TcalAcc* acc;
};

__device__ __forceinline__ void tcal_tap(const TcalWarpArgs& a, int x, int y, double wgt, double& den, double& num) {
  double m = 0.0;
  bool ok = x >= 0 && x < a.cam_w && y >= 0 && y < a.cam_h;
  if (ok) {
    const size_t i = (size_t)y * (size_t)a.cam_w + (size_t)x;
    ok = a.valid[i] != 0;
    m = ok ? a.mean[i] : 0.0;
  }
  const double wt = ok ? wgt : 0.0;
  den = den + wt;
  num = num + wt * m;
}

__global__ __launch_bounds__(BLOCK) void k_tcal_warp(const TcalWarpArgs a) {
  const u64 n_px = (u64)a.proj_w * (u64)a.proj_h, i = (u64)blockIdx.x * BLOCK + threadIdx.x;
  bool present = false;
  double val = 0.0;
  if (i < n_px) {
    const u32 vi = (u32)(i / (u32)a.proj_w), ui = (u32)(i - (u64)vi * (u32)a.proj_w);
    const double u = (double)ui, v = (double)vi;
    const double X = a.h[0] * u + a.h[1] * v + a.h[2];
    const double Y = a.h[3] * u + a.h[4] * v + a.h[5];
    const double D = a.h[6] * u + a.h[7] * v + a.h[8];
    const double x = X / D, y = Y / D;
    // a tap can only lie inside the image for -1 < x < cam_w, -1 < y < cam_h (NaN fails every comparison)
    if (x > -1.0 && x < (double)a.cam_w && y > -1.0 && y < (double)a.cam_h) {
      const double xf = floor(x), yf = floor(y);
      const double fx = x - xf, fy = y - yf;
      const int x0 = (int)xf, y0 = (int)yf;
      double den = 0.0, num = 0.0;
      tcal_tap(a, x0, y0, (1.0 - fx) * (1.0 - fy), den, num);
      tcal_tap(a, x0 + 1, y0, fx * (1.0 - fy), den, num);
      tcal_tap(a, x0, y0 + 1, (1.0 - fx) * fy, den, num);
      tcal_tap(a, x0 + 1, y0 + 1, fx * fy, den, num);
      if (den > 0.0) present = true, val = num / den;
    }
    a.value[i] = val;
    a.present[i] = present ? 1 : 0;
  }
  const u32 n_missing = (u32)__popcll(__ballot(i < n_px && !present));
  if ((threadIdx.x & 63) == 0 && n_missing) __hip_atomic_fetch_add(&a.acc->n_missing, n_missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// T5 ------------------------------------------------------------------------------------------------------------------------
constexpr int TCAL_NONE_R = 0x7fffffff;  // no present column to the right; to the left: -1

// inclusive scans over the block's BLOCK values in thread order, `carry` in front of (behind) them: wave scan, then the other
// waves' totals through LDS.  Every thread returns with the block's total folded into `carry`.
__device__ inline int tcal_scan_max_fwd(int v, int& carry, int* s_w) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= (u32)o) v = up > v ? up : v;
  }
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  int before = carry, total = carry;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; ++w) {
    const int t = s_w[w];
    before = ((u32)w < wave && t > before) ? t : before;
    total = t > total ? t : total;
  }
  __syncthreads();  // (s_w is written again by the next chunk)
  carry = total;
  return before > v ? before : v;
}
__device__ inline int tcal_scan_min_bwd(int v, int& carry, int* s_w) {
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int dn = __shfl_down(v, o, 64);
    if (lane + (u32)o < 64u) v = dn < v ? dn : v;
  }
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  int after = carry, total = carry;
#pragma unroll
  for (int w = 0; w < BLOCK / 64; ++w) {
    const int t = s_w[w];
    after = ((u32)w > wave && t < after) ? t : after;
    total = t < total ? t : total;
  }
  __syncthreads();
  carry = total;
  return after < v ? after : v;
}

// grid = proj_h blocks.  next_r: [proj_h][proj_w] scratch (a thread reads back only what it stored itself)
__global__ __launch_bounds__(BLOCK) void k_tcal_fill(const double* __restrict__ value, const uint8_t* __restrict__ present, int proj_w,
                                                      int* __restrict__ next_r, float* __restrict__ out, TcalAcc* __restrict__ acc) {
  __shared__ int s_w[BLOCK / 64];
  const size_t row = (size_t)blockIdx.x * (size_t)proj_w;
  const int n_chunks = (proj_w + BLOCK - 1) / BLOCK;
  int carry = TCAL_NONE_R;
  for (int c = n_chunks - 1; c >= 0; --c) {  // the next present column at or behind u
    const int u = c * BLOCK + (int)threadIdx.x;
    const int v = (u < proj_w && present[row + u]) ? u : TCAL_NONE_R;
    const int r = tcal_scan_min_bwd(v, carry, s_w);
    if (u < proj_w) next_r[row + u] = r;
  }
  carry = -1;
  for (int c = 0; c < n_chunks; ++c) {  // the previous present column at or in front of u
    const int u = c * BLOCK + (int)threadIdx.x;
    const bool p = u < proj_w && present[row + u];
    const int l = tcal_scan_max_fwd(p ? u : -1, carry, s_w);
    if (u >= proj_w) continue;  // (after the scan's barriers)
    double val = 0.0;
    if (p) {
      val = value[row + u];
    } else {
      const int r = next_r[row + u];
      if (l >= 0 && r != TCAL_NONE_R) {
        const double ml = value[row + l], mr = value[row + r];
        val = ml + (mr - ml) * ((double)(u - l) / (double)(r - l));
      } else if (l >= 0) {
        val = value[row + l];
      } else if (r != TCAL_NONE_R) {
        val = value[row + r];
      }
    }
    out[row + u] = (float)val;
  }
  if (threadIdx.x == 0 && carry < 0) __hip_atomic_fetch_add(&acc->n_unfilled, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace xm
