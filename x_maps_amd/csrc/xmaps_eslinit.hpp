// xmaps_eslinit.hpp -- gfx950 device code of the ESL-init baseline (xm_esl_init_*): the disparity search the reference's evaluation
// runs beside X-maps (python/eval/compute_depth_esl.py:72-85 disparity_init, :204-226 its caller), on the device.
//
// Per rectified pixel (r, c) whose camera value e = cam_rect[r][c] is > 0: the window proj_rect[r][c + min_disp : c + max_disp]
// (clipped at the row's end, possibly empty); its NON-ZERO entries are the candidates; with more than one candidate the disparity is
// the offset of the FIRST minimum of cost = (f64(p) - e)^2 (np.argmin), otherwise 0.  Two kernels:
//   k_esl_stage  the whole rectified frame: cam_rect f64 + proj_rect f32 -> disparity u16 (disparity_init as a function).  A block
//                takes ESL_TX columns of one row and stages the part of the projector row its windows cover in LDS.
//   k_esl_fused  what the evaluation needs, per camera pixel of a GROUP of time surfaces: follow rect_to_cam_map to its one
//                rectified pixel, fetch that pixel's normalised camera value through cam_to_rect_map on the fly, search its window,
//                divide, ONE plain store of depth[y][x].  Only the rectified pixels the back map references are ever searched and no
//                rectified image exists.  lo / hi of a surface are k_surf_extrema's partials (xmaps_surface.hpp), re-reduced by every
//                wave; the searched / matched counts leave as one partial per block and k_esl_stats adds them up.
// No atomics, and no block waits for another: every cross-block dependency is a kernel boundary.
//
// Arithmetic (built with -ffp-contract=off): the surface is widened to float64 before it is normalised (surf_norm, the convention
// golden G7 pins); p is widened exactly, the subtraction and the product are each rounded once, comparisons are strict so the first
// minimum wins whatever ties, exact matches or underflowed squares the window holds.  NaN / +-inf surfaces are out of contract: e is
// only ever compared and subtracted, never an index, so they cannot reach outside a table.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_surface.hpp"  // SurfPart1, surf_norm, surf_normalisable, surf_block_reduce's wave helpers

namespace xm {

constexpr int ESL_TX = BLOCK;     // stage kernel: columns of one row per block
constexpr int ESL_CHUNK = 1024;   // ... window offsets staged per pass (one pass at the reference's 895)
constexpr int ESL_FW = 64, ESL_FR = BLOCK / 64;  // fused kernel: 64 camera pixels of a row per wave, one row per wave

struct EslTables {  // what k_esl_fused takes by value: views of the tables an xm_esl_init owns
  const short2* rect_to_cam;  // [cam_h][cam_w]   camera pixel -> (rx, ry): where its disparity lies in the rectified frame
  const short2* cam_to_rect;  // [rect_h][rect_w] rectified pixel -> (mx, my): where its value lies in the camera image
  const float* proj_rect;     // [rect_h][rect_w] rectified projector time surface, 0 = no data
  int cam_w, cam_h, rect_w, rect_h, min_disp, max_disp;
  double p1_03;
};
struct EslStats {  // == xm_esl_init_stats (include/xmaps.h)
  u64 n_nonzero, n_searched, n_matched;
  double lo, hi;
};

// the running first minimum of one window
struct EslBest {
  double cost = INFINITY;
  u32 k = 0, n = 0;  // offset of the winner inside the window, candidates so far
  __device__ inline void consider(float p, u32 at, double e) {
    if (p != 0.0f) {
      const double d = (double)p - e;
      const double c = d * d;
      if (n == 0 || c < cost) cost = c, k = at;
      n += 1;
    }
  }
  __device__ inline u32 disparity(int min_disp) const { return n > 1 ? (u32)min_disp + k : 0u; }
};

// walk nk consecutive window entries from `win` (global memory or LDS): eight loads in flight in front of the dependent compare chain
template <typename P> __device__ inline void esl_walk(EslBest& b, P win, u32 k0, u32 nk, double e) {
  u32 k = 0;
  for (; k + 8 <= nk; k += 8) {
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = win[k + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) b.consider(p[i], k0 + k + i, e);
  }
  for (; k < nk; ++k) b.consider(win[k], k0 + k, e);
}

// ---- the stage kernel: grid = (ceil(rect_w / ESL_TX), rect_h) -----------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_esl_stage(const double* __restrict__ cam_rect, const float* __restrict__ proj_rect,
                                                      int rect_w, int min_disp, int max_disp, uint16_t* __restrict__ disparity) {
  __shared__ float s_win[ESL_TX + ESL_CHUNK];
  const u32 c0 = blockIdx.x * ESL_TX, c = c0 + threadIdx.x, w = (u32)rect_w;
  const size_t row = (size_t)blockIdx.y * w;
  const double e = c < w ? cam_rect[row + c] : 0.0;
  const bool live = e > 0.0;
  if (!__syncthreads_or(live)) {  // no pixel of the tile is searched: its zeros and out
    if (c < w) disparity[row + c] = 0;
    return;
  }
  const u32 span = (u32)(max_disp - min_disp);  // window offsets 0 .. span - 1 <-> columns c + min_disp + k
  EslBest best;
  for (u32 k0 = 0; k0 < span; k0 += ESL_CHUNK) {
    const u32 nk = span - k0 < (u32)ESL_CHUNK ? span - k0 : (u32)ESL_CHUNK;
    // s_win[i] = proj_rect[r][c0 + min_disp + k0 + i]; beyond the row's end 0 -- never a candidate, which is what clipping does
    const u64 col0 = (u64)c0 + (u32)min_disp + k0;
    if (k0) __syncthreads();  // (the previous pass has been read)
    for (u32 i = threadIdx.x; i < (u32)ESL_TX + nk; i += BLOCK) s_win[i] = col0 + i < w ? proj_rect[row + col0 + i] : 0.0f;
    __syncthreads();
    if (live) esl_walk(best, (const float*)s_win + threadIdx.x, k0, nk, e);
  }
  if (c < w) disparity[row + c] = (uint16_t)(live ? best.disparity(min_disp) : 0u);
}

// ---- the fused kernel: grid = (ceil(cam_w / ESL_FW), ceil(cam_h / ESL_FR), surfaces) ------------------------------------------
// part1: k_surf_extrema's partials [surface][nb_red]; cnt: {searched, matched} per block, [surface][gridDim.y][gridDim.x]
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_esl_fused(const T* __restrict__ surf, EslTables tb, const SurfPart1* __restrict__ part1,
                                                      u32 nb_red, float* __restrict__ depth, uint16_t* __restrict__ disp_cam,
                                                      uint2* __restrict__ cnt) {
  __shared__ u32 s_cnt[2][BLOCK / 64];
  const u32 s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SurfPart1* p1 = part1 + (size_t)s * nb_red;
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0;
  for (u32 i = lane; i < nb_red; i += 64) {  // every wave reduces the surface's partials itself (a few KB, L2-hot)
    const SurfPart1 p = p1[i];
    lo = p.lo < lo ? p.lo : lo;
    hi = p.hi > hi ? p.hi : hi;
    nnz += (u32)p.nnz;
  }
  lo = wave_min_f64(lo);
  hi = wave_max_f64(hi);
  nnz = wave_sum_u32(nnz);
  const bool valid = surf_normalisable(lo, hi, nnz);
  const double den = hi - lo;
  const u32 x = blockIdx.x * ESL_FW + lane, y = blockIdx.y * ESL_FR + wave;
  const bool in = x < (u32)tb.cam_w && y < (u32)tb.cam_h;
  const size_t n_px = (size_t)tb.cam_w * tb.cam_h, px = (size_t)y * tb.cam_w + x;
  double e = 0.0;
  int rx = 0, ry = 0;
  if (in && valid) {
    const short2 r = tb.rect_to_cam[px];
    rx = r.x, ry = r.y;
    if ((u32)rx < (u32)tb.rect_w && (u32)ry < (u32)tb.rect_h) {  // else: border 0
      const short2 m = tb.cam_to_rect[(size_t)ry * tb.rect_w + rx];
      if ((u32)m.x < (u32)tb.cam_w && (u32)m.y < (u32)tb.cam_h)  // else: border 0
        e = surf_norm(surf[s * n_px + (size_t)m.y * tb.cam_w + m.x], lo, den);
    }
  }
  const bool live = e > 0.0;  // (implies rx, ry inside the rectified frame)
  u32 d = 0;
  if (live) {
    const int first = rx + tb.min_disp, end = rx + tb.max_disp < tb.rect_w ? rx + tb.max_disp : tb.rect_w;
    if (first < end) {
      EslBest best;
      esl_walk(best, tb.proj_rect + (size_t)ry * tb.rect_w + first, 0u, (u32)(end - first), e);
      d = best.disparity(tb.min_disp);
    }
  }
  if (in) {
    depth[s * n_px + px] = d ? (float)(tb.p1_03 / (double)d) : 0.0f;
    if (disp_cam) disp_cam[s * n_px + px] = (uint16_t)d;
  }
  const u32 n_live = (u32)__popcll(__ballot(live)), n_hit = (u32)__popcll(__ballot(d != 0));
  if (lane == 0) s_cnt[0][wave] = n_live, s_cnt[1][wave] = n_hit;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint2 c = make_uint2(0, 0);
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) c.x += s_cnt[0][w], c.y += s_cnt[1][w];
    cnt[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = c;
  }
}

// one block per surface: the surface's statistics out of the extrema partials and the fused kernel's per-block counts
__global__ __launch_bounds__(BLOCK) void k_esl_stats(const SurfPart1* __restrict__ part1, u32 nb_red, const uint2* __restrict__ cnt,
                                                      u32 n_cnt, EslStats* __restrict__ stats) {
  __shared__ u32 s_sum[2][BLOCK / 64];
  const u32 s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0, a = 0, b = 0;  // (each at most cam_w * cam_h < 2^32: the host checks)
  for (u32 i = threadIdx.x; i < nb_red; i += BLOCK) {
    const SurfPart1 p = part1[(size_t)s * nb_red + i];
    lo = p.lo < lo ? p.lo : lo;
    hi = p.hi > hi ? p.hi : hi;
    nnz += (u32)p.nnz;
  }
  for (u32 i = threadIdx.x; i < n_cnt; i += BLOCK) {
    const uint2 c = cnt[(size_t)s * n_cnt + i];
    a += c.x, b += c.y;
  }
  surf_block_reduce(lo, hi, nnz);  // (valid in thread 0; ends behind a barrier)
  a = wave_sum_u32(a);
  b = wave_sum_u32(b);
  if (lane == 0) s_sum[0][wave] = a, s_sum[1][wave] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 sa = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) sa += s_sum[0][w], sb += s_sum[1][w];
    stats[s] = EslStats{nnz, sa, sb, nnz ? lo : 0.0, nnz ? hi : 0.0};
  }
}

}  // namespace xm
