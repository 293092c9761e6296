// xmaps_surface.hpp -- gfx950 device code of the time-surface entry (xm_process_time_surfaces): a GROUP of camera time surfaces
// (f32 / f64 images, 0 = no event; python/eval/compute_depth_x_maps.py:79-131 of the reference) -> depth maps and per-event point
// clouds, everything in between on the device.
//
// A time surface holds at most one event per camera pixel, and in camera view that event's frame cell is its own pixel
// (cam_proj_calibration.py:312-317): there is nothing to resolve, so this path has no key frame, no atomics and no clear.  Per group
// (grid = surfaces x blocks everywhere):
//   S0 k_surf_extrema       lo / hi over the non-zero entries + their count                         -> one partial per block
//   S1 k_surf_norm_extrema  v' = max((f64(v) - lo) / (hi - lo), 0) as eval_depth.time_surface_to_events computes it;
//                           (tmin, tmax) = extrema of the v' > 0 (the events) + their count         -> one partial per block
//   S2 k_surf_pixels        per pixel: v' -> A1 (packed LUT) -> A2 (TimeNorm<double> + event_disparity_col: the code K1 runs)
//                           -> A5 (disparity -> depth table) -> ONE plain store of depth[y][x]; inliers per 64-pixel row segment
//   S3 k_surf_scan          one block per surface: exclusive scan of the segment counts (raster order) + the surface's statistics
//   S4 k_surf_cloud         (clouds only) stable compaction in raster order = the order of xr_f[mask]: ballot + mbcnt inside the
//                           segment, the scanned offset in front; gather of the float rectify maps; Q in k_point_cloud's arithmetic
// No block ever waits for another block: every cross-block dependency is a kernel boundary (partials are re-reduced by the waves
// that need them; offsets come from the scan launch).  Nothing here spins on a flag.
//
// Arithmetic: the surface is widened to float64 BEFORE it is normalised, whatever the file's dtype -- that is what
// time_surface_to_events does and what golden G7 pins (the reference normalises float32 files in float32: last-bit differences of
// t are an existing property of this build, not of this path).  NaN / +-inf entries are out of contract: they never become extrema
// (comparisons with NaN are false) and an event's column is bounds-checked like K1's, so they cannot index outside a table.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_stage.hpp"  // Mat4f, point_from_disparity

namespace xm {

constexpr int SURF_RED_ITEMS = 8;                       // pixels per thread of the two reduction passes (independent loads in flight)
constexpr int SURF_RED_CHUNK = BLOCK * SURF_RED_ITEMS;  // pixels per block
// S2's tile: 64 pixels of a row per wave instruction (coalesced surface loads and depth stores), 16 rows per block -- the packed
// LUT is column-major ([cam_w][cam_h]: a lane's entries for consecutive rows share a 128-byte line), so a tile fetches each of its
// 64 LUT lines once and serves the other rows from L1
constexpr int SURF_TW = 64, SURF_TR = 16, SURF_ROWS_PER_WAVE = SURF_TR / (BLOCK / 64);
constexpr int SURF_SCAN_BLOCK = 1024;

struct SurfPart1 {  // S0, per block
  double lo, hi;
  u64 nnz, pad;
};
struct SurfPart2 {  // S1, per block (lo / hi / nnz: the surface's, the same in all of its entries)
  double tmin, tmax, lo, hi;
  u64 nev, nnz, pad[2];
};
struct SurfStats {  // == xm_surface_stats (include/xmaps.h)
  u64 n_nonzero, n_events, n_inliers, n_index_errors;
  double lo, hi, t_min, t_max;
};

// {min, max, count} of a block (BLOCK threads): valid in thread 0
__device__ inline void surf_block_reduce(double& mn, double& mx, u32& cnt) {
  __shared__ double s_mn[BLOCK / 64], s_mx[BLOCK / 64];
  __shared__ u32 s_c[BLOCK / 64];
  mn = wave_min_f64(mn);
  mx = wave_max_f64(mx);
  cnt = wave_sum_u32(cnt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_mn[wave] = mn, s_mx[wave] = mx, s_c[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = s_mx[w] > mx ? s_mx[w] : mx;
      cnt += s_c[w];
    }
  }
}

// eval_depth.time_surface_to_events: (f64(v) - lo) / (hi - lo), negatives to 0 (IEEE divide; built with -ffp-contract=off)
template <typename T> __device__ inline double surf_norm(T v, double lo, double den) {
  const double vn = ((double)v - lo) / den;
  return vn < 0.0 ? 0.0 : vn;
}
// a surface has events only if it has two distinct non-zero values (all-zero: lo = +inf; one value: hi == lo)
__device__ inline bool surf_normalisable(double lo, double hi, u64 nnz) { return nnz != 0 && hi > lo; }

// S0 ------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_surf_extrema(const T* __restrict__ surf, u32 n_px, SurfPart1* __restrict__ part) {
  const T* img = surf + (size_t)blockIdx.y * n_px;
  const u32 base = blockIdx.x * (u32)SURF_RED_CHUNK + threadIdx.x;
  T v[SURF_RED_ITEMS];
#pragma unroll
  for (int k = 0; k < SURF_RED_ITEMS; ++k) {
    const u32 i = base + (u32)k * BLOCK;
    v[k] = i < n_px ? img[i] : (T)0;
  }
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0;
#pragma unroll
  for (int k = 0; k < SURF_RED_ITEMS; ++k) {
    const double d = (double)v[k];
    if (d != 0.0) {
      nnz += 1;
      lo = d < lo ? d : lo;
      hi = d > hi ? d : hi;
    }
  }
  surf_block_reduce(lo, hi, nnz);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = SurfPart1{lo, hi, nnz, 0};
}

// S1 ------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_surf_norm_extrema(const T* __restrict__ surf, u32 n_px, const SurfPart1* __restrict__ part1,
                                                              SurfPart2* __restrict__ part2) {
  const u32 nb = gridDim.x, lane = threadIdx.x & 63;
  const SurfPart1* p1 = part1 + (size_t)blockIdx.y * nb;
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0;
  for (u32 i = lane; i < nb; i += 64) {  // every wave reduces the surface's S0 partials itself (a few KB, L2-hot)
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
  const T* img = surf + (size_t)blockIdx.y * n_px;
  const u32 base = blockIdx.x * (u32)SURF_RED_CHUNK + threadIdx.x;
  T v[SURF_RED_ITEMS];
#pragma unroll
  for (int k = 0; k < SURF_RED_ITEMS; ++k) {
    const u32 i = base + (u32)k * BLOCK;
    v[k] = i < n_px ? img[i] : (T)0;
  }
  double tmin = INFINITY, tmax = -INFINITY;
  u32 nev = 0;
  if (valid) {
#pragma unroll
    for (int k = 0; k < SURF_RED_ITEMS; ++k) {
      const double vn = surf_norm(v[k], lo, den);
      if (base + (u32)k * BLOCK < n_px && vn > 0.0) {
        nev += 1;
        tmin = vn < tmin ? vn : tmin;
        tmax = vn > tmax ? vn : tmax;
      }
    }
  }
  surf_block_reduce(tmin, tmax, nev);
  if (threadIdx.x == 0)
    part2[(size_t)blockIdx.y * nb + blockIdx.x] = SurfPart2{tmin, tmax, nnz ? lo : 0.0, nnz ? hi : 0.0, nev, nnz, {0, 0}};
}

// the surface's (tmin, tmax, events) out of its S1 partials: every wave for itself, wave-uniform result
__device__ inline void surf_load_part2(const SurfPart2* __restrict__ p2, u32 nb, double& tmin, double& tmax, u32& nev) {
  const u32 lane = threadIdx.x & 63;
  tmin = INFINITY, tmax = -INFINITY, nev = 0;
  for (u32 i = lane; i < nb; i += 64) {
    const double a = p2[i].tmin, b = p2[i].tmax;
    tmin = a < tmin ? a : tmin;
    tmax = b > tmax ? b : tmax;
    nev += (u32)p2[i].nev;
  }
  tmin = wave_min_f64(tmin);
  tmax = wave_max_f64(tmax);
  nev = wave_sum_u32(nev);
}

// S2 ------------------------------------------------------------------------------------------------------------------------
// grid = (tiles_x, tiles_y, surfaces).  code (CLOUD): u16 per pixel, disparity + 1 of an inlier, else 0 -- what S4 compacts.
// seg_cnt[surface][y][tile_x]: inliers of the 64-pixel row segment (raster order of the segments = raster order of the pixels).
template <typename T, bool CLOUD>
__global__ __launch_bounds__(BLOCK) void k_surf_pixels(const T* __restrict__ surf, DevTables tb, const SurfPart2* __restrict__ part2,
                                                        u32 nb_red, float* __restrict__ depth, uint16_t* __restrict__ code,
                                                        u32* __restrict__ seg_cnt, u32* __restrict__ wave_oob) {
  const u32 s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SurfPart2* p2 = part2 + (size_t)s * nb_red;
  double tmin, tmax;
  u32 nev;
  surf_load_part2(p2, nb_red, tmin, tmax, nev);
  const double lo = p2[0].lo, den = p2[0].hi - p2[0].lo;
  const bool valid = nev != 0;  // (implies a normalisable surface)
  const TimeNorm<double> tn(tmin, tmax, tb.t_px_scale);
  const u32 n_px = (u32)tb.cam_w * (u32)tb.cam_h;
  const size_t img0 = (size_t)s * n_px;
  const u32 x = blockIdx.x * SURF_TW + lane, y0 = blockIdx.y * SURF_TR + wave * SURF_ROWS_PER_WAVE;
  const bool x_in = x < (u32)tb.cam_w;
  T v[SURF_ROWS_PER_WAVE];
#pragma unroll
  for (int r = 0; r < SURF_ROWS_PER_WAVE; ++r) {
    const u32 y = y0 + r;
    v[r] = x_in && y < (u32)tb.cam_h ? surf[img0 + (size_t)y * tb.cam_w + x] : (T)0;
  }
  u32 n_oob = 0;
#pragma unroll
  for (int r = 0; r < SURF_ROWS_PER_WAVE; ++r) {
    const u32 y = y0 + r;
    if (y >= (u32)tb.cam_h) break;  // wave-uniform
    bool inl = false, oob = false;
    int dsp = 0;
    if (x_in && valid) {
      const double vn = surf_norm(v[r], lo, den);
      if (vn > 0.0) {  // an event: the pixel is its own (x, y), vn its time stamp
        const EventResult e = event_disparity_col(tb, tn.column(vn), x, y, oob);
        inl = e.inlier;
        dsp = e.disp;
      }
    }
    const u64 bal = __ballot(inl);
    n_oob += (u32)__popcll(__ballot(oob));
    if (x_in) {
      const size_t px = img0 + (size_t)y * tb.cam_w + x;
      depth[px] = inl ? __uint_as_float(tb.dlut[dsp & 0xffff].x) : 0.0f;
      if constexpr (CLOUD) code[px] = inl ? (uint16_t)(dsp + 1) : (uint16_t)0;
    }
    if (lane == 0) seg_cnt[((size_t)s * tb.cam_h + y) * gridDim.x + blockIdx.x] = (u32)__popcll(bal);
  }
  if (lane == 0) {
    const u32 blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    wave_oob[(size_t)blk * (BLOCK / 64) + wave] = n_oob;
  }
}

// S3 ------------------------------------------------------------------------------------------------------------------------
// one block per surface: seg_off = exclusive scan of seg_cnt (n_seg entries), the surface's statistics
__global__ __launch_bounds__(SURF_SCAN_BLOCK) void k_surf_scan(const u32* __restrict__ seg_cnt, u32 n_seg, const u32* __restrict__ wave_oob,
                                                                u32 n_wo, const SurfPart2* __restrict__ part2, u32 nb_red,
                                                                u32* __restrict__ seg_off, SurfStats* __restrict__ stats) {
  __shared__ u32 s_w[SURF_SCAN_BLOCK / 64], s_oob[SURF_SCAN_BLOCK / 64];
  const u32 s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32* cnt = seg_cnt + (size_t)s * n_seg;
  u32* off = seg_off + (size_t)s * n_seg;
  const u32 ipt = (n_seg + SURF_SCAN_BLOCK - 1) / SURF_SCAN_BLOCK;  // consecutive segments per thread
  const u32 first = tid * ipt, last = first + ipt < n_seg ? first + ipt : n_seg;
  u32 sum = 0;
  for (u32 i = first; i < last; ++i) sum += cnt[i];
  u32 incl = sum;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 up = __shfl_up(incl, o, 64);
    if (lane >= (u32)o) incl += up;
  }
  u32 oob = 0;
  for (u32 i = tid; i < n_wo; i += SURF_SCAN_BLOCK) oob += wave_oob[(size_t)s * n_wo + i];
  oob = wave_sum_u32(oob);
  if (lane == 63) s_w[wave] = incl;
  if (lane == 0) s_oob[wave] = oob;
  __syncthreads();
  u32 before = 0, total = 0, oob_total = 0;
#pragma unroll
  for (int w = 0; w < SURF_SCAN_BLOCK / 64; ++w) {
    before += (u32)w < wave ? s_w[w] : 0u;
    total += s_w[w];
    oob_total += s_oob[w];
  }
  u32 run = before + incl - sum;
  for (u32 i = first; i < last; ++i) {
    off[i] = run;
    run += cnt[i];
  }
  if (wave == 0) {
    const SurfPart2* p2 = part2 + (size_t)s * nb_red;
    double tmin, tmax;
    u32 nev;
    surf_load_part2(p2, nb_red, tmin, tmax, nev);
    if (lane == 0)
      stats[s] = SurfStats{p2[0].nnz, nev, total, oob_total, p2[0].lo, p2[0].hi, nev ? tmin : 0.0, nev ? tmax : 0.0};
  }
}

// S4 ------------------------------------------------------------------------------------------------------------------------
// one wave per 64-pixel row segment; cloud: f32 [surfaces][cam_h * cam_w][3], the first n_inliers rows of a surface valid
__global__ __launch_bounds__(BLOCK) void k_surf_cloud(const uint16_t* __restrict__ code, const u32* __restrict__ seg_off, int cam_w,
                                                       int cam_h, u32 tiles_x, const float* __restrict__ mapx,
                                                       const float* __restrict__ mapy, Mat4f Q, float* __restrict__ cloud) {
  const u32 s = blockIdx.y, lane = threadIdx.x & 63, n_seg = (u32)cam_h * tiles_x;
  const u32 seg = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if (seg >= n_seg) return;
  const u32 y = seg / tiles_x, x = (seg - y * tiles_x) * SURF_TW + lane, n_px = (u32)cam_w * (u32)cam_h;
  const u32 px = y * (u32)cam_w + x;
  const u32 c = x < (u32)cam_w ? (u32)code[(size_t)s * n_px + px] : 0u;
  const u64 bal = __ballot(c != 0);
  if (c == 0) return;
  const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
  const u32 row = seg_off[(size_t)s * n_seg + seg] + rank;  // < n_px: a surface has at most one inlier per pixel
  float p[3];
  point_from_disparity(Q, mapx[px], mapy[px], (float)(int)(c - 1u), p);
  float* out = cloud + ((size_t)s * n_px + row) * 3;
  out[0] = p[0];
  out[1] = p[1];
  out[2] = p[2];
}

}  // namespace xm
