// xmaps_evaltable.hpp -- gfx950 device code of the evaluation table's scorer (xm_eval_table_*): what turns the depth maps of a
// sequence -- the ground truth and every method's estimates, scan by scan -- into the cells of the reference's Table 1
// (python/eval/create_evaluation_table.py:14-62,121-163 with esl_utilities.py:153-175 combine_mc3d).  The contract is written
// out in include/xmaps.h at xm_eval_table; x_maps_amd/eval_table.py and tests/eval_ref.py state the same arithmetic in NumPy.
//
// A call is a FIXED schedule of launches, nothing is read back in between:
//   k_evt_combine  grid (tiles, stacks): per pixel the mean over a stack's scans of the depths inside (min_d, max_d), scans in index
//                  order, float32.  Stack 0 is the ground truth, the others the methods that have a "1 sec" row
//   k_evt_median   grid (tiles_x, tiles_y, stacks): the 3 x 3 median of that mean, borders replicated; per block a partial of
//                  sum(comb[comb > 0]) and its count, for avg_depth.  Stack 0's map is the mask
//   k_evt_pass1    grid (tiles, scans): g = load_and_filter(gt[s], mask); per block a partial of sum(g[g > 0]), #(g > 0), #(g == 0)
//   k_evt_pass2    grid (tiles, scans): every block folds its scan's pass-1 partials into the margin, keeps its tile of g in
//                  registers and walks the rows: e = load_and_filter(est[m][s], mask), or the 1-sec map as it is; k_eval_stats'
//                  element-wise arithmetic; per block and row a partial of the squared-error sum and five counts
//   k_evt_fold     grid (rows * scans): a cell's partials -> its xm_eval_sums
//   k_evt_avg      grid (stacks): the median's partials -> avg_depth
// The streams are cut into flat tiles of EVT_TILE pixels; a tile is the unit of every partial, and a total is the partials folded
// in tile-index order (eslf_fold: thread t takes t, t + BLOCK, ..., then the xor butterfly of a wave, then the waves in order).
// Inside a tile thread t owns quads t, t + BLOCK, ... (four consecutive pixels each) and adds its pixels in index order, whether
// the quads come as 16-byte loads (VEC: the map's pixel count is a multiple of four and every pointer 16-byte aligned) or as
// four scalar loads.  So a cell's bits depend on the maps alone: not on the grid, the run, the alignment of a caller's pointer or
// the other methods in the call.  No atomics; no block waits for another; every cross-block dependency is a kernel boundary.
//
// Arithmetic (built with -ffp-contract=off, no fast-math): combine_mc3d's d = v; if (d >= max_d) d = 0; if (d <= min_d) d = 0;
// acc += d; cnt += d > 0 with float32 bounds; mean = cnt == 0 ? 0 : acc / cnt, the float64 quotient rounded once more, which is
// the correctly rounded float32 quotient.  A NaN depth follows from these comparisons: acc turns NaN and cnt is untouched.  The
// median is the exact rank-4 value of the nine; a NaN in the window is unspecified.
//
// Needs xmaps_eval.hpp (EvalAcc, eval_filtered) and xmaps_eslfilter.hpp (eslf_block_sum, eslf_fold).
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_eval.hpp"
#include "xmaps_eslfilter.hpp"

namespace xm {

struct EvtStacks {  // the stacks k_evt_combine reads: [n_maps][px] each
  const float* p[EVT_MAX_STACKS];
};
struct EvtRows {  // the rows k_evt_pass2 walks
  const float* est[EVT_MAX_ROWS];  // a method's [scans][px], or a 1-sec row's one [px] map
  u32 n_rows, one_sec;             // bit r of one_sec: row r is a 1-sec row (unfiltered, the same map for every scan)
};
constexpr int EVT_P1_CNT = 2, EVT_P2_CNT = 5;  // counts per pass-1 partial (n_gt_pos, n_gt_zero) and per pass-2 partial (n_close, n_valid, n1, n5, n10)

// quad q of a map of n pixels, starting at pixel i: beyond n come zeros (the callers skip them by index)
template <bool VEC>
__device__ inline void evt_load4(const float* __restrict__ p, size_t i, size_t n, float v[4]) {
  if (VEC) {
    const float4 q = i < n ? *reinterpret_cast<const float4*>(p + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i + k < n ? p[i + k] : 0.0f;
  }
}
template <bool VEC>
__device__ inline void evt_store4(float* __restrict__ p, size_t i, size_t n, const float v[4]) {
  if (VEC) {
    if (i < n) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < n) p[i + k] = v[k];
  }
}
// the first pixel of thread's quad j in its block's tile
__device__ inline size_t evt_quad(int j) { return (size_t)blockIdx.x * EVT_TILE + ((size_t)j * BLOCK + threadIdx.x) * 4; }

// counts in the order of eslf_block_sum (integers: any order gives the same sum; one shape for both)
__device__ inline u64 evt_block_count(u64 v, u64* s_cnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 t = s_cnt[0];
#pragma unroll
  for (int w = 1; w < BLOCK / 64; ++w) t += s_cnt[w];
  __syncthreads();
  return t;
}
__device__ inline u64 evt_fold_count(const u32* part, int n_tiles, u64* s_cnt) {
  u64 a = 0;
  for (int i = threadIdx.x; i < n_tiles; i += BLOCK) a += part[i];
  return evt_block_count(a, s_cnt);
}

// ---- combine -------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_evt_combine(EvtStacks st, u32 n_maps, size_t px, float min_d, float max_d,
                                                       float* __restrict__ mean) {
  const float* __restrict__ in = st.p[blockIdx.y];
  float acc[EVT_UN][4], cnt[EVT_UN][4];
#pragma unroll
  for (int j = 0; j < EVT_UN; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.0f, cnt[j][k] = 0.0f;
  for (u32 s = 0; s < n_maps; ++s) {
    const float* __restrict__ img = in + (size_t)s * px;
#pragma unroll
    for (int j = 0; j < EVT_UN; ++j) {
      float v[4];
      evt_load4<VEC>(img, evt_quad(j), px, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float d = v[k];
        if (d >= max_d) d = 0.0f;
        if (d <= min_d) d = 0.0f;
        acc[j][k] = acc[j][k] + d;
        cnt[j][k] = cnt[j][k] + (d > 0.0f ? 1.0f : 0.0f);  // (a float32 count, as the reference's: exact up to 2^24 maps)
      }
    }
  }
#pragma unroll
  for (int j = 0; j < EVT_UN; ++j) {
    float m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = cnt[j][k] == 0.0f ? 0.0f : (float)((double)acc[j][k] / (double)cnt[j][k]);
    evt_store4<VEC>(mean + (size_t)blockIdx.y * px, evt_quad(j), px, m);
  }
}

// ---- median ----------------------------------------------------------------------------------------------------------------------
__device__ inline void evt_sort2(float& a, float& b) {
  const float lo = b < a ? b : a, hi = b < a ? a : b;
  a = lo, b = hi;
}
// the median of nine: the 19-exchange network (Paeth / Smith); v[4] ends as the rank-4 value
__device__ inline float evt_median9(float v[9]) {
  evt_sort2(v[1], v[2]), evt_sort2(v[4], v[5]), evt_sort2(v[7], v[8]);
  evt_sort2(v[0], v[1]), evt_sort2(v[3], v[4]), evt_sort2(v[6], v[7]);
  evt_sort2(v[1], v[2]), evt_sort2(v[4], v[5]), evt_sort2(v[7], v[8]);
  evt_sort2(v[0], v[3]), evt_sort2(v[5], v[8]), evt_sort2(v[4], v[7]);
  evt_sort2(v[3], v[6]), evt_sort2(v[1], v[4]), evt_sort2(v[2], v[5]);
  evt_sort2(v[4], v[7]), evt_sort2(v[4], v[2]), evt_sort2(v[6], v[4]);
  evt_sort2(v[4], v[2]);
  return v[4];
}

// comb0: stack 0's map (the mask; may be the caller's); comb_rest: [stacks - 1][px]
__global__ __launch_bounds__(BLOCK) void k_evt_median(const float* __restrict__ mean, int W, int H, float* __restrict__ comb0,
                                                      float* __restrict__ comb_rest, double* __restrict__ msum, u32* __restrict__ mcnt) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ u64 s_cnt[BLOCK / 64];
  const u32 g = blockIdx.z;
  const size_t px = (size_t)W * H;
  const float* __restrict__ img = mean + g * px;
  float* __restrict__ out = g == 0 ? comb0 : comb_rest + (size_t)(g - 1) * px;
  const int x = (int)blockIdx.x * EVT_MW + (int)threadIdx.x % EVT_MW, y = (int)blockIdx.y * EVT_MH + (int)threadIdx.x / EVT_MW;
  double s = 0.0;
  u64 c = 0;
  if (x < W && y < H) {
    float v[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        int yy = y + dy, xx = x + dx;
        yy = yy < 0 ? 0 : yy > H - 1 ? H - 1 : yy;
        xx = xx < 0 ? 0 : xx > W - 1 ? W - 1 : xx;
        v[(dy + 1) * 3 + dx + 1] = img[(size_t)yy * W + xx];
      }
    const float m = evt_median9(v);
    out[(size_t)y * W + x] = m;
    if (m > 0.0f) s = (double)m, c = 1;
  }
  const size_t tile = (size_t)g * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const double ts = eslf_block_sum(s, s_red);
  const u64 tc = evt_block_count(c, s_cnt);
  if (threadIdx.x == 0) msum[tile] = ts, mcnt[tile] = (u32)tc;
}

__global__ __launch_bounds__(BLOCK) void k_evt_avg(const double* __restrict__ msum, const u32* __restrict__ mcnt, int n_mt,
                                                   double* __restrict__ avg) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ u64 s_cnt[BLOCK / 64];
  const u32 g = blockIdx.x;
  const double s = eslf_fold(msum + (size_t)g * n_mt, n_mt, s_red);
  const u64 c = evt_fold_count(mcnt + (size_t)g * n_mt, n_mt, s_cnt);
  if (threadIdx.x == 0) avg[g] = s / (double)(c ? c : 1);  // (no positive pixel: 0, as eval_table.combine_depth_maps)
}

// ---- score -----------------------------------------------------------------------------------------------------------------------
// p1_sum [scans][n_tiles], p1_cnt [scans][EVT_P1_CNT][n_tiles]
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_evt_pass1(const float* __restrict__ gt, const float* __restrict__ mask, size_t px, float min_d,
                                                     float max_d, double* __restrict__ p1_sum, u32* __restrict__ p1_cnt) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ u64 s_cnt[BLOCK / 64];
  const u32 s = blockIdx.y, n_tiles = gridDim.x;
  const float* __restrict__ img = gt + (size_t)s * px;
  double sum = 0.0;
  u64 pos = 0, zero = 0;
#pragma unroll
  for (int j = 0; j < EVT_UN; ++j) {
    const size_t i = evt_quad(j);
    float v[4], m[4];
    evt_load4<VEC>(img, i, px, v);
    evt_load4<VEC>(mask, i, px, m);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < px) {
        const float g = eval_filtered(v[k], m[k], 1, min_d, max_d);
        if (g > 0.0f) sum += (double)g, pos += 1;
        zero += g == 0.0f;
      }
  }
  const double ts = eslf_block_sum(sum, s_red);
  const u64 tp = evt_block_count(pos, s_cnt), tz = evt_block_count(zero, s_cnt);
  if (threadIdx.x == 0) {
    p1_sum[(size_t)s * n_tiles + blockIdx.x] = ts;
    p1_cnt[((size_t)s * EVT_P1_CNT + 0) * n_tiles + blockIdx.x] = (u32)tp;
    p1_cnt[((size_t)s * EVT_P1_CNT + 1) * n_tiles + blockIdx.x] = (u32)tz;
  }
}

// p2_sum [rows][scans][n_tiles], p2_cnt [rows][scans][EVT_P2_CNT][n_tiles]
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_evt_pass2(const float* __restrict__ gt, const float* __restrict__ mask, EvtRows rows, size_t px,
                                                     float min_d, float max_d, const double* __restrict__ p1_sum,
                                                     const u32* __restrict__ p1_cnt, double* __restrict__ p2_sum, u32* __restrict__ p2_cnt) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ u64 s_cnt[BLOCK / 64];
  __shared__ double w_sum[EVT_MAX_ROWS][BLOCK / 64];
  __shared__ u32 w_cnt[EVT_MAX_ROWS][BLOCK / 64][EVT_P2_CNT];
  const u32 s = blockIdx.y, n_scans = gridDim.y, n_tiles = gridDim.x;
  // the scan's margin, as k_eval_stats takes it: NaN when no g > 0, like NumPy's 0 / 0
  const double sum_gt = eslf_fold(p1_sum + (size_t)s * n_tiles, (int)n_tiles, s_red);
  const u64 n_gt_pos = evt_fold_count(p1_cnt + ((size_t)s * EVT_P1_CNT + 0) * n_tiles, (int)n_tiles, s_cnt);
  const double margin = 0.01 * sum_gt / (double)n_gt_pos;
  float g[EVT_UN][4], m[EVT_UN][4];
#pragma unroll
  for (int j = 0; j < EVT_UN; ++j) {
    float v[4];
    evt_load4<VEC>(gt + (size_t)s * px, evt_quad(j), px, v);
    evt_load4<VEC>(mask, evt_quad(j), px, m[j]);
#pragma unroll
    for (int k = 0; k < 4; ++k) g[j][k] = eval_filtered(v[k], m[j][k], 1, min_d, max_d);
  }
  for (u32 r = 0; r < rows.n_rows; ++r) {
    const bool one_sec = (rows.one_sec >> r) & 1u;  // (block-uniform)
    const float* __restrict__ est = rows.est[r] + (one_sec ? 0 : (size_t)s * px);
    double sq = 0.0;
    u32 c[EVT_P2_CNT] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < EVT_UN; ++j) {
      const size_t i = evt_quad(j);
      float v[4];
      evt_load4<VEC>(est, i, px, v);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < px) {
          const float gg = g[j][k];
          const float e = eval_filtered(v[k], m[j][k], one_sec ? 0 : 1, min_d, max_d);
          const float d = gg - e;
          const float a = gg == 0.0f ? 0.0f : fabsf(d);
          c[0] += (double)a < margin;
          if (gg > 0.0f && e > 0.0f) {
            c[1] += 1;
            sq += (double)(d * d);  // pow(gt - est, 2) on f32 arrays is an f32 product
          }
          c[2] += a > 1.0f;
          c[3] += a > 5.0f;
          c[4] += a > 10.0f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sq += __shfl_xor(sq, o, 64);
#pragma unroll
      for (int k = 0; k < EVT_P2_CNT; ++k) c[k] += __shfl_xor(c[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      w_sum[r][threadIdx.x >> 6] = sq;
#pragma unroll
      for (int k = 0; k < EVT_P2_CNT; ++k) w_cnt[r][threadIdx.x >> 6][k] = c[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < rows.n_rows) {  // thread r: row r's waves in order
    const u32 r = threadIdx.x;
    const size_t cell = (size_t)r * n_scans + s;
    double t = w_sum[r][0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) t += w_sum[r][w];
    p2_sum[cell * n_tiles + blockIdx.x] = t;
#pragma unroll
    for (int k = 0; k < EVT_P2_CNT; ++k) {
      u32 n = 0;
#pragma unroll
      for (int w = 0; w < BLOCK / 64; ++w) n += w_cnt[r][w][k];
      p2_cnt[(cell * EVT_P2_CNT + k) * n_tiles + blockIdx.x] = n;
    }
  }
}

// sums [rows][scans]
__global__ __launch_bounds__(BLOCK) void k_evt_fold(const double* __restrict__ p1_sum, const u32* __restrict__ p1_cnt,
                                                    const double* __restrict__ p2_sum, const u32* __restrict__ p2_cnt, u32 n_scans,
                                                    int n_tiles, EvalAcc* __restrict__ sums) {
  __shared__ double s_red[BLOCK / 64];
  __shared__ u64 s_cnt[BLOCK / 64];
  const size_t cell = blockIdx.x, s = cell % n_scans;
  EvalAcc a;
  a.sum_gt = eslf_fold(p1_sum + s * n_tiles, n_tiles, s_red);
  a.sum_sq = eslf_fold(p2_sum + cell * n_tiles, n_tiles, s_red);
  a.n_gt_pos = evt_fold_count(p1_cnt + (s * EVT_P1_CNT + 0) * n_tiles, n_tiles, s_cnt);
  a.n_gt_zero = evt_fold_count(p1_cnt + (s * EVT_P1_CNT + 1) * n_tiles, n_tiles, s_cnt);
  const u32* c = p2_cnt + cell * EVT_P2_CNT * n_tiles;
  a.n_close = evt_fold_count(c, n_tiles, s_cnt);
  a.n_valid = evt_fold_count(c + (size_t)n_tiles, n_tiles, s_cnt);
  a.n1 = evt_fold_count(c + (size_t)2 * n_tiles, n_tiles, s_cnt);
  a.n5 = evt_fold_count(c + (size_t)3 * n_tiles, n_tiles, s_cnt);
  a.n10 = evt_fold_count(c + (size_t)4 * n_tiles, n_tiles, s_cnt);
  if (threadIdx.x == 0) sums[cell] = a;
}

}  // namespace xm
