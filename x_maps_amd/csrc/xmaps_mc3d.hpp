// xmaps_mc3d.hpp -- gfx950 device code of the MC3D baseline (xm_mc3d_*): the per-pixel search of the reference's
// python/eval/mc3d_baseline.py:40-78 (compute_disparity) with the 3 x 3 median in front of it (:130) and the depth division behind
// it (:15-18, :139), for a GROUP of camera time surfaces in one launch.
//
// Per camera pixel (i, j): v = median of the 3 x 3 neighbourhood (replicate border, exact median of nine) or, with
// XM_MC3D_NO_BLUR, the pixel itself.  v > 0: (xc, yc) = cam_map[i][j], kept if 0 < xc < rect_x_limit and 0 < yc < rect_y_limit;
// id = int(W * H * v) -- the product in the surface's own type --, dropped if id >= W * H; proj_x = id / H, proj_y = id % H; over
// y in [max(proj_y - nc, 0), min(proj_y + nc, H)) the FIRST minimum of |yc - yp(y, proj_x)| wins, is accepted if <= max_row_diff,
// disp = xp(winner) - xc is stored if > 0.  A poisoned (NaN / +-inf) projector entry inside the window zeroes the pixel.
//
// The projector table is stored by (proj_x, y), so a window is ONE contiguous run of at most 2 * nc int32: yp_t for the search
// (poison of either component folded into it), xp_t read once at the winner.  A wave takes 64 pixels of a camera row; it then walks
// its lit pixels MC3D_GL lanes to a window (coalesced runs of MC3D_GL * 4 bytes), 64 / MC3D_GL windows at once, and reduces one 32-bit key
//   0 = poison | 1 + (min(cost, max_row_diff + 1) << pos_bits | position in the window)
// by min: the smallest cost, among equals the first position; a cost beyond max_row_diff is refused whatever its size, so the clamp
// changes no result (mc3d_key_fits: the host refuses tables whose key would not fit).  -DXM_MC3D_GL=8 / 16 / 32 / 64 sets the lanes
// per window and -DXM_MC3D_LANE_WALK builds the other shape, each lane walking its own pixel's window: profiles/mc3d.md compares them.
// One plain store of depth (and of the u16 disparity) per pixel; no atomics, no block waits for another: the counts leave as one
// partial per block and k_mc3d_stats adds them up.  Built with -ffp-contract=off; NaN surfaces are out of contract: v > 0 is false
// for NaN and id is only formed behind (product < W * H), so nothing can index outside a table.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

struct Mc3dTables {  // what k_mc3d takes by value: views of the tables an xm_mc3d owns
  const int2* cam_map;  // [cam_h][cam_w] camera pixel -> (xc, yc), truncated; MC3D_POISON fails 0 < xc by itself
  const int* yp_t;      // [proj_w][proj_h] yp by (proj_x, y); MC3D_POISON where either component of the entry is poisoned
  const int* xp_t;      // [proj_w][proj_h] xp by (proj_x, y)
  int cam_w, cam_h, proj_w, proj_h, nc, max_row_diff, rect_x_limit, rect_y_limit;
  u32 pos_bits;  // mc3d_pos_bits(2 * nc)
  double p1_03;
};
struct Mc3dStats {  // == xm_mc3d_stats (include/xmaps.h)
  u64 n[MC3D_N_CNT];
};
struct Mc3dCnt {  // one block's partial of the same counts
  u32 n[MC3D_N_CNT];
};
enum { MC3D_C_NONZERO, MC3D_C_POSITIVE, MC3D_C_IN_RECT, MC3D_C_OUT_OF_RANGE, MC3D_C_POISONED, MC3D_C_MATCHED, MC3D_C_DISP_OVERFLOW };

// exact median of nine: the 19-exchange selection network; every exchange picks, so the result is one of the inputs bit for bit
template <typename T> __host__ __device__ inline T mc3d_median9(T (&p)[9]) {
#define XM_MC3D_SORT2(a, b)                 \
  {                                         \
    const T lo_ = p[b] < p[a] ? p[b] : p[a]; \
    const T hi_ = p[b] < p[a] ? p[a] : p[b]; \
    p[a] = lo_, p[b] = hi_;                 \
  }
  XM_MC3D_SORT2(1, 2) XM_MC3D_SORT2(4, 5) XM_MC3D_SORT2(7, 8) XM_MC3D_SORT2(0, 1) XM_MC3D_SORT2(3, 4) XM_MC3D_SORT2(6, 7)
  XM_MC3D_SORT2(1, 2) XM_MC3D_SORT2(4, 5) XM_MC3D_SORT2(7, 8) XM_MC3D_SORT2(0, 3) XM_MC3D_SORT2(5, 8) XM_MC3D_SORT2(4, 7)
  XM_MC3D_SORT2(3, 6) XM_MC3D_SORT2(1, 4) XM_MC3D_SORT2(2, 5) XM_MC3D_SORT2(4, 7) XM_MC3D_SORT2(4, 2) XM_MC3D_SORT2(6, 4)
  XM_MC3D_SORT2(4, 2)
#undef XM_MC3D_SORT2
  return p[4];
}

// the key of window position i: yc in (0, 2^30), yp in [-2^30, 2^30] or poison, so the difference fits an int
__device__ inline u32 mc3d_key(int yp, int yc, u32 i, u32 cap, u32 pos_bits) {
  const int d = yc - yp;
  const u32 cost = (u32)(d < 0 ? -d : d);
  return yp == MC3D_POISON ? 0u : (((cost < cap ? cost : cap) << pos_bits) | i) + 1u;
}

// min over aligned groups of GL lanes, in every lane of the group: DPP inside a row of 16 lanes (xor 1, xor 2, mirror of 8,
// mirror of 16), shuffles beyond it
template <u32 GL> __device__ inline u32 group_min_u32(u32 v) {
#define XM_MC3D_DPP_MIN(ctrl)                                                                 \
  {                                                                                           \
    const u32 w = (u32)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, 0xf, 0xf, false);    \
    v = w < v ? w : v;                                                                        \
  }
  if (GL >= 2) XM_MC3D_DPP_MIN(0xB1)    // quad_perm [1, 0, 3, 2]
  if (GL >= 4) XM_MC3D_DPP_MIN(0x4E)    // quad_perm [2, 3, 0, 1]
  if (GL >= 8) XM_MC3D_DPP_MIN(0x141)   // row_half_mirror
  if (GL >= 16) XM_MC3D_DPP_MIN(0x140)  // row_mirror
#undef XM_MC3D_DPP_MIN
#pragma unroll
  for (u32 o = 16; o < GL; o <<= 1) {
    const u32 w = __shfl_xor(v, (int)o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// ---- grid = (ceil(cam_w / MC3D_FW), ceil(cam_h / MC3D_FR), surfaces); cnt: [surface][gridDim.y][gridDim.x] ---------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_mc3d(const T* __restrict__ surf, Mc3dTables tb, u32 flags, float* __restrict__ depth,
                                                 uint16_t* __restrict__ disp_out, Mc3dCnt* __restrict__ cnt) {
  __shared__ u32 s_cnt[MC3D_N_CNT][BLOCK / 64];
  const u32 s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = (int)(blockIdx.x * MC3D_FW + lane), y = (int)(blockIdx.y * MC3D_FR + wave);
  const bool in = x < tb.cam_w && y < tb.cam_h;
  const size_t n_px = (size_t)tb.cam_w * tb.cam_h, px = (size_t)y * tb.cam_w + x;
  const T* img = surf + s * n_px;
  T v = 0;
  bool nz = false;
  if (in) {
    const T c = img[px];
    nz = c != 0;
    if (flags & MC3D_NO_BLUR) {
      v = c;
    } else {
      const int x0 = x > 0 ? x - 1 : 0, x1 = x + 1 < tb.cam_w ? x + 1 : x, y0 = y > 0 ? y - 1 : 0, y1 = y + 1 < tb.cam_h ? y + 1 : y;
      const T *r0 = img + (size_t)y0 * tb.cam_w, *r1 = img + (size_t)y * tb.cam_w, *r2 = img + (size_t)y1 * tb.cam_w;
      T p[9] = {r0[x0], r0[x], r0[x1], r1[x0], c, r1[x1], r2[x0], r2[x], r2[x1]};
      v = mc3d_median9(p);
    }
  }
  const bool pos = v > 0;
  int xc = 0, yc = 0;
  if (pos) {
    const int2 m = tb.cam_map[px];
    xc = m.x, yc = m.y;
  }
  const bool in_rect = pos && xc > 0 && xc < tb.rect_x_limit && yc > 0 && yc < tb.rect_y_limit;
  bool in_range = false;
  u32 base = 0, n_win = 0;  // the window: yp_t[base .. base + n_win)
  if (in_rect) {
    const T wh = (T)(tb.proj_w * tb.proj_h);  // (exact: at most 2^24)
    const T prod = wh * v;                    // the surface's own type, as the reference's int(W * H * v)
    if (prod < wh) {                          // (false for +inf: the reference's swallowed exception)
      in_range = true;
      const u32 id = (u32)prod, H = (u32)tb.proj_h, col = id / H, row = id - col * H, nc = (u32)tb.nc;
      const u32 lo = row > nc ? row - nc : 0u, hi = row + nc < H ? row + nc : H;
      base = col * H + lo, n_win = hi - lo;
    }
  }
  const bool live = in_range && n_win > 0;
  const u32 cap = (u32)tb.max_row_diff + 1u;
  u32 key = 0xffffffffu;
#ifdef XM_MC3D_LANE_WALK
  if (live) {  // every lane walks its own window: eight loads in flight in front of the compare chain
    const int* win = tb.yp_t + base;
    u32 i = 0;
    for (; i + 8 <= n_win; i += 8) {
      int q[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) q[j] = win[i + j];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const u32 k = mc3d_key(q[j], yc, i + j, cap, tb.pos_bits);
        key = k < key ? k : key;
      }
    }
    for (; i < n_win; ++i) {
      const u32 k = mc3d_key(win[i], yc, i, cap, tb.pos_bits);
      key = k < key ? k : key;
    }
  }
#else
  // MC3D_GL lanes share one window, 64 / MC3D_GL windows are walked at once: group g serves the lit pixels of its own lanes, one
  // after the other.  MC3D_UN loads per lane are in flight in front of the compares; positions past the window's end repeat entry 0
  // and are masked out of the key
  constexpr u32 GL = MC3D_GL;
  const u32 sub = lane & (GL - 1), g0 = lane & ~(GL - 1);
  u64 mine = (__ballot(live) >> g0) & (GL == 64 ? ~0ull : (1ull << (GL & 63)) - 1ull);  // my group's lit lanes, not yet served
  while (__any(mine != 0)) {
    const int src = (int)g0 + (mine ? (int)__builtin_ctzll(mine) : 0);
    const u32 b_l = (u32)__shfl((int)base, src, 64), n_l = mine ? (u32)__shfl((int)n_win, src, 64) : 0u;
    const int yc_l = __shfl(yc, src, 64);
    const int* win = tb.yp_t + b_l;
    u32 k = 0xffffffffu;
    for (u32 i = sub; i < n_l; i += MC3D_UN * GL) {
      int q[MC3D_UN];
#pragma unroll
      for (u32 j = 0; j < MC3D_UN; ++j) q[j] = win[i + j * GL < n_l ? i + j * GL : 0u];
#pragma unroll
      for (u32 j = 0; j < MC3D_UN; ++j) {
        const u32 kj = i + j * GL < n_l ? mc3d_key(q[j], yc_l, i + j * GL, cap, tb.pos_bits) : 0xffffffffu;
        k = kj < k ? kj : k;
      }
    }
    k = group_min_u32<GL>(k);
    if ((int)lane == src && mine) key = k;
    mine &= mine - 1;
  }
#endif
  u32 d = 0;
  bool poisoned = false, overflow = false;
  if (live) {
    if (key == 0) {
      poisoned = true;
    } else {
      const u32 kk = key - 1u, at = kk & ((1u << tb.pos_bits) - 1u);
      if ((kk >> tb.pos_bits) < cap) {  // the minimum is <= max_row_diff: only this candidate is ever examined
        const int disp = tb.xp_t[base + at] - xc;  // (|xp| <= 2^30, 0 < xc < 2^30)
        if (disp > 65535) overflow = true;
        else if (disp > 0) d = (u32)disp;
      }
    }
  }
  if (in) {
    depth[s * n_px + px] = d ? (float)(tb.p1_03 / (double)d) : 0.0f;
    if (disp_out) disp_out[s * n_px + px] = (uint16_t)d;
  }
  const bool what[MC3D_N_CNT] = {nz, pos, in_rect, in_rect && !in_range, poisoned, d != 0, overflow};
#pragma unroll
  for (int c = 0; c < MC3D_N_CNT; ++c) {
    const u32 n = (u32)__popcll(__ballot(what[c]));
    if (lane == 0) s_cnt[c][wave] = n;
  }
  __syncthreads();
  if (threadIdx.x < MC3D_N_CNT) {
    u32 sum = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) sum += s_cnt[threadIdx.x][w];
    cnt[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x].n[threadIdx.x] = sum;
  }
}

// one block per surface: the per-block counts added up (each at most cam_w * cam_h < 2^31: the host checks)
__global__ __launch_bounds__(BLOCK) void k_mc3d_stats(const Mc3dCnt* __restrict__ cnt, u32 n_cnt, Mc3dStats* __restrict__ stats) {
  __shared__ u32 s_sum[MC3D_N_CNT][BLOCK / 64];
  const u32 s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 a[MC3D_N_CNT] = {};
  for (u32 i = threadIdx.x; i < n_cnt; i += BLOCK) {
    const Mc3dCnt c = cnt[(size_t)s * n_cnt + i];
#pragma unroll
    for (int k = 0; k < MC3D_N_CNT; ++k) a[k] += c.n[k];
  }
#pragma unroll
  for (int k = 0; k < MC3D_N_CNT; ++k) {
    const u32 t = wave_sum_u32(a[k]);
    if (lane == 0) s_sum[k][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < MC3D_N_CNT) {
    u64 sum = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) sum += s_sum[threadIdx.x][w];
    stats[s].n[threadIdx.x] = sum;
  }
}

}  // namespace xm
