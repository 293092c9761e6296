// xmaps_esloptim.hpp -- gfx950 device code of the ESL depth optimisation (xm_esl_optim_*): the point-wise refinement behind ESL-init
// that writes the evaluation's ground truth before its two filters (python/eval/compute_depth_esl.py:104-129 depth_optimization,
// :45-69 cost_calculator, :27-42 project_and_backproject_punkt), on the device.
//
// Per camera pixel (x, y) inside the window_size border whose depth_init d0 is > 0: one bounded scalar minimisation of
//   cost(rho) = || cam'[y-w..y+w][x-w..x+w] - proj[yp-w..yp+w][xp-w..xp+w] ||,  (xp, yp) = trunc(project(backproject(x, y, rho)))
// over rho in [d0 - d0^2 / P1[0,3], d0 + d0^2 / P1[0,3]], 100000 where the projected patch leaves the projector.  The minimiser is
// scipy's _minimize_scalar_bounded (golden section + parabolic interpolation), restated operation for operation in float64:
// eslo_minimise below keeps its variable names.  Its trip count depends on the data; num >= maxfun bounds every loop.
//   k_esl_optim        one lane per camera pixel, grid = (tiles_x, tiles_y, surfaces): lo / hi of the surface from k_surf_extrema's
//                      partials (xmaps_surface.hpp), re-reduced by every wave; the (2w+1)^2 normalised, filled camera patch and the
//                      undistorted pixel in registers; the projector patch gathered per evaluation (the surface stays in L2); ONE
//                      plain store of the depth and one of the evaluation count; the counts leave as one partial per block
//   k_esl_optim_stats  one block per surface: the partials added up
// No atomics, and no block waits for another: every cross-block dependency is a kernel boundary.
//
// Arithmetic (built with -ffp-contract=off): every operation is an IEEE float64 one in the order it is written -- divisions and the
// square root correctly rounded -- except where the restatement says otherwise: d0 * d0 is a float32 product, the undistorted pixel
// is rounded to float32, and the patch sum is the chain s = fma(d, d, s) (what np.linalg.norm's dot computes).  NaN follows
// np.sign / np.maximum (it propagates) and comparisons (false).  A projected coordinate that is not finite or does not fit an int32
// counts as outside, so nothing here indexes a table with it.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_surface.hpp"  // SurfPart1, surf_norm, surf_normalisable, surf_block_reduce

namespace xm {

constexpr int ESLO_FW = 64, ESLO_FR = BLOCK / 64;  // 64 camera pixels of a row per wave, one row per wave
constexpr int ESLO_MAX_WS = 7;                     // window_size: odd, at most this
constexpr double ESLO_OUTSIDE = 100000.0;          // compute_depth_esl.py:68

struct EslOptPinhole {  // K and the Brown coefficients k1 k2 p1 p2 k3
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};
struct EslOptTables {  // what k_esl_optim takes by value
  const float* proj;   // [proj_h][proj_w] the unrectified projector time surface
  int cam_w, cam_h, proj_w, proj_h, ws;
  u32 max_iter;
  double xatol, p1_03, sqrt_eps, golden_mean;  // (the two constants: sqrt(2.2e-16) and 0.5 * (3 - sqrt(5)), taken on the host)
  EslOptPinhole cam, prj;
  double Rt[12];  // R' row-major, then t
};
struct EslOptStats {  // == xm_esl_optim_stats (include/xmaps.h)
  u64 n_optimised, n_evals, n_hit_limit, n_bad_bounds;
  double lo, hi;
};
struct EslOptCnt {  // per block
  u32 n_optimised, n_evals, n_hit_limit, n_bad_bounds;
};

__device__ inline double eslo_sign_or_one(double v) {  // np.sign(v) + (v == 0): NaN stays NaN
  return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : v == 0.0 ? 1.0 : v;
}
__device__ inline double eslo_maximum(double a, double b) {  // np.maximum: NaN if either is
  return a != a ? a : b != b ? b : a >= b ? a : b;
}
__device__ inline bool eslo_finite(double v) { return fabs(v) < INFINITY; }

struct EslOptResult {
  double xf;
  u32 nfev;
  bool hit_limit;
};

// scipy.optimize._optimize._minimize_scalar_bounded (1.15): func is evaluated at most max(maxfun, 2) times
template <typename F>
__device__ inline EslOptResult eslo_minimise(F&& func, double x1, double x2, double xatol, u32 maxfun, double sqrt_eps,
                                             double golden_mean) {
  double a = x1, b = x2;
  double fulc = a + golden_mean * (b - a);
  double nfc = fulc, xf = fulc;
  double rat = 0.0, e = 0.0;
  double x = xf;
  double fx = func(x);
  u32 num = 1;
  double ffulc = fx, fnfc = fx;
  double xm = 0.5 * (a + b);
  double tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
  double tol2 = 2.0 * tol1;
  bool hit = false;
  while (fabs(xf - xm) > (tol2 - 0.5 * (b - a))) {
    bool golden = true;
    if (fabs(e) > tol1) {  // a parabolic fit
      golden = false;
      double r = (xf - nfc) * (fx - ffulc);
      double q = (xf - fulc) * (fx - fnfc);
      double p = (xf - fulc) * q - (xf - nfc) * r;
      q = 2.0 * (q - r);
      if (q > 0.0) p = -p;
      q = fabs(q);
      r = e;
      e = rat;
      if (fabs(p) < fabs(0.5 * q * r) && p > q * (a - xf) && p < q * (b - xf)) {
        rat = (p + 0.0) / q;
        x = xf + rat;
        if ((x - a) < tol2 || (b - x) < tol2) rat = tol1 * eslo_sign_or_one(xm - xf);
      } else {
        golden = true;
      }
    }
    if (golden) {  // a golden-section step
      e = xf >= xm ? a - xf : b - xf;
      rat = golden_mean * e;
    }
    x = xf + eslo_sign_or_one(rat) * eslo_maximum(fabs(rat), tol1);
    const double fu = func(x);
    num += 1;
    if (fu <= fx) {
      if (x >= xf) a = xf;
      else b = xf;
      fulc = nfc, ffulc = fnfc;
      nfc = xf, fnfc = fx;
      xf = x, fx = fu;
    } else {
      if (x < xf) a = x;
      else b = x;
      if (fu <= fnfc || nfc == xf) {
        fulc = nfc, ffulc = fnfc;
        nfc = x, fnfc = fu;
      } else if (fu <= ffulc || fulc == xf || fulc == nfc) {
        fulc = x, ffulc = fu;
      }
    }
    xm = 0.5 * (a + b);
    tol1 = sqrt_eps * fabs(xf) + xatol / 3.0;
    tol2 = 2.0 * tol1;
    if (num >= maxfun) {
      hit = true;
      break;
    }
  }
  return EslOptResult{xf, num, hit};
}

// cv2.undistortPoints((x, y) float32, K, D, P = K): five fixed-point rounds, the result rounded to float32
__device__ inline void eslo_undistort(const EslOptPinhole& c, float px, float py, float& ux, float& uy) {
  const double x0 = ((double)px - c.cx) / c.fx, y0 = ((double)py - c.cy) / c.fy;
  double x = x0, y = y0;
#pragma unroll 1
  for (int it = 0; it < 5; ++it) {
    const double r2 = x * x + y * y;
    const double icdist = 1.0 / (1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3)));
    const double dx = ((2.0 * c.p1) * x) * y + c.p2 * (r2 + (2.0 * x) * x);
    const double dy = c.p1 * (r2 + (2.0 * y) * y) + ((2.0 * c.p2) * x) * y;
    x = (x0 - dx) * icdist;
    y = (y0 - dy) * icdist;
  }
  ux = (float)(c.fx * x + c.cx);
  uy = (float)(c.fy * y + c.cy);
}

// cv2.projectPoints of one point: R' (X, Y, Z) + t, perspective divide, Brown distortion, K
__device__ inline void eslo_project(const EslOptTables& tb, double X, double Y, double Z, double& u, double& v) {
  const double* R = tb.Rt;
  const EslOptPinhole& c = tb.prj;
  const double xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[9];
  const double yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + R[10];
  const double zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + R[11];
  const double x = xc / zc, y = yc / zc;
  const double r2 = x * x + y * y;
  const double radial = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
  const double xd = (x * radial + ((2.0 * c.p1) * x) * y) + c.p2 * (r2 + (2.0 * x) * x);
  const double yd = (y * radial + c.p1 * (r2 + (2.0 * y) * y)) + ((2.0 * c.p2) * x) * y;
  u = c.fx * xd + c.cx;
  v = c.fy * yd + c.cy;
}

// float64 -> int32 by truncation toward zero; false for a value that is not finite or not representable
__device__ inline bool eslo_trunc(double v, int& out) {
  const bool ok = v > -2147483649.0 && v < 2147483648.0;
  out = ok ? (int)v : 0;
  return ok;
}

// ---- grid = (ceil(cam_w / ESLO_FW), ceil(cam_h / ESLO_FR), surfaces); W = window_size / 2 --------------------------------------
// part1: k_surf_extrema's partials [surface][nb_red]; cnt: [surface][gridDim.y][gridDim.x]
template <typename T, int W>
__global__ __launch_bounds__(BLOCK) void k_esl_optim(const T* __restrict__ surf, const float* __restrict__ depth_init, EslOptTables tb,
                                                      const SurfPart1* __restrict__ part1, u32 nb_red, float* __restrict__ depth,
                                                      uint16_t* __restrict__ nfev, EslOptCnt* __restrict__ cnt) {
  constexpr int P = 2 * W + 1;
  __shared__ u32 s_cnt[4][BLOCK / 64];
  const u32 s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SurfPart1* p1 = part1 + (size_t)s * nb_red;
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0;
  for (u32 i = lane; i < nb_red; i += 64) {  // every wave reduces the surface's partials itself, as k_esl_fused does (a few KB, L2-hot)
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
  const int x = (int)(blockIdx.x * ESLO_FW + lane), y = (int)(blockIdx.y * ESLO_FR + wave);
  const bool in = x < tb.cam_w && y < tb.cam_h;
  const size_t n_px = (size_t)tb.cam_w * tb.cam_h, px = (size_t)y * tb.cam_w + x;
  const T* img = surf + s * n_px;
  const float d0 = in ? depth_init[s * n_px + px] : 0.0f;
  // (the border is window_size, the patch half-width w = window_size / 2: compute_depth_esl.py:107-108, :53)
  const bool live = in && valid && x >= tb.ws && x < tb.cam_w - tb.ws && y >= tb.ws && y < tb.cam_h - tb.ws && d0 > 0.0f;
  bool bad = false;
  EslOptResult res{0.0, 0u, false};
  if (live) {
    const double diff = (double)(d0 * d0) / tb.p1_03;  // (a float32 product, a float64 quotient)
    const double a = (double)d0 - diff, b = (double)d0 + diff;
    bad = !(eslo_finite(a) && eslo_finite(b)) || a > b;
    if (!bad) {
      const double fill = 1.0 / surf_norm(img[0], lo, den);  // (:212; +inf when pixel (0, 0) normalises to 0)
      double cam[P * P];
#pragma unroll
      for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const double v = surf_norm(img[(size_t)(y + i - W) * tb.cam_w + (x + j - W)], lo, den);
          cam[i * P + j] = v == 0.0 ? fill : v;
        }
      float ux, uy;
      eslo_undistort(tb.cam, (float)x, (float)y, ux, uy);
      const double ax = ((double)ux - tb.cam.cx) / tb.cam.fx, ay = ((double)uy - tb.cam.cy) / tb.cam.fy;
      auto cost = [&](double rho) -> double {
        double u, v;
        eslo_project(tb, ax * rho, ay * rho, rho, u, v);
        int xp, yp;
        const bool ok = eslo_trunc(u, xp) & eslo_trunc(v, yp);
        if (!(ok && yp > W && yp < tb.proj_h - W && xp > W && xp < tb.proj_w - W)) return ESLO_OUTSIDE;
        const float* pp = tb.proj + (size_t)(yp - W) * tb.proj_w + (xp - W);  // rows yp-W .. yp+W lie in [1, proj_h - 1)
        double sum = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const double d = cam[i * P + j] - (double)pp[(size_t)i * tb.proj_w + j];
            sum = fma(d, d, sum);
          }
        return sqrt(sum);
      };
      res = eslo_minimise(cost, a, b, tb.xatol, tb.max_iter, tb.sqrt_eps, tb.golden_mean);
    }
  }
  const bool opt = live && !bad;
  if (in) {
    depth[s * n_px + px] = opt ? (float)res.xf : 0.0f;
    if (nfev) nfev[s * n_px + px] = (uint16_t)res.nfev;  // (at most max(max_iter, 2) <= 65535)
  }
  const u32 n_opt = (u32)__popcll(__ballot(opt)), n_ev = wave_sum_u32(res.nfev), n_hit = (u32)__popcll(__ballot(res.hit_limit)),
            n_bad = (u32)__popcll(__ballot(bad));
  if (lane == 0) s_cnt[0][wave] = n_opt, s_cnt[1][wave] = n_ev, s_cnt[2][wave] = n_hit, s_cnt[3][wave] = n_bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int w = 0; w < BLOCK / 64; ++w) c[k] += s_cnt[k][w];
    cnt[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = EslOptCnt{c[0], c[1], c[2], c[3]};  // (c[1] <= 256 * 65535)
  }
}

__device__ inline u64 eslo_wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one block per surface: the surface's statistics out of the extrema partials and k_esl_optim's per-block counts
__global__ __launch_bounds__(BLOCK) void k_esl_optim_stats(const SurfPart1* __restrict__ part1, u32 nb_red, const EslOptCnt* __restrict__ cnt,
                                                            u32 n_cnt, EslOptStats* __restrict__ stats) {
  __shared__ u64 s_sum[4][BLOCK / 64];
  const u32 s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double lo = INFINITY, hi = -INFINITY;
  u32 nnz = 0;
  for (u32 i = threadIdx.x; i < nb_red; i += BLOCK) {
    const SurfPart1 p = part1[(size_t)s * nb_red + i];
    lo = p.lo < lo ? p.lo : lo;
    hi = p.hi > hi ? p.hi : hi;
    nnz += (u32)p.nnz;
  }
  u64 a[4] = {0, 0, 0, 0};
  for (u32 i = threadIdx.x; i < n_cnt; i += BLOCK) {
    const EslOptCnt c = cnt[(size_t)s * n_cnt + i];
    a[0] += c.n_optimised, a[1] += c.n_evals, a[2] += c.n_hit_limit, a[3] += c.n_bad_bounds;
  }
  surf_block_reduce(lo, hi, nnz);  // (valid in thread 0; ends behind a barrier)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const u64 t = eslo_wave_sum_u64(a[k]);
    if (lane == 0) s_sum[k][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int w = 0; w < BLOCK / 64; ++w) t[k] += s_sum[k][w];
    stats[s] = EslOptStats{t[0], t[1], t[2], t[3], nnz ? lo : 0.0, nnz ? hi : 0.0};
  }
}

}  // namespace xm
