// xmaps_eslfilter.hpp -- gfx950 device code of the two filters behind ESL's depth optimisation (xm_esl_filter_*): what turns
// esl/depth_optim into esl/depth_optim_filtered, the evaluation's ground truth (python/eval/compute_depth_esl.py:243-244:
// cv2.bilateralFilter(depth_optim, 5, 3, 3), then esl_utilities.py:194-224 denoise_tv(mu = 0.5)).  The contract of both stages is
// written out in include/xmaps.h at xm_esl_filter; tests/esl_filter_ref.py states the same arithmetic in NumPy.
//
// Stage 1, float32:
//   k_eslf_extrema    grid (blocks, surfaces): min / max of ESLF_RED_CHUNK pixels as one partial per block
//   k_eslf_table      grid (ceil(4098 / BLOCK), surfaces): every block folds its surface's partials, block 0 records {lo, hi, scale,
//                     copy}; thread i writes colour-table entry i, taken in float64 and rounded
//   k_eslf_bilateral  grid (tiles_x, tiles_y, surfaces): an ESLF_BW x ESLF_BH tile with halo 2 in LDS (REFLECT_101), one pixel per
//                     lane, the taps in raster order; the table is read from memory (16 KB per surface: it stays in cache)
// Stage 2, float64: split Bregman around scipy's lsqr, as a FIXED schedule of launches the host issues without reading anything
// back.  A surface is a flat vector of N = H * W pixels cut into tiles of ESLF_TILE; grid (tiles, surfaces).  Every launch reads
// the surface's control record EslfCtl (one of two copies, by launch parity) and returns at once -- block-uniformly -- where the
// surface's loop has ended; otherwise each block derives the next scalars itself from the previous launch's per-tile partial sums,
// folded in one fixed order (eslf_fold), so all blocks of a surface hold the same bits and the result depends neither on the grid
// nor on the group; block 0 writes the record's other copy.  Partials alternate between two buffers the same way.
//   k_eslf_rhs     per inner call: at the head of an outer iteration the test norm(x - xold) > tol and xold = x; then
//                  u = [y; e_i (d_i - b_i)] - A x, lsqr's x = 0, |u|^2
//   k_eslf_v0      beta = |u|; v = A'(u / beta), |v|^2
//   k_eslf_ustep   C(j), j = 1 .. iter_lim + 1: alfa = |v| and ddnorm from the partials, then the rest of iteration j - 1's
//                  recurrences and its seven stopping tests; x += t1 w (and, unless stopped, w = v + t2 w); then iteration j's
//                  u = A v - alfa u, |u|^2
//   k_eslf_vstep   D(j): beta = |u|, the two plane rotations' first halves; v = A'u - beta v, |v|^2; dk = w / rho, |dk|^2
//   k_eslf_shrink  x += lsqr's x (into the other of two x buffers: neighbours are re-derived from the old one), d_i =
//                  shrink(D_i x + b_i); behind the last inner call b_i += tau (D_i x - d_i) and |x - xold|^2
//   k_eslf_finish  the last norm, the map out, the statistics
// u and v stay UNSCALED in memory: the normalisation (1 / beta) * u is applied by whoever reads an element, which rounds exactly as
// storing it would.  No atomics; no block waits for another; every cross-block dependency is a kernel boundary; the launch counts
// come from the configuration alone.
//
// Arithmetic (built with -ffp-contract=off): every operation is the IEEE one of its format in the order written; float32
// quotients are float64 quotients rounded once more, which is the correctly rounded float32 quotient.  Squares are products
// (the restatement's ** 2 is pow(x, 2)).  NaN input is out of contract: the colour-table index is clamped before its conversion.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

struct EslfExt {  // per surface, from k_eslf_table
  float lo, hi, scale;
  u32 copy;  // hi - lo < FLT_EPSILON: the map passes stage 1 unchanged
};
struct EslfTaps {
  int n;
  int di[ESLF_MAX_TAPS], dj[ESLF_MAX_TAPS];
  float w[ESLF_MAX_TAPS];
};
struct EslfStats {  // == xm_esl_filter_stats (include/xmaps.h)
  double lo, hi, final_norm;
  u32 n_outer, n_lsqr, sum_itn, reserved;
  u32 istop_count[8];
};
struct EslfCtl {
  double alfa, beta, bnorm, rhobar, phibar, anorm, ddnorm, res2, xnorm, xxnorm, z, cs2, sn2;  // scipy's names
  double cs, sn, rho, psi;   // the open iteration's rotations (k_eslf_vstep) for k_eslf_ustep to finish it
  double su, sv;             // pending scales of the stored u and v
  double final_norm;
  u32 itn, lsqr_done, outer_done, beta_zero;
  u32 n_outer, n_lsqr, sum_itn, reserved;
  u32 istop_count[8];
};
struct EslfTv {  // what the stage-2 kernels take by value
  int H, N, n_tiles;  // H: the stride of difference 0 (the image's height: the reference's swapped dims)
  u32 iter_lim, n_calls;  // n_calls = niter_outer * niter_inner: a row of trips
  double e0, e1, lam0, lam1, tau, tol, damp, dampsq, atol, btol, ctol;
  const float* y;  // [surfaces][N]
  double *u0, *u1, *u2, *v, *w, *dx, *x[2], *xold, *b0, *b1, *d0, *d1;  // [surfaces][N] each
  EslfCtl* ctl[2];   // [surfaces]
  double* part[2];   // [surfaces][2][n_tiles]
  uint8_t* trips;    // [surfaces][n_calls]
};

__device__ inline double eslf_sign(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : v; }  // np.sign: 0 and NaN stay

// the sum of a value per thread in one fixed order: the xor butterfly of a wave (every lane ends with the same bits), then the
// waves in order.  Ends behind a barrier, so s_red can be used again at once.
__device__ inline double eslf_block_sum(double v, double* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_red[0];
#pragma unroll
  for (int w = 1; w < BLOCK / 64; ++w) t += s_red[w];
  __syncthreads();
  return t;
}
// a surface's n_tiles partials: thread t takes t, t + BLOCK, ... in order, then eslf_block_sum
__device__ inline double eslf_fold(const double* part, int n_tiles, double* s_red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < n_tiles; i += BLOCK) a += part[i];
  return eslf_block_sum(a, s_red);
}

// ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_eslf_extrema(const float* __restrict__ in, u32 n_px, float2* __restrict__ part) {
  __shared__ float s_lo[BLOCK / 64], s_hi[BLOCK / 64];
  const u32 s = blockIdx.y, base = blockIdx.x * (u32)ESLF_RED_CHUNK;
  const float* img = in + (size_t)s * n_px;
  float lo = INFINITY, hi = -INFINITY;
  for (u32 i = threadIdx.x; i < (u32)ESLF_RED_CHUNK && base + i < n_px; i += BLOCK) {
    const float v = img[base + i];
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) lo = s_lo[w] < lo ? s_lo[w] : lo, hi = s_hi[w] > hi ? s_hi[w] : hi;
    part[(size_t)s * gridDim.x + blockIdx.x] = make_float2(lo, hi);
  }
}

__global__ __launch_bounds__(BLOCK) void k_eslf_table(const float2* __restrict__ part, u32 nb, double color_coeff, float* __restrict__ lut,
                                                       EslfExt* __restrict__ ext) {
  __shared__ float s_lo[BLOCK / 64], s_hi[BLOCK / 64];
  const u32 s = blockIdx.y;
  float lo = INFINITY, hi = -INFINITY;
  for (u32 i = threadIdx.x; i < nb; i += BLOCK) {
    const float2 p = part[(size_t)s * nb + i];
    lo = p.x < lo ? p.x : lo;
    hi = p.y > hi ? p.y : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo, s_hi[threadIdx.x >> 6] = hi;
  __syncthreads();
  lo = s_lo[0], hi = s_hi[0];
#pragma unroll
  for (int w = 1; w < BLOCK / 64; ++w) lo = s_lo[w] < lo ? s_lo[w] : lo, hi = s_hi[w] > hi ? s_hi[w] : hi;
  const double span = (double)hi - (double)lo;  // (exact)
  const bool copy = fabs(span) < (double)1.1920928955078125e-07f;
  const float len = (float)span;
  const float scale = (float)((double)ESLF_BINS / (double)len);
  if (blockIdx.x == 0 && threadIdx.x == 0) ext[s] = EslfExt{lo, hi, scale, copy ? 1u : 0u};
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < (u32)ESLF_BINS + 2u) {
    const double val = (double)(float)((double)(float)i / (double)scale);
    lut[(size_t)s * (ESLF_BINS + 2) + i] = (float)exp(val * val * color_coeff);
  }
}

__device__ inline int eslf_reflect101(int i, int n) {  // |offset| <= 2, any n >= 1
  if (n == 1) return 0;
#pragma unroll 1
  for (int t = 0; t < 4 && (i < 0 || i >= n); ++t) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i < 0 ? 0 : i >= n ? n - 1 : i;
}

__global__ __launch_bounds__(BLOCK) void k_eslf_bilateral(const float* __restrict__ in, int W, int H, EslfTaps taps,
                                                           const float* __restrict__ lut, const EslfExt* __restrict__ ext,
                                                           float* __restrict__ out) {
  constexpr int R = ESLF_HALO, LW = ESLF_BW + 2 * R, LH = ESLF_BH + 2 * R;
  __shared__ float tile[LH][LW];
  const u32 s = blockIdx.z;
  const size_t n_px = (size_t)W * H;
  const float* img = in + s * n_px;
  const EslfExt e = ext[s];
  const int x0 = (int)blockIdx.x * ESLF_BW, y0 = (int)blockIdx.y * ESLF_BH;
  const int tx = (int)threadIdx.x % ESLF_BW, ty = (int)threadIdx.x / ESLF_BW;
  const int x = x0 + tx, y = y0 + ty;
  const bool in_img = x < W && y < H;
  if (e.copy) {  // (block-uniform)
    if (in_img) out[s * n_px + (size_t)y * W + x] = img[(size_t)y * W + x];
    return;
  }
  for (int i = (int)threadIdx.x; i < LW * LH; i += BLOCK) {
    const int lx = i % LW, ly = i / LW;
    int gx = x0 + lx - R, gy = y0 + ly - R;
    gx = gx > W - 1 + R ? W - 1 + R : gx;  // (cells beyond the image's halo are never read: keep the reflection's input small)
    gy = gy > H - 1 + R ? H - 1 + R : gy;
    tile[ly][lx] = img[(size_t)eslf_reflect101(gy, H) * W + eslf_reflect101(gx, W)];
  }
  __syncthreads();
  if (!in_img) return;
  const float* tab = lut + (size_t)s * (ESLF_BINS + 2);
  const float v0 = tile[ty + R][tx + R];
  float sum = 0.0f, wsum = 0.0f;
  for (int k = 0; k < taps.n; ++k) {
    const float v = tile[ty + R + taps.di[k]][tx + R + taps.dj[k]];
    const float a = fabsf(v - v0) * e.scale;
    const int idx = (int)fminf(fmaxf(a, 0.0f), (float)ESLF_BINS);  // (in contract a <= ESLF_BINS; NaN -> 0: nothing indexes outside)
    const float al = a - (float)idx;
    const float l0 = tab[idx], l1 = tab[idx + 1];
    const float w = taps.w[k] * (l0 + al * (l1 - l0));
    sum = sum + v * w;
    wsum = wsum + w;
  }
  out[s * n_px + (size_t)y * W + x] = (float)((double)sum / (double)wsum);
}

__global__ __launch_bounds__(BLOCK) void k_eslf_cast(const float* __restrict__ in, size_t n, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------------
#define ESLF_FOR_OWN(k)                                                                                   \
  for (int k = (int)blockIdx.x * ESLF_TILE + (int)threadIdx.x, k##_end = min(p.N, ((int)blockIdx.x + 1) * ESLF_TILE); k < k##_end; \
       k += BLOCK)

// a block's partial of the sum the next launch folds
__device__ inline void eslf_put_partial(double acc, double* part, int which, int n_tiles, double* s_red) {
  const double t = eslf_block_sum(acc, s_red);
  if (threadIdx.x == 0) part[(size_t)which * n_tiles + blockIdx.x] = t;
}
__device__ inline void eslf_put_ctl(const EslfTv& p, int out, u32 s, const EslfCtl& c) {
  if (blockIdx.x == 0 && threadIdx.x == 0) p.ctl[out][s] = c;
}
// lsqr has returned (istop, itn): the counts, and the call's trip count
__device__ inline void eslf_lsqr_done(const EslfTv& p, u32 s, u32 call, EslfCtl& c, u32 istop) {
  c.lsqr_done = 1;
  c.n_lsqr += 1;
  c.sum_itn += c.itn;
  c.istop_count[istop & 7] += 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) p.trips[(size_t)s * p.n_calls + call] = (uint8_t)c.itn;
}

// D_i' of a (scaled) u_i at k: (u[k] where D_i has a row k) - (u[k'] where row k' reads x[k])
__device__ inline double eslf_dt0(const double* u, double su, int k, int H, int N) {
  return (k >= H ? su * u[k] : 0.0) - (k + H < N ? su * u[k + H] : 0.0);
}
__device__ inline double eslf_dt1(const double* u, double su, int k, int H, int N) {
  return (k % H != 0 ? su * u[k] : 0.0) - ((k + 1) % H != 0 && k + 1 < N ? su * u[k + 1] : 0.0);
}

// launch parity `par`: reads ctl[par] / part[par], writes ctl[par ^ 1] / part[par ^ 1]
__global__ __launch_bounds__(BLOCK) void k_eslf_rhs(EslfTv p, int par, int xsel, int first_inner, int outer) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  EslfCtl c = p.ctl[par][s];
  if (c.outer_done) {
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const size_t o = (size_t)s * p.N;
  const double* X = p.x[xsel] + o;
  if (first_inner) {
    if (outer > 0) {
      const double nrm = sqrt(eslf_fold(p.part[par] + (size_t)s * 2 * p.n_tiles, p.n_tiles, s_red));
      c.final_norm = nrm;
      if (!(nrm > p.tol)) {
        c.outer_done = 1;
        eslf_put_ctl(p, par ^ 1, s, c);
        return;
      }
    }
    c.n_outer += 1;
    ESLF_FOR_OWN(k) p.xold[o + k] = X[k];
  }
  c.itn = 0, c.lsqr_done = 0, c.beta_zero = 0;
  c.anorm = 0.0, c.ddnorm = 0.0, c.res2 = 0.0, c.xnorm = 0.0, c.xxnorm = 0.0, c.z = 0.0, c.cs2 = -1.0, c.sn2 = 0.0;
  c.su = 1.0, c.sv = 1.0;
  double acc = 0.0;
  ESLF_FOR_OWN(k) {
    const double xk = X[k];
    const double r0 = (double)p.y[o + k] - xk;
    const double D0 = k >= p.H ? xk - X[k - p.H] : 0.0, D1 = k % p.H != 0 ? xk - X[k - 1] : 0.0;
    const double r1 = p.e0 * (p.d0[o + k] - p.b0[o + k]) - p.e0 * D0;
    const double r2 = p.e1 * (p.d1[o + k] - p.b1[o + k]) - p.e1 * D1;
    p.u0[o + k] = r0, p.u1[o + k] = r1, p.u2[o + k] = r2;
    p.dx[o + k] = 0.0;
    acc = ((acc + r0 * r0) + r1 * r1) + r2 * r2;
  }
  eslf_put_partial(acc, p.part[par ^ 1] + (size_t)s * 2 * p.n_tiles, 0, p.n_tiles, s_red);
  eslf_put_ctl(p, par ^ 1, s, c);
}

__global__ __launch_bounds__(BLOCK) void k_eslf_v0(EslfTv p, int par, u32 call) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  EslfCtl c = p.ctl[par][s];
  if (c.outer_done || c.lsqr_done) {
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const size_t o = (size_t)s * p.N;
  const double beta = sqrt(eslf_fold(p.part[par] + (size_t)s * 2 * p.n_tiles, p.n_tiles, s_red));
  c.bnorm = beta, c.beta = beta;
  if (!(beta > 0.0)) {  // alfa = 0, arnorm = 0: "the exact solution is x = 0"
    eslf_lsqr_done(p, s, call, c, 0);
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const double su = 1.0 / beta;
  c.su = su;
  const double *u0 = p.u0 + o, *u1 = p.u1 + o, *u2 = p.u2 + o;
  double acc = 0.0;
  ESLF_FOR_OWN(k) {
    const double vk = (su * u0[k] + p.e0 * eslf_dt0(u1, su, k, p.H, p.N)) + p.e1 * eslf_dt1(u2, su, k, p.H, p.N);
    p.v[o + k] = vk;
    acc += vk * vk;
  }
  eslf_put_partial(acc, p.part[par ^ 1] + (size_t)s * 2 * p.n_tiles, 0, p.n_tiles, s_red);
  eslf_put_ctl(p, par ^ 1, s, c);
}

// the second half of lsqr's iteration c.itn (its first half: k_eslf_vstep): -> istop; t1 / t2 are the x and w updates' factors
__device__ inline u32 eslf_finish_iteration(const EslfTv& p, EslfCtl& c, double& t1x, double& t2w) {
  const double eps = 2.220446049250313e-16;
  const double theta = c.sn * c.alfa;
  c.rhobar = -c.cs * c.alfa;
  const double phi = c.cs * c.phibar;
  c.phibar = c.sn * c.phibar;
  const double tau = c.sn * phi;
  t1x = phi / c.rho;
  t2w = -theta / c.rho;
  const double delta = c.sn2 * c.rho;
  const double gambar = -c.cs2 * c.rho;
  const double rhs = phi - delta * c.z;
  const double zbar = rhs / gambar;
  c.xnorm = sqrt(c.xxnorm + zbar * zbar);
  const double gamma = sqrt(gambar * gambar + theta * theta);
  c.cs2 = gambar / gamma;
  c.sn2 = theta / gamma;
  c.z = rhs / gamma;
  c.xxnorm = c.xxnorm + c.z * c.z;
  const double acond = c.anorm * sqrt(c.ddnorm);
  const double res1 = c.phibar * c.phibar;
  c.res2 = c.res2 + c.psi * c.psi;
  const double rnorm = sqrt(res1 + c.res2);
  const double arnorm = c.alfa * fabs(tau);
  const double test1 = rnorm / c.bnorm;
  const double test2 = arnorm / (c.anorm * rnorm + eps);
  const double test3 = 1.0 / (acond + eps);
  const double t1 = test1 / (1.0 + c.anorm * c.xnorm / c.bnorm);
  const double rtol = p.btol + p.atol * c.anorm * c.xnorm / c.bnorm;
  u32 istop = 0;
  if (c.itn >= p.iter_lim) istop = 7;
  if (1.0 + test3 <= 1.0) istop = 6;
  if (1.0 + test2 <= 1.0) istop = 5;
  if (1.0 + t1 <= 1.0) istop = 4;
  if (test3 <= p.ctol) istop = 3;
  if (test2 <= p.atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  return istop;
}

// C(j): c.itn == j - 1 on entry
__global__ __launch_bounds__(BLOCK) void k_eslf_ustep(EslfTv p, int par, u32 call) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  EslfCtl c = p.ctl[par][s];
  if (c.outer_done || c.lsqr_done) {
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const size_t o = (size_t)s * p.N;
  const double* part = p.part[par] + (size_t)s * 2 * p.n_tiles;
  const double* v = p.v + o;
  const bool first = c.itn == 0;
  double t1x = 0.0, t2w = 0.0;
  u32 istop = 0;
  if (first) {
    c.alfa = sqrt(eslf_fold(part, p.n_tiles, s_red));
    if (c.alfa > 0.0) c.sv = 1.0 / c.alfa;
    c.rhobar = c.alfa, c.phibar = c.beta;
    if (c.alfa * c.beta == 0.0 || c.alfa != c.alfa) {  // arnorm == 0: x = 0 (a NaN norm ends the call the same way: nothing to iterate on)
      eslf_lsqr_done(p, s, call, c, 0);
      eslf_put_ctl(p, par ^ 1, s, c);
      return;
    }
  } else {
    if (!c.beta_zero) {
      c.alfa = sqrt(eslf_fold(part, p.n_tiles, s_red));
      c.sv = c.alfa > 0.0 ? 1.0 / c.alfa : 1.0;
    }
    const double dn = sqrt(eslf_fold(part + p.n_tiles, p.n_tiles, s_red));
    c.ddnorm = c.ddnorm + dn * dn;
    istop = eslf_finish_iteration(p, c, t1x, t2w);
  }
  const double sv = c.sv;
  if (istop != 0) {
    ESLF_FOR_OWN(k) p.dx[o + k] = p.dx[o + k] + t1x * p.w[o + k];
    eslf_lsqr_done(p, s, call, c, istop);
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const double su = c.su, alfa = c.alfa;
  double acc = 0.0;
  ESLF_FOR_OWN(k) {
    const double vk = sv * v[k];
    if (first) {
      p.w[o + k] = vk;
    } else {
      const double wk = p.w[o + k];
      p.dx[o + k] = p.dx[o + k] + t1x * wk;
      p.w[o + k] = vk + t2w * wk;
    }
    const double a1 = p.e0 * (k >= p.H ? vk - sv * v[k - p.H] : 0.0), a2 = p.e1 * (k % p.H != 0 ? vk - sv * v[k - 1] : 0.0);
    const double n0 = vk - alfa * (su * p.u0[o + k]), n1 = a1 - alfa * (su * p.u1[o + k]), n2 = a2 - alfa * (su * p.u2[o + k]);
    p.u0[o + k] = n0, p.u1[o + k] = n1, p.u2[o + k] = n2;
    acc = ((acc + n0 * n0) + n1 * n1) + n2 * n2;
  }
  c.itn += 1;
  eslf_put_partial(acc, p.part[par ^ 1] + (size_t)s * 2 * p.n_tiles, 0, p.n_tiles, s_red);
  eslf_put_ctl(p, par ^ 1, s, c);
}

// scipy's _sym_ortho
__device__ inline void eslf_sym_ortho(double a, double b, double& c, double& s, double& r) {
  if (b == 0.0) {
    c = eslf_sign(a), s = 0.0, r = fabs(a);
  } else if (a == 0.0) {
    c = 0.0, s = eslf_sign(b), r = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = eslf_sign(b) / sqrt(1.0 + tau * tau);
    c = s * tau;
    r = b / s;
  } else {
    const double tau = b / a;
    c = eslf_sign(a) / sqrt(1.0 + tau * tau);
    s = c * tau;
    r = a / c;
  }
}

// D(j)
__global__ __launch_bounds__(BLOCK) void k_eslf_vstep(EslfTv p, int par) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  EslfCtl c = p.ctl[par][s];
  if (c.outer_done || c.lsqr_done) {
    eslf_put_ctl(p, par ^ 1, s, c);
    return;
  }
  const size_t o = (size_t)s * p.N;
  const double beta = sqrt(eslf_fold(p.part[par] + (size_t)s * 2 * p.n_tiles, p.n_tiles, s_red));
  c.beta = beta;
  const bool live = beta > 0.0;
  const double sv_old = c.sv;
  if (live) {
    c.su = 1.0 / beta;
    c.anorm = sqrt(((c.anorm * c.anorm + c.alfa * c.alfa) + beta * beta) + p.dampsq);
    c.beta_zero = 0;
  } else {
    c.su = 1.0;
    c.beta_zero = 1;
  }
  double rhobar1;
  if (p.damp > 0.0) {
    rhobar1 = sqrt(c.rhobar * c.rhobar + p.dampsq);
    const double cs1 = c.rhobar / rhobar1, sn1 = p.damp / rhobar1;
    c.psi = sn1 * c.phibar;
    c.phibar = cs1 * c.phibar;
  } else {
    rhobar1 = c.rhobar;
    c.psi = 0.0;
  }
  eslf_sym_ortho(rhobar1, beta, c.cs, c.sn, c.rho);
  const double su = c.su, inv_rho = 1.0 / c.rho;
  const double *u0 = p.u0 + o, *u1 = p.u1 + o, *u2 = p.u2 + o;
  double accv = 0.0, accd = 0.0;
  ESLF_FOR_OWN(k) {
    if (live) {
      const double au = (su * u0[k] + p.e0 * eslf_dt0(u1, su, k, p.H, p.N)) + p.e1 * eslf_dt1(u2, su, k, p.H, p.N);
      const double vk = au - beta * (sv_old * p.v[o + k]);
      p.v[o + k] = vk;
      accv += vk * vk;
    }
    const double dk = inv_rho * p.w[o + k];
    accd += dk * dk;
  }
  double* part = p.part[par ^ 1] + (size_t)s * 2 * p.n_tiles;
  eslf_put_partial(accv, part, 0, p.n_tiles, s_red);
  eslf_put_partial(accd, part, 1, p.n_tiles, s_red);
  eslf_put_ctl(p, par ^ 1, s, c);
}

__device__ inline double eslf_shrink(double t, double lam) {
  const double m = fabs(t) - lam;
  return (m > 0.0 ? m : m != m ? m : 0.0) * eslf_sign(t);
}

// xsel: the x buffer the call started from; the sum goes into the other one
__global__ __launch_bounds__(BLOCK) void k_eslf_shrink(EslfTv p, int par, int xsel, int last_inner) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  const EslfCtl c = p.ctl[par][s];
  eslf_put_ctl(p, par ^ 1, s, c);
  if (c.outer_done) return;
  const size_t o = (size_t)s * p.N;
  const double *X = p.x[xsel] + o, *dx = p.dx + o;
  double acc = 0.0;
  ESLF_FOR_OWN(k) {
    const double xn = X[k] + dx[k];
    p.x[xsel ^ 1][o + k] = xn;
    const double D0 = k >= p.H ? xn - (X[k - p.H] + dx[k - p.H]) : 0.0, D1 = k % p.H != 0 ? xn - (X[k - 1] + dx[k - 1]) : 0.0;
    const double b0 = p.b0[o + k], b1 = p.b1[o + k];
    const double d0 = eslf_shrink(D0 + b0, p.lam0), d1 = eslf_shrink(D1 + b1, p.lam1);
    p.d0[o + k] = d0, p.d1[o + k] = d1;
    if (last_inner) {
      p.b0[o + k] = b0 + p.tau * (D0 - d0);
      p.b1[o + k] = b1 + p.tau * (D1 - d1);
      const double df = xn - p.xold[o + k];
      acc += df * df;
    }
  }
  if (last_inner) eslf_put_partial(acc, p.part[par ^ 1] + (size_t)s * 2 * p.n_tiles, 0, p.n_tiles, s_red);
}

__global__ __launch_bounds__(BLOCK) void k_eslf_finish(EslfTv p, int par, const EslfExt* __restrict__ ext, double* __restrict__ out,
                                                        EslfStats* __restrict__ stats) {
  __shared__ double s_red[BLOCK / 64];
  const u32 s = blockIdx.y;
  EslfCtl c = p.ctl[par][s];
  if (!c.outer_done) c.final_norm = sqrt(eslf_fold(p.part[par] + (size_t)s * 2 * p.n_tiles, p.n_tiles, s_red));  // (block-uniform)
  const size_t o = (size_t)s * p.N;
  const double* X = p.x[c.n_lsqr & 1] + o;
  ESLF_FOR_OWN(k) out[o + k] = X[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    EslfStats st{};
    st.lo = (double)ext[s].lo, st.hi = (double)ext[s].hi, st.final_norm = c.final_norm;
    st.n_outer = c.n_outer, st.n_lsqr = c.n_lsqr, st.sum_itn = c.sum_itn;
    for (int i = 0; i < 8; ++i) st.istop_count[i] = c.istop_count[i];
    stats[s] = st;
  }
}

// statistics of a call without stage 2
__global__ void k_eslf_stats_only(const EslfExt* __restrict__ ext, u32 n, EslfStats* __restrict__ stats) {
  const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  EslfStats st{};
  st.lo = (double)ext[s].lo, st.hi = (double)ext[s].hi;
  stats[s] = st;
}

#undef ESLF_FOR_OWN

}  // namespace xm
