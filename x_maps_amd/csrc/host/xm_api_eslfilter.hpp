// xm_api_eslfilter.hpp -- C-ABI: the two filters behind ESL's depth optimisation (a group of depth_optim maps -> depth_optim_filtered)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_eslfilter.hpp.  No xm_handle: the object owns its device, stream and scratch.
#pragma once

static_assert(sizeof(xm_esl_filter_stats) == sizeof(EslfStats), "xm_esl_filter_stats is what k_eslf_finish writes");
static_assert(XM_ESL_FILTER_NO_BILATERAL == ESLF_NO_BILATERAL && XM_ESL_FILTER_NO_TV == ESLF_NO_TV, "xmaps.h and xmaps_geometry.hpp");
static_assert(ESLF_BW * ESLF_BH == BLOCK && ESLF_TILE % BLOCK == 0, "one pixel per lane; whole passes per tile");

struct xm_esl_filter : GroupObj {
  int W = 0, H = 0;
  u32 flags = 0, niter_outer = 0, niter_inner = 0;
  double color_coeff = 0.0;
  EslfTaps taps{};
  EslfTv tv{};  // (the parameters; the pointers are set per call)
  u64 last_launches = 0;
  DevBuf red, lut, ext, vec, ctl, part, trips, stats;  // device-side intermediates of a group
  DevBuf in, bil, out;                                 // staging of XM_MEM_HOST calls, and stage 1's result
};

extern "C" {

void xm_esl_filter_destroy(xm_esl_filter* e) { group_destroy(e); }

int xm_esl_filter_create(int device, const xm_esl_filter_config* cfg, xm_esl_filter** out) {
  if (int rc = group_create_args(cfg, out, "xm_esl_filter_config")) return rc;
  if (cfg->width <= 0 || cfg->height <= 0) return fail(XM_ERR_INVALID, "dimensions must be positive");
  if ((u64)cfg->width * (u64)cfg->height > (1ull << 30)) return fail(XM_ERR_INVALID, "map too large");
  if (cfg->flags & ~(XM_ESL_FILTER_NO_BILATERAL | XM_ESL_FILTER_NO_TV)) return fail(XM_ERR_INVALID, "unknown flag");
  if ((cfg->flags & XM_ESL_FILTER_NO_BILATERAL) && (cfg->flags & XM_ESL_FILTER_NO_TV)) return fail(XM_ERR_INVALID, "no stage left");
  const int d = cfg->d ? cfg->d : 5, n_out = cfg->niter_outer ? cfg->niter_outer : 20, n_in = cfg->niter_inner ? cfg->niter_inner : 10,
            iter_lim = cfg->iter_lim ? cfg->iter_lim : 5;
  if (d != 1 && d != 3 && d != 5) return fail(XM_ERR_INVALID, "d must be 1, 3 or 5 (got %d)", d);
  if (n_out < 1 || n_out > 255 || n_in < 1 || n_in > 255) return fail(XM_ERR_INVALID, "niter_outer and niter_inner must lie in 1 .. 255");
  if (iter_lim < 1 || iter_lim > 254) return fail(XM_ERR_INVALID, "iter_lim must lie in 1 .. 254");
  const double sc = cfg->sigma_color != 0.0 ? cfg->sigma_color : 3.0, ss = cfg->sigma_space != 0.0 ? cfg->sigma_space : 3.0;
  const double mu = cfg->mu != 0.0 ? cfg->mu : 0.5, l0 = cfg->lambda0 != 0.0 ? cfg->lambda0 : 0.1, l1 = cfg->lambda1 != 0.0 ? cfg->lambda1 : 0.1;
  const double tol = cfg->tol != 0.0 ? cfg->tol : 1e-4, tau = cfg->tau != 0.0 ? cfg->tau : 1.0, damp = cfg->damp != 0.0 ? cfg->damp : 1e-4;
  const double pos[] = {sc, ss, mu, l0, l1, tol, tau, damp};
  for (double v : pos)
    if (!(v > 0.0) || !std::isfinite(v)) return fail(XM_ERR_INVALID, "sigmas, mu, lambdas, tol, tau and damp must be positive and finite");
  Owned<xm_esl_filter, xm_esl_filter_destroy> e;
  if (int rc = group_open(device, e)) return rc;
  e->noun = "maps", e->px = (size_t)cfg->width * cfg->height, e->total_log2 = 36;
  e->W = cfg->width, e->H = cfg->height, e->flags = cfg->flags, e->niter_outer = (u32)n_out, e->niter_inner = (u32)n_in;
  e->color_coeff = -0.5 / (sc * sc);
  const int radius = d / 2;
  const double space_coeff = -0.5 / (ss * ss);
  for (int i = -radius; i <= radius; ++i)
    for (int j = -radius; j <= radius; ++j) {
      const double r = std::sqrt((double)(i * i + j * j));
      if (r > radius) continue;
      EslfTaps& t = e->taps;
      t.di[t.n] = i, t.dj[t.n] = j, t.w[t.n] = (float)std::exp(r * r * space_coeff);
      ++t.n;
    }
  EslfTv& p = e->tv;
  p.H = cfg->height, p.N = cfg->width * cfg->height, p.n_tiles = (int)grid_for((u64)p.N, ESLF_TILE);
  p.iter_lim = (u32)iter_lim, p.n_calls = (u32)(n_out * n_in);
  p.e0 = std::sqrt(l0 / 2.0) / std::sqrt(mu / 2.0), p.e1 = std::sqrt(l1 / 2.0) / std::sqrt(mu / 2.0);
  p.lam0 = l0, p.lam1 = l1, p.tau = tau, p.tol = tol, p.damp = damp;
  p.dampsq = std::pow(damp, 2.0);  // (scipy's damp**2)
  p.atol = 1e-6, p.btol = 1e-6, p.ctol = 1.0 / 1e8;
  *out = e.release();
  return XM_OK;
}

int xm_esl_filter_last_launches(xm_esl_filter* e, uint64_t* out) {
  if (!e || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = e->last_launches;
  return XM_OK;
}

int xm_esl_filter_maps(xm_esl_filter* e, const float* depth_optim, int n_maps, int mem, double* filtered_out, float* bilateral_out,
                       uint8_t* trips_out, xm_esl_filter_stats* stats_out) {
  if (int rc = group_enter(e, n_maps, mem)) return rc;
  if (!depth_optim || !filtered_out) return fail(XM_ERR_INVALID, "NULL argument");
  const size_t n = (size_t)n_maps, px = e->px, total = n * px;
  const bool do_bil = !(e->flags & XM_ESL_FILTER_NO_BILATERAL), do_tv = !(e->flags & XM_ESL_FILTER_NO_TV);
  const u32 nb_red = grid_for(px, ESLF_RED_CHUNK), nb_lut = grid_for(ESLF_BINS + 2, BLOCK);
  const u32 tiles_x = grid_for(e->W, ESLF_BW), tiles_y = grid_for(e->H, ESLF_BH);
  if (tiles_y > 65535) return fail(XM_ERR_INVALID, "map too tall (at most %d rows)", 65535 * ESLF_BH);
  EslfTv p = e->tv;
  const size_t n_tiles = (size_t)p.n_tiles;
  constexpr size_t N_VEC = 13;
  hipStream_t stream = e->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const float* d_in = c.in(e->in, depth_optim, total * 4);
  double* d_out = c.out(e->out, filtered_out, total * 8);
  // stage 1's result: stage 2 reads it, so it exists whether or not the caller asked for it
  float* d_bil = c.out(e->bil, do_bil ? bilateral_out : nullptr, total * 4, do_bil);
  if (int rc = c.start({{e->red, n * nb_red * sizeof(float2)},
                     {e->lut, n * (ESLF_BINS + 2) * sizeof(float)},
                     {e->ext, n * sizeof(EslfExt)},
                     {e->vec, do_tv ? N_VEC * total * sizeof(double) : 0},
                     {e->ctl, do_tv ? 2 * n * sizeof(EslfCtl) : 0},
                     {e->part, do_tv ? 2 * n * 2 * n_tiles * sizeof(double) : 0},
                     {e->trips, do_tv ? n * p.n_calls : 0},
                     {e->stats, n * sizeof(EslfStats)}}))
    return rc;
  u64 launches = 0;
  float2* red = (float2*)e->red.p;
  float* lut = (float*)e->lut.p;
  EslfExt* ext = (EslfExt*)e->ext.p;
  EslfStats* d_stats = (EslfStats*)e->stats.p;
  const unsigned m = (unsigned)n;

  // stage 1 (the extrema are statistics too: they are taken even when the filter is off)
  hipLaunchKernelGGL(k_eslf_extrema, dim3(nb_red, m), dim3(BLOCK), 0, stream, d_in, (u32)px, red);
  hipLaunchKernelGGL(k_eslf_table, dim3(nb_lut, m), dim3(BLOCK), 0, stream, (const float2*)red, nb_red, e->color_coeff, lut, ext);
  launches += 2;
  const float* d_mid = d_in;
  if (do_bil) {
    hipLaunchKernelGGL(k_eslf_bilateral, dim3(tiles_x, tiles_y, m), dim3(BLOCK), 0, stream, d_in, e->W, e->H, e->taps, (const float*)lut,
                       (const EslfExt*)ext, d_bil);
    ++launches;
    d_mid = d_bil;
  }
  if (!do_tv) {
    hipLaunchKernelGGL(k_eslf_cast, dim3(grid_for(total, BLOCK)), dim3(BLOCK), 0, stream, d_mid, total, d_out);
    hipLaunchKernelGGL(k_eslf_stats_only, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, (const EslfExt*)ext, (u32)n, d_stats);
    launches += 2;
  } else {
    // stage 2: the fixed schedule.  Launch l reads ctl / part [l & 1] and writes [(l + 1) & 1].
    double* vec = (double*)e->vec.p;
    double** const slots[] = {&p.u0, &p.u1, &p.u2, &p.v, &p.w, &p.dx, &p.x[0], &p.x[1], &p.xold, &p.b0, &p.b1, &p.d0, &p.d1};
    for (size_t i = 0; i < N_VEC; ++i) *slots[i] = vec + i * total;
    p.y = d_mid;
    p.ctl[0] = (EslfCtl*)e->ctl.p, p.ctl[1] = p.ctl[0] + n;
    p.part[0] = (double*)e->part.p, p.part[1] = p.part[0] + n * 2 * n_tiles;
    p.trips = (uint8_t*)e->trips.p;
    HIP_TRY(hipMemsetAsync(p.x[0], 0, total * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(p.b0, 0, 4 * total * sizeof(double), stream));  // b0, b1, d0, d1 lie in a row
    HIP_TRY(hipMemsetAsync(p.ctl[0], 0, n * sizeof(EslfCtl), stream));
    HIP_TRY(hipMemsetAsync(p.trips, 0xFF, n * p.n_calls, stream));
    const dim3 grid((unsigned)n_tiles, m), block(BLOCK);
    int l = 0;
    u32 call = 0;
    for (u32 it = 0; it < e->niter_outer; ++it)
      for (u32 in = 0; in < e->niter_inner; ++in, ++call) {
        const int xsel = (int)(call & 1);
        hipLaunchKernelGGL(k_eslf_rhs, grid, block, 0, stream, p, l++ & 1, xsel, in == 0 ? 1 : 0, (int)it);
        hipLaunchKernelGGL(k_eslf_v0, grid, block, 0, stream, p, l++ & 1, call);
        for (u32 j = 1; j <= p.iter_lim; ++j) {
          hipLaunchKernelGGL(k_eslf_ustep, grid, block, 0, stream, p, l++ & 1, call);
          hipLaunchKernelGGL(k_eslf_vstep, grid, block, 0, stream, p, l++ & 1);
        }
        hipLaunchKernelGGL(k_eslf_ustep, grid, block, 0, stream, p, l++ & 1, call);
        hipLaunchKernelGGL(k_eslf_shrink, grid, block, 0, stream, p, l++ & 1, xsel, in + 1 == e->niter_inner ? 1 : 0);
      }
    hipLaunchKernelGGL(k_eslf_finish, grid, block, 0, stream, p, l++ & 1, (const EslfExt*)ext, d_out, d_stats);
    launches += (u64)l;
  }
  HIP_TRY(hipGetLastError());
  e->last_launches = launches;
  if (do_tv) c.back(trips_out, e->trips.p, n * p.n_calls);
  c.back(stats_out, d_stats, n * sizeof(EslfStats));
  return c.finish();
}

}  // extern "C"
