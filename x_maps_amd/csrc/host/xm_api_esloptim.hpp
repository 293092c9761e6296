// xm_api_esloptim.hpp -- C-ABI: the ESL depth optimisation (a group of camera time surfaces + their depth_init maps -> depth_optim maps)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_esloptim.hpp.  No xm_handle: the object owns its device, stream, table and scratch.
#pragma once

static_assert(sizeof(xm_esl_optim_stats) == sizeof(EslOptStats), "xm_esl_optim_stats is what k_esl_optim_stats writes");

struct xm_esl_optim : GroupObj {
  EslOptTables tb{};
  DevMem<float> d_proj;
  DevBuf part1, cnt, stats;       // device-side intermediates of a group
  DevBuf in, d0, depth, nfev;     // staging of XM_MEM_HOST calls
};

namespace {

constexpr size_t ESLO_GRID_CAP = 65535;  // surfaces per launch: a grid's y and z dimensions end there

template <typename T>
void eslo_launch(const EslOptTables& tb, dim3 grid, hipStream_t stream, const T* surf, const float* d0, const SurfPart1* p1, u32 nb_red,
                 float* depth, uint16_t* nfev, EslOptCnt* cnt) {
  switch (tb.ws / 2) {
    case 0: hipLaunchKernelGGL((k_esl_optim<T, 0>), grid, dim3(BLOCK), 0, stream, surf, d0, tb, p1, nb_red, depth, nfev, cnt); break;
    case 1: hipLaunchKernelGGL((k_esl_optim<T, 1>), grid, dim3(BLOCK), 0, stream, surf, d0, tb, p1, nb_red, depth, nfev, cnt); break;
    case 2: hipLaunchKernelGGL((k_esl_optim<T, 2>), grid, dim3(BLOCK), 0, stream, surf, d0, tb, p1, nb_red, depth, nfev, cnt); break;
    default: hipLaunchKernelGGL((k_esl_optim<T, 3>), grid, dim3(BLOCK), 0, stream, surf, d0, tb, p1, nb_red, depth, nfev, cnt); break;
  }
}

EslOptPinhole eslo_pinhole(const double* K, const double* D) { return EslOptPinhole{K[0], K[4], K[2], K[5], D[0], D[1], D[2], D[3], D[4]}; }

}  // namespace

extern "C" {

void xm_esl_optim_destroy(xm_esl_optim* e) { group_destroy(e); }

int xm_esl_optim_create(int device, const xm_esl_optim_config* cfg, xm_esl_optim** out) {
  if (int rc = group_create_args(cfg, out, "xm_esl_optim_config")) return rc;
  if (!cfg->proj_surface) return fail(XM_ERR_INVALID, "NULL table");
  if (cfg->cam_width <= 0 || cfg->cam_height <= 0 || cfg->proj_width <= 0 || cfg->proj_height <= 0)
    return fail(XM_ERR_INVALID, "dimensions must be positive");
  if ((u64)cfg->cam_width * (u64)cfg->cam_height >= (1ull << 31) || (u64)cfg->proj_width * (u64)cfg->proj_height >= (1ull << 31))
    return fail(XM_ERR_INVALID, "frame too large");
  const int ws = cfg->window_size ? cfg->window_size : 3, max_iter = cfg->max_iter ? cfg->max_iter : 500;  // compute_depth_esl.py:151; scipy
  const double xatol = cfg->xatol != 0.0 ? cfg->xatol : 1e-5;
  if (ws < 1 || ws > ESLO_MAX_WS || ws % 2 == 0) return fail(XM_ERR_INVALID, "window_size must be odd and at most %d (got %d)", ESLO_MAX_WS, ws);
  if (max_iter < 1 || max_iter > 65535) return fail(XM_ERR_INVALID, "max_iter must lie in 1 .. 65535 (got %d)", max_iter);
  if (!(xatol > 0.0) || !std::isfinite(xatol)) return fail(XM_ERR_INVALID, "xatol must be positive and finite");
  if (!std::isfinite(cfg->p1_03) || cfg->p1_03 == 0.0) return fail(XM_ERR_INVALID, "p1_03 must be finite and non-zero");
  if (cfg->cam_width < 2 * ws + 1 || cfg->cam_height < 2 * ws + 1)
    return fail(XM_ERR_INVALID, "the camera must be at least 2 * window_size + 1 = %d pixels in either direction", 2 * ws + 1);
  bool finite = true;
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(cfg->cam_K[i]) && std::isfinite(cfg->proj_K[i]);
  for (int i = 0; i < 5; ++i) finite = finite && std::isfinite(cfg->cam_D[i]) && std::isfinite(cfg->proj_D[i]);
  for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(cfg->Rt[i]);
  if (!finite) return fail(XM_ERR_INVALID, "the calibration must be finite");
  if (cfg->cam_K[0] == 0.0 || cfg->cam_K[4] == 0.0) return fail(XM_ERR_INVALID, "the camera's focal lengths must not be zero");
  Owned<xm_esl_optim, xm_esl_optim_destroy> e;
  if (int rc = group_open(device, e)) return rc;
  e->px = (size_t)cfg->cam_width * cfg->cam_height;
  e->max_n = 0;  // (a group beyond ESLO_GRID_CAP goes in several launches)
  const size_t proj_px = (size_t)cfg->proj_width * cfg->proj_height;
  HIP_TRY(e->d_proj.alloc(proj_px));
  HIP_TRY(hipMemcpy(e->d_proj, cfg->proj_surface, proj_px * sizeof(float), hipMemcpyHostToDevice));
  EslOptTables& tb = e->tb;
  tb.proj = e->d_proj.get();
  tb.cam_w = cfg->cam_width, tb.cam_h = cfg->cam_height, tb.proj_w = cfg->proj_width, tb.proj_h = cfg->proj_height, tb.ws = ws;
  tb.max_iter = (u32)max_iter;
  tb.xatol = xatol, tb.p1_03 = cfg->p1_03;
  tb.sqrt_eps = std::sqrt(2.2e-16), tb.golden_mean = 0.5 * (3.0 - std::sqrt(5.0));  // (scipy's two constants, correctly rounded roots)
  tb.cam = eslo_pinhole(cfg->cam_K, cfg->cam_D), tb.prj = eslo_pinhole(cfg->proj_K, cfg->proj_D);
  for (int i = 0; i < 12; ++i) tb.Rt[i] = cfg->Rt[i];
  *out = e.release();
  return XM_OK;
}

int xm_esl_optim_time_surfaces(xm_esl_optim* e, const void* surfaces, int dtype, int n_surfaces, int mem, const float* depth_init,
                               float* depth_optim_out, uint16_t* nfev_out, xm_esl_optim_stats* stats_out) {
  if (int rc = group_enter(e, n_surfaces, mem, &dtype)) return rc;
  if (!surfaces || !depth_init || !depth_optim_out) return fail(XM_ERR_INVALID, "NULL argument");
  const EslOptTables& tb = e->tb;
  const size_t n = (size_t)n_surfaces, px = e->px, esz = t_size(dtype);
  const u32 nb_red = grid_for(px, SURF_RED_CHUNK);
  const u32 tiles_x = grid_for(tb.cam_w, ESLO_FW), tiles_y = grid_for(tb.cam_h, ESLO_FR), n_cnt = tiles_x * tiles_y;
  if (tiles_y > 65535) return fail(XM_ERR_INVALID, "camera frame too tall (at most %d rows)", 65535 * ESLO_FR);
  hipStream_t stream = e->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const char* d_in = (const char*)c.in(e->in, surfaces, n * px * esz);
  const float* d_d0 = c.in(e->d0, depth_init, n * px * 4);
  float* d_depth = c.out(e->depth, depth_optim_out, n * px * 4);
  uint16_t* d_nfev = c.out(e->nfev, nfev_out, n * px * 2);
  if (int rc = c.start({{e->part1, n * nb_red * sizeof(SurfPart1)}, {e->cnt, n * n_cnt * sizeof(EslOptCnt)}, {e->stats, n * sizeof(EslOptStats)}}))
    return rc;
  SurfPart1* p1 = (SurfPart1*)e->part1.p;
  EslOptCnt* cnt = (EslOptCnt*)e->cnt.p;
  EslOptStats* d_stats = (EslOptStats*)e->stats.p;
  for (size_t s0 = 0; s0 < n; s0 += ESLO_GRID_CAP) {  // a group beyond the grid's cap goes in several launches
    const unsigned m = (unsigned)(n - s0 < ESLO_GRID_CAP ? n - s0 : ESLO_GRID_CAP);
    const dim3 g_red(nb_red, m), g_px(tiles_x, tiles_y, m);
    SurfPart1* p1s = p1 + s0 * nb_red;
    EslOptCnt* cnts = cnt + s0 * n_cnt;
    uint16_t* nf = d_nfev ? d_nfev + s0 * px : nullptr;
    by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      const T* in = (const T*)(d_in + s0 * px * esz);
      hipLaunchKernelGGL((k_surf_extrema<T>), g_red, dim3(BLOCK), 0, stream, in, (u32)px, p1s);
      eslo_launch<T>(tb, g_px, stream, in, d_d0 + s0 * px, p1s, nb_red, d_depth + s0 * px, nf, cnts);
    });
    hipLaunchKernelGGL(k_esl_optim_stats, dim3(m), dim3(BLOCK), 0, stream, (const SurfPart1*)p1s, nb_red, (const EslOptCnt*)cnts, n_cnt,
                       d_stats + s0);
  }
  HIP_TRY(hipGetLastError());
  c.back(stats_out, d_stats, n * sizeof(EslOptStats));
  return c.finish();
}

}  // extern "C"
