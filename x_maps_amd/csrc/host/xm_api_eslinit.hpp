// xm_api_eslinit.hpp -- C-ABI: the ESL-init baseline (a group of camera time surfaces -> depth_init maps; disparity_init alone)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_eslinit.hpp.  No xm_handle: the object owns its device, stream, tables and scratch.
#pragma once

static_assert(sizeof(xm_esl_init_stats) == sizeof(EslStats), "xm_esl_init_stats is what k_esl_stats writes");

struct xm_esl_init : GroupObj {
  EslTables tb{};
  DevMem<short2> d_rect_to_cam, d_cam_to_rect;
  DevMem<float> d_proj_rect;
  DevBuf part1, cnt, stats;    // device-side intermediates of a group
  DevBuf in, depth, disp;      // staging of XM_MEM_HOST calls
  DevBuf st_cam, st_disp;      // xm_esl_init_stage_disparity
};

extern "C" {

void xm_esl_init_destroy(xm_esl_init* e) { group_destroy(e); }

int xm_esl_init_create(int device, const xm_esl_init_config* cfg, xm_esl_init** out) {
  if (int rc = group_create_args(cfg, out, "xm_esl_init_config")) return rc;
  if (!cfg->cam_to_rect_map || !cfg->rect_to_cam_map || !cfg->proj_rect) return fail(XM_ERR_INVALID, "NULL table");
  if (cfg->cam_width <= 0 || cfg->cam_height <= 0 || cfg->rect_width <= 0 || cfg->rect_height <= 0)
    return fail(XM_ERR_INVALID, "dimensions must be positive");
  // the maps are int16 pairs: nothing beyond 32767 can be addressed; rows of a grid dimension
  if (cfg->cam_width > 32768 || cfg->cam_height > 32768 || cfg->rect_width > 32768 || cfg->rect_height > 32768)
    return fail(XM_ERR_INVALID, "dimensions must fit the int16 maps (at most 32768)");
  if ((u64)cfg->cam_width * (u64)cfg->cam_height >= (1ull << 31)) return fail(XM_ERR_INVALID, "camera frame too large");
  int min_disp = cfg->min_disp, max_disp = cfg->max_disp;
  if (min_disp == 0 && max_disp == 0) min_disp = 5, max_disp = 900;  // compute_depth_esl.py:74
  if (min_disp < 0 || max_disp <= min_disp || max_disp > 65535)
    return fail(XM_ERR_INVALID, "need 0 <= min_disp < max_disp <= 65535 (got %d, %d)", min_disp, max_disp);
  Owned<xm_esl_init, xm_esl_init_destroy> e;
  if (int rc = group_open(device, e)) return rc;
  const size_t cam_px = (size_t)cfg->cam_width * cfg->cam_height, rect_px = (size_t)cfg->rect_width * cfg->rect_height;
  HIP_TRY(e->d_rect_to_cam.alloc(cam_px));
  HIP_TRY(e->d_cam_to_rect.alloc(rect_px));
  HIP_TRY(e->d_proj_rect.alloc(rect_px));
  HIP_TRY(hipMemcpy(e->d_rect_to_cam, cfg->rect_to_cam_map, cam_px * sizeof(short2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_cam_to_rect, cfg->cam_to_rect_map, rect_px * sizeof(short2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_proj_rect, cfg->proj_rect, rect_px * sizeof(float), hipMemcpyHostToDevice));
  e->tb = EslTables{e->d_rect_to_cam.get(), e->d_cam_to_rect.get(), e->d_proj_rect.get(), cfg->cam_width, cfg->cam_height,
                    cfg->rect_width, cfg->rect_height, min_disp, max_disp, cfg->p1_03};
  e->px = cam_px;
  *out = e.release();
  return XM_OK;
}

int xm_esl_init_time_surfaces(xm_esl_init* e, const void* surfaces, int dtype, int n_surfaces, int mem, float* depth_out,
                              uint16_t* disp_cam_out, xm_esl_init_stats* stats_out) {
  if (int rc = group_enter(e, n_surfaces, mem, &dtype)) return rc;
  if (!surfaces || !depth_out) return fail(XM_ERR_INVALID, "NULL argument");
  const EslTables& tb = e->tb;
  const size_t n = (size_t)n_surfaces, px = e->px;
  const u32 nb_red = grid_for(px, SURF_RED_CHUNK);
  const u32 tiles_x = grid_for(tb.cam_w, ESL_FW), tiles_y = grid_for(tb.cam_h, ESL_FR), n_cnt = tiles_x * tiles_y;
  hipStream_t stream = e->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const void* d_in = c.in(e->in, surfaces, n * px * t_size(dtype));
  float* d_depth = c.out(e->depth, depth_out, n * px * 4);
  uint16_t* d_disp = c.out(e->disp, disp_cam_out, n * px * 2);
  if (int rc = c.start({{e->part1, n * nb_red * sizeof(SurfPart1)}, {e->cnt, n * n_cnt * sizeof(uint2)}, {e->stats, n * sizeof(EslStats)}}))
    return rc;
  SurfPart1* p1 = (SurfPart1*)e->part1.p;
  uint2* cnt = (uint2*)e->cnt.p;
  EslStats* d_stats = (EslStats*)e->stats.p;
  const dim3 g_red(nb_red, (unsigned)n), g_px(tiles_x, tiles_y, (unsigned)n);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_surf_extrema<T>), g_red, dim3(BLOCK), 0, stream, (const T*)d_in, (u32)px, p1);
    hipLaunchKernelGGL((k_esl_fused<T>), g_px, dim3(BLOCK), 0, stream, (const T*)d_in, tb, (const SurfPart1*)p1, nb_red, d_depth, d_disp,
                       cnt);
  });
  hipLaunchKernelGGL(k_esl_stats, dim3((unsigned)n), dim3(BLOCK), 0, stream, (const SurfPart1*)p1, nb_red, (const uint2*)cnt, n_cnt,
                     d_stats);
  HIP_TRY(hipGetLastError());
  c.back(stats_out, d_stats, n * sizeof(EslStats));
  return c.finish();
}

int xm_esl_init_stage_disparity(xm_esl_init* e, const double* cam_rect_host, uint16_t* disparity_rect_out) {
  if (!e || !cam_rect_host || !disparity_rect_out) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  const EslTables& tb = e->tb;
  const size_t rect_px = (size_t)tb.rect_w * tb.rect_h;
  int rc;
  if ((rc = e->st_cam.reserve(rect_px * sizeof(double))) || (rc = e->st_disp.reserve(rect_px * sizeof(uint16_t)))) return rc;
  hipStream_t stream = e->stream;
  HIP_TRY(hipMemcpyAsync(e->st_cam.p, cam_rect_host, rect_px * sizeof(double), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(k_esl_stage, dim3(grid_for(tb.rect_w, ESL_TX), (unsigned)tb.rect_h), dim3(BLOCK), 0, stream,
                     (const double*)e->st_cam.p, tb.proj_rect, tb.rect_w, tb.min_disp, tb.max_disp, (uint16_t*)e->st_disp.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(disparity_rect_out, e->st_disp.p, rect_px * sizeof(uint16_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return XM_OK;
}

}  // extern "C"
