// xm_api_eslinit.hpp -- C-ABI: the ESL-init baseline (a group of camera time surfaces -> depth_init maps; disparity_init alone)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_eslinit.hpp.  No xm_handle: the object owns its device, stream, tables and scratch.
#pragma once

static_assert(sizeof(xm_esl_init_stats) == sizeof(EslStats), "xm_esl_init_stats is what k_esl_stats writes");

struct xm_esl_init {
  int device = 0;
  Stream stream;  // (before the buffers: released after them)
  EslTables tb{};
  DevMem<short2> d_rect_to_cam, d_cam_to_rect;
  DevMem<float> d_proj_rect;
  DevBuf part1, cnt, stats;    // device-side intermediates of a group
  DevBuf in, depth, disp;      // staging of XM_MEM_HOST calls
  DevBuf st_cam, st_disp;      // xm_esl_init_stage_disparity
};

extern "C" {

void xm_esl_init_destroy(xm_esl_init* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  delete e;
}

int xm_esl_init_create(int device, const xm_esl_init_config* cfg, xm_esl_init** out) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(xm_esl_init_config)) return fail(XM_ERR_INVALID, "xm_esl_init_config.struct_size mismatch");
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(XM_ERR_HIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(XM_ERR_INVALID, "no device %d", device);
  HIP_TRY(hipSetDevice(device));
  Owned<xm_esl_init, xm_esl_init_destroy> e(new (std::nothrow) xm_esl_init);
  if (!e) return fail(XM_ERR_NOMEM, "out of host memory");
  e->device = device;
  HIP_TRY(e->stream.create());
  const size_t cam_px = (size_t)cfg->cam_width * cfg->cam_height, rect_px = (size_t)cfg->rect_width * cfg->rect_height;
  HIP_TRY(e->d_rect_to_cam.alloc(cam_px));
  HIP_TRY(e->d_cam_to_rect.alloc(rect_px));
  HIP_TRY(e->d_proj_rect.alloc(rect_px));
  HIP_TRY(hipMemcpy(e->d_rect_to_cam, cfg->rect_to_cam_map, cam_px * sizeof(short2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_cam_to_rect, cfg->cam_to_rect_map, rect_px * sizeof(short2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(e->d_proj_rect, cfg->proj_rect, rect_px * sizeof(float), hipMemcpyHostToDevice));
  e->tb = EslTables{e->d_rect_to_cam.get(), e->d_cam_to_rect.get(), e->d_proj_rect.get(), cfg->cam_width, cfg->cam_height,
                    cfg->rect_width, cfg->rect_height, min_disp, max_disp, cfg->p1_03};
  *out = e.release();
  return XM_OK;
}

int xm_esl_init_time_surfaces(xm_esl_init* e, const void* surfaces, int dtype, int n_surfaces, int mem, float* depth_out,
                              uint16_t* disp_cam_out, xm_esl_init_stats* stats_out) {
  if (!e) return fail(XM_ERR_INVALID, "NULL object");
  if (dtype != XM_T_FLOAT32 && dtype != XM_T_FLOAT64) return fail(XM_ERR_INVALID, "a time surface is XM_T_FLOAT32 or XM_T_FLOAT64");
  if (n_surfaces <= 0) return fail(XM_ERR_INVALID, "n_surfaces must be positive");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  if (!surfaces || !depth_out) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  const EslTables& tb = e->tb;
  const size_t n = (size_t)n_surfaces, px = (size_t)tb.cam_w * tb.cam_h, esz = t_size(dtype);
  const u32 nb_red = grid_for(px, SURF_RED_CHUNK);
  const u32 tiles_x = grid_for(tb.cam_w, ESL_FW), tiles_y = grid_for(tb.cam_h, ESL_FR), n_cnt = tiles_x * tiles_y;
  if (n > 65535 || n * px >= (1ull << 40)) return fail(XM_ERR_TOO_MANY, "group too large (at most 65535 surfaces per call)");
  hipStream_t stream = e->stream;
  const bool host = mem == XM_MEM_HOST;
  const size_t need[] = {n * nb_red * sizeof(SurfPart1), n * n_cnt * sizeof(uint2), n * sizeof(EslStats), host ? n * px * esz : 0,
                         host ? n * px * 4 : 0, host && disp_cam_out ? n * px * 2 : 0};
  DevBuf* const bufs[] = {&e->part1, &e->cnt, &e->stats, &e->in, &e->depth, &e->disp};
  int rc;
  for (int i = 0; i < 6; ++i)  // (every call is synchronous: nothing in flight can still use a buffer that grows)
    if (need[i] && (rc = bufs[i]->reserve(need[i]))) return rc;

  const void* d_in = surfaces;
  float* d_depth = depth_out;
  uint16_t* d_disp = disp_cam_out;
  if (host) {
    HIP_TRY(hipMemcpyAsync(e->in.p, surfaces, n * px * esz, hipMemcpyHostToDevice, stream));
    d_in = e->in.p;
    d_depth = (float*)e->depth.p;
    if (disp_cam_out) d_disp = (uint16_t*)e->disp.p;
  }
  SurfPart1* p1 = (SurfPart1*)e->part1.p;
  uint2* cnt = (uint2*)e->cnt.p;
  EslStats* d_stats = (EslStats*)e->stats.p;
  const dim3 g_red(nb_red, (unsigned)n), g_px(tiles_x, tiles_y, (unsigned)n);
  if (dtype == XM_T_FLOAT32) {
    hipLaunchKernelGGL((k_surf_extrema<float>), g_red, dim3(BLOCK), 0, stream, (const float*)d_in, (u32)px, p1);
    hipLaunchKernelGGL((k_esl_fused<float>), g_px, dim3(BLOCK), 0, stream, (const float*)d_in, tb, (const SurfPart1*)p1, nb_red, d_depth,
                       d_disp, cnt);
  } else {
    hipLaunchKernelGGL((k_surf_extrema<double>), g_red, dim3(BLOCK), 0, stream, (const double*)d_in, (u32)px, p1);
    hipLaunchKernelGGL((k_esl_fused<double>), g_px, dim3(BLOCK), 0, stream, (const double*)d_in, tb, (const SurfPart1*)p1, nb_red,
                       d_depth, d_disp, cnt);
  }
  hipLaunchKernelGGL(k_esl_stats, dim3((unsigned)n), dim3(BLOCK), 0, stream, (const SurfPart1*)p1, nb_red, (const uint2*)cnt, n_cnt,
                     d_stats);
  HIP_TRY(hipGetLastError());
  if (host) {
    HIP_TRY(hipMemcpyAsync(depth_out, d_depth, n * px * 4, hipMemcpyDeviceToHost, stream));
    if (disp_cam_out) HIP_TRY(hipMemcpyAsync(disp_cam_out, d_disp, n * px * 2, hipMemcpyDeviceToHost, stream));
  }
  if (stats_out)
    HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(EslStats), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return XM_OK;
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
