// xm_api_mc3d.hpp -- C-ABI: the MC3D baseline (a group of camera time surfaces -> depth maps of python/eval/mc3d_baseline.py)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and the arithmetic: ../xmaps_mc3d.hpp.  No xm_handle: the object owns its device, stream, tables and scratch.
#pragma once

static_assert(sizeof(xm_mc3d_stats) == sizeof(Mc3dStats), "xm_mc3d_stats is what k_mc3d_stats writes");
static_assert(XM_MC3D_POISON == MC3D_POISON && XM_MC3D_NO_BLUR == MC3D_NO_BLUR, "xmaps.h and xmaps_geometry.hpp agree");

struct xm_mc3d : GroupObj {
  Mc3dTables tb{};
  DevMem<int2> d_cam_map;
  DevMem<int> d_yp_t, d_xp_t;
  DevBuf cnt, stats;       // device-side intermediates of a group
  DevBuf in, depth, disp;  // staging of XM_MEM_HOST calls
};

extern "C" {

void xm_mc3d_destroy(xm_mc3d* m) { group_destroy(m); }

int xm_mc3d_create(int device, const xm_mc3d_config* cfg, xm_mc3d** out) {
  if (int rc = group_create_args(cfg, out, "xm_mc3d_config")) return rc;
  if (!cfg->cam_map || !cfg->proj_map) return fail(XM_ERR_INVALID, "NULL table");
  if (cfg->cam_width <= 0 || cfg->cam_height <= 0 || cfg->proj_width <= 0 || cfg->proj_height <= 0)
    return fail(XM_ERR_INVALID, "dimensions must be positive");
  if ((u64)cfg->cam_width * (u64)cfg->cam_height >= (1ull << 31)) return fail(XM_ERR_INVALID, "camera frame too large");
  const u64 proj_px = (u64)cfg->proj_width * (u64)cfg->proj_height;
  if (proj_px > (1ull << 24))  // float32(W * H) * v must have its first factor exact, and the ids fit a float32's integers
    return fail(XM_ERR_INVALID, "proj_width * proj_height must not exceed 2^24 (got %llu)", (unsigned long long)proj_px);
  const int W = cfg->proj_width, H = cfg->proj_height;
  const int nc = cfg->nc ? cfg->nc : H / 15, mrd = cfg->max_row_diff ? cfg->max_row_diff : 50;  // mc3d_baseline.py:43-45, :71
  if (nc < 0 || 2 * (long long)nc > H) return fail(XM_ERR_INVALID, "need 0 <= 2 * nc <= proj_height (got nc %d)", nc);
  if (mrd < 0 || mrd > MC3D_SAT / 2) return fail(XM_ERR_INVALID, "max_row_diff must lie in 0 .. 2^29");
  int x_lim = cfg->rect_x_limit, y_lim = cfg->rect_y_limit;
  if (x_lim == 0 && y_lim == 0) x_lim = 3 * H, y_lim = 3 * W;  // (:100 with :54-56: swapped, as the reference)
  if (x_lim <= 0 || y_lim <= 0 || x_lim > MC3D_SAT / 2 || y_lim > MC3D_SAT / 2)  // (half the saturation bound: xmaps.h says why)
    return fail(XM_ERR_INVALID, "rect limits must lie in 1 .. 2^29 (got %d, %d)", x_lim, y_lim);
  if (!mc3d_key_fits((u32)mrd, 2u * (u32)nc))
    return fail(XM_ERR_INVALID, "(max_row_diff + 2) * the window's size rounded up to a power of two must stay below 2^32");
  Owned<xm_mc3d, xm_mc3d_destroy> m;
  if (int rc = group_open(device, m)) return rc;
  const size_t cam_px = (size_t)cfg->cam_width * cfg->cam_height;
  // the tables as the kernel reads them: saturated, the projector's by (proj_x, y) with poison folded into yp
  auto sat = [](int32_t v) { return v == MC3D_POISON ? v : v > MC3D_SAT ? MC3D_SAT : v < -MC3D_SAT ? -MC3D_SAT : v; };
  std::vector<int32_t> cam, yp_t, xp_t;
  try {
    cam.resize(cam_px * 2), yp_t.resize(proj_px), xp_t.resize(proj_px);
  } catch (const std::bad_alloc&) {
    return fail(XM_ERR_NOMEM, "out of host memory");
  }
  for (size_t i = 0; i < cam_px * 2; ++i) cam[i] = sat(cfg->cam_map[i]);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int32_t xp = cfg->proj_map[((size_t)y * W + x) * 2], yp = cfg->proj_map[((size_t)y * W + x) * 2 + 1];
      const bool poison = xp == MC3D_POISON || yp == MC3D_POISON;
      yp_t[(size_t)x * H + y] = poison ? MC3D_POISON : sat(yp);
      xp_t[(size_t)x * H + y] = poison ? 0 : sat(xp);
    }
  HIP_TRY(m->d_cam_map.alloc(cam_px));
  HIP_TRY(m->d_yp_t.alloc(proj_px));
  HIP_TRY(m->d_xp_t.alloc(proj_px));
  HIP_TRY(hipMemcpy(m->d_cam_map, cam.data(), cam_px * sizeof(int2), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->d_yp_t, yp_t.data(), proj_px * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(m->d_xp_t, xp_t.data(), proj_px * sizeof(int), hipMemcpyHostToDevice));
  m->tb = Mc3dTables{m->d_cam_map.get(), m->d_yp_t.get(), m->d_xp_t.get(), cfg->cam_width, cfg->cam_height, W, H, nc, mrd, x_lim, y_lim,
                     mc3d_pos_bits(2u * (u32)nc), cfg->p1_03};
  m->px = cam_px;
  *out = m.release();
  return XM_OK;
}

int xm_mc3d_time_surfaces(xm_mc3d* m, const void* surfaces, int dtype, int n_surfaces, int mem, int flags, float* depth_out,
                          uint16_t* disp_out, xm_mc3d_stats* stats_out) {
  if (int rc = group_enter(m, n_surfaces, mem, &dtype)) return rc;
  if (flags & ~(int)XM_MC3D_NO_BLUR) return fail(XM_ERR_INVALID, "unknown flags");
  if (!surfaces || !depth_out) return fail(XM_ERR_INVALID, "NULL argument");
  const Mc3dTables& tb = m->tb;
  const size_t n = (size_t)n_surfaces, px = m->px;
  const u32 tiles_x = grid_for(tb.cam_w, MC3D_FW), tiles_y = grid_for(tb.cam_h, MC3D_FR), n_cnt = tiles_x * tiles_y;
  if (tiles_y > 65535) return fail(XM_ERR_INVALID, "camera frame too tall (at most %d rows)", 65535 * MC3D_FR);
  hipStream_t stream = m->stream;
  GroupCall c{stream, mem == XM_MEM_HOST};
  const void* d_in = c.in(m->in, surfaces, n * px * t_size(dtype));
  float* d_depth = c.out(m->depth, depth_out, n * px * 4);
  uint16_t* d_disp = c.out(m->disp, disp_out, n * px * 2);
  if (int rc = c.start({{m->cnt, n * n_cnt * sizeof(Mc3dCnt)}, {m->stats, n * sizeof(Mc3dStats)}})) return rc;
  Mc3dCnt* cnt = (Mc3dCnt*)m->cnt.p;
  Mc3dStats* d_stats = (Mc3dStats*)m->stats.p;
  const dim3 g_px(tiles_x, tiles_y, (unsigned)n);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_mc3d<T>), g_px, dim3(BLOCK), 0, stream, (const T*)d_in, tb, (u32)flags, d_depth, d_disp, cnt);
  });
  hipLaunchKernelGGL(k_mc3d_stats, dim3((unsigned)n), dim3(BLOCK), 0, stream, (const Mc3dCnt*)cnt, n_cnt, d_stats);
  HIP_TRY(hipGetLastError());
  c.back(stats_out, d_stats, n * sizeof(Mc3dStats));
  return c.finish();
}

}  // extern "C"
