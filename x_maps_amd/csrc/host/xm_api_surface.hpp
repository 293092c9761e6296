// xm_api_surface.hpp -- C-ABI: a group of camera time surfaces -> depth maps + per-event point clouds in one device call
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and what each stage does: ../xmaps_surface.hpp.
#pragma once

static_assert(sizeof(xm_surface_stats) == sizeof(SurfStats), "xm_surface_stats is what k_surf_scan writes");

extern "C" {

int xm_surface_set_cloud_tables(xm_handle* h, const float* mapx_f32, const float* mapy_f32, const double* Q) {
  if (!h || !mapx_f32 || !mapy_f32 || !Q) return fail(XM_ERR_INVALID, "NULL argument");
  if (h->cfg.view != XM_VIEW_CAMERA) return fail(XM_ERR_INVALID, "time surfaces need a camera-view handle (XM_VIEW_CAMERA)");
  XM_ENTER(h);
  SurfaceScratch& sc = h->surf;
  if (int rc = sc.order.settle()) return rc;  // a group in flight may still read the old tables
  sc.has_cloud_tables = false;
  const size_t px = (size_t)h->cfg.cam_width * h->cfg.cam_height;
  HIP_TRY(sc.mapx.alloc(px));
  HIP_TRY(sc.mapy.alloc(px));
  HIP_TRY(hipMemcpy(sc.mapx, mapx_f32, px * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sc.mapy, mapy_f32, px * 4, hipMemcpyHostToDevice));
  for (int i = 0; i < 16; ++i) sc.q.m[i] = (float)Q[i];  // self.Q.astype(np.float32), as xm_stage_point_cloud
  sc.has_cloud_tables = true;
  return XM_OK;
}

int xm_process_time_surfaces(xm_handle* h, const void* surfaces, int dtype, int n_surfaces, int mem, float* depth_out,
                             float* cloud_out, xm_surface_stats* stats_out) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  if (h->cfg.view != XM_VIEW_CAMERA) return fail(XM_ERR_INVALID, "time surfaces need a camera-view handle (XM_VIEW_CAMERA)");
  int rc;
  if ((rc = group_args(n_surfaces, mem, &dtype, "surfaces"))) return rc;
  if (!surfaces || !depth_out) return fail(XM_ERR_INVALID, "NULL argument");
  SurfaceScratch& sc = h->surf;
  if (cloud_out && !sc.has_cloud_tables)
    return fail(XM_ERR_INVALID, "cloud_out needs the float rectify maps and Q: call xm_surface_set_cloud_tables first");
  XM_ENTER(h);
  const DevTables& tb = h->tb;
  const size_t n = (size_t)n_surfaces, px = (size_t)tb.cam_w * tb.cam_h, esz = t_size(dtype);
  const u32 nb_red = grid_for(px, SURF_RED_CHUNK);
  const u32 tiles_x = grid_for(tb.cam_w, SURF_TW), tiles_y = grid_for(tb.cam_h, SURF_TR);
  const u32 n_seg = (u32)tb.cam_h * tiles_x, n_wo = tiles_x * tiles_y * (BLOCK / 64);
  if (n * px >= (1ull << 40) || n > 65535 || tiles_y > 65535)
    return fail(XM_ERR_TOO_MANY, "group too large (at most 65535 surfaces per call)");
  Slot& s = pick_slot(h);
  hipStream_t stream = s.stream;
  const bool host = mem == XM_MEM_HOST;

  // scratch: grown when a larger group arrives -- only once nothing that was enqueued earlier can still be using it
  const std::initializer_list<BufNeed> needs = {{sc.part1, n * nb_red * sizeof(SurfPart1)},
                                                {sc.part2, n * nb_red * sizeof(SurfPart2)},
                                                {sc.seg_cnt, n * n_seg * 4},
                                                {sc.seg_off, n * n_seg * 4},
                                                {sc.wave_oob, n * n_wo * 4},
                                                {sc.code, cloud_out ? n * px * 2 : 0},
                                                {sc.stats, n * sizeof(SurfStats)},
                                                {sc.in, host ? n * px * esz : 0},
                                                {sc.depth, host ? n * px * 4 : 0},
                                                {sc.cloud, host && cloud_out ? n * px * 12 : 0}};
  if ((rc = sc.order.enter(stream, any_grows(needs), false, [&] { return reserve_all(needs); }, [] { return 0; }))) return rc;

  const void* d_in = surfaces;
  float* d_depth = depth_out;
  float* d_cloud = cloud_out;
  SurfStats* d_stats = (SurfStats*)sc.stats.p;
  if (host) {
    HIP_TRY(hipMemcpyAsync(sc.in.p, surfaces, n * px * esz, hipMemcpyHostToDevice, stream));
    d_in = sc.in.p;
    d_depth = (float*)sc.depth.p;
    if (cloud_out) d_cloud = (float*)sc.cloud.p;
  }
  const dim3 g_red(nb_red, (unsigned)n), g_px(tiles_x, tiles_y, (unsigned)n);
  SurfPart1* p1 = (SurfPart1*)sc.part1.p;
  SurfPart2* p2 = (SurfPart2*)sc.part2.p;
  u32 *seg_cnt = (u32*)sc.seg_cnt.p, *seg_off = (u32*)sc.seg_off.p, *wave_oob = (u32*)sc.wave_oob.p;
  uint16_t* code = (uint16_t*)sc.code.p;
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    XM_LAUNCH((k_surf_extrema<T>), g_red, dim3(BLOCK), 0, stream, (const T*)d_in, (u32)px, p1);
    XM_LAUNCH((k_surf_norm_extrema<T>), g_red, dim3(BLOCK), 0, stream, (const T*)d_in, (u32)px, (const SurfPart1*)p1, p2);
    if (cloud_out)
      XM_LAUNCH((k_surf_pixels<T, true>), g_px, dim3(BLOCK), 0, stream, (const T*)d_in, tb, (const SurfPart2*)p2, nb_red, d_depth, code,
                seg_cnt, wave_oob);
    else
      XM_LAUNCH((k_surf_pixels<T, false>), g_px, dim3(BLOCK), 0, stream, (const T*)d_in, tb, (const SurfPart2*)p2, nb_red, d_depth,
                (uint16_t*)nullptr, seg_cnt, wave_oob);
  });
  HIP_TRY(hipGetLastError());
  XM_LAUNCH(k_surf_scan, dim3((unsigned)n), dim3(SURF_SCAN_BLOCK), 0, stream, (const u32*)seg_cnt, n_seg, (const u32*)wave_oob, n_wo,
            (const SurfPart2*)p2, nb_red, seg_off, d_stats);
  if (cloud_out)
    XM_LAUNCH(k_surf_cloud, dim3(grid_for(n_seg, BLOCK / 64), (unsigned)n), dim3(BLOCK), 0, stream, (const uint16_t*)code,
              (const u32*)seg_off, tb.cam_w, tb.cam_h, tiles_x, (const float*)sc.mapx.get(), (const float*)sc.mapy.get(), sc.q, d_cloud);
  HIP_TRY(hipGetLastError());
  s.order.note_eager();

  if (!host) {
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(SurfStats), hipMemcpyDeviceToDevice, stream));
    return sc.order.leave_async(stream);
  }
  std::vector<xm_surface_stats> st(n);
  HIP_TRY(hipMemcpyAsync(depth_out, d_depth, n * px * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(st.data(), d_stats, n * sizeof(SurfStats), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sc.order.leave_sync();
  if (cloud_out) {  // only the valid rows of every surface cross the bus
    for (size_t i = 0; i < n; ++i)
      if (st[i].n_inliers)
        HIP_TRY(hipMemcpyAsync(cloud_out + i * px * 3, d_cloud + i * px * 3, (size_t)st[i].n_inliers * 12, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (stats_out) std::memcpy(stats_out, st.data(), n * sizeof(xm_surface_stats));
  return XM_OK;
}

}  // extern "C"
