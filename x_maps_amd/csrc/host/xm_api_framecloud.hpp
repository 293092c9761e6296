// xm_api_framecloud.hpp -- C-ABI: a group of frames of EventCD records -> one per-event point cloud per frame, in one device call
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels and what each pass leaves behind: ../xmaps_framecloud.hpp.  The ingest runs the same launches as a stage of its
// frame stream (xm_ingest_launch.hpp, xm_api_ingest.hpp) and reads the tables set here.
#pragma once

static_assert(sizeof(xm_frame_cloud_stats) == sizeof(FcStats), "xm_frame_cloud_stats is what k_fc_scan writes");

extern "C" {

int xm_cloud_set_tables(xm_handle* h, const float* mapx_f32, const float* mapy_f32, const double* Q) {
  if (!h || !mapx_f32 || !mapy_f32 || !Q) return fail(XM_ERR_INVALID, "NULL argument");
  XM_ENTER(h);
  FrameCloudScratch& sc = h->fcloud;
  if (int rc = sc.order.settle()) return rc;  // a group in flight may still read the old tables
  const size_t px = (size_t)h->cfg.cam_width * h->cfg.cam_height;
  if (sc.has_tables) {  // (same sizes: rewritten in place, so that an ingest's cloud stage keeps valid pointers)
    HIP_TRY(hipDeviceSynchronize());
  } else {
    HIP_TRY(sc.mapx.alloc(px));
    HIP_TRY(sc.mapy.alloc(px));
  }
  HIP_TRY(hipMemcpy(sc.mapx, mapx_f32, px * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(sc.mapy, mapy_f32, px * 4, hipMemcpyHostToDevice));
  for (int i = 0; i < 16; ++i) sc.q.m[i] = (float)Q[i];  // self.Q.astype(np.float32), as xm_stage_point_cloud
  sc.has_tables = true;
  return XM_OK;
}

int xm_frames_to_point_clouds(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_polarity,
                              int mem, float* cloud_out, xm_frame_cloud_stats* stats_out) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = group_args(n_frames, mem, nullptr, "frames"))) return rc;
  if (!offsets_host) return fail(XM_ERR_INVALID, "NULL argument");
  FrameCloudScratch& sc = h->fcloud;
  if (cloud_out && !sc.has_tables)
    return fail(XM_ERR_INVALID, "cloud_out needs the float rectify maps and Q: call xm_cloud_set_tables first");
  FrameSpans sp;
  if ((rc = frame_spans(eventcd16, offsets_host, n_frames, mem, 1ull << 36, "group too large (a frame holds at most 2^32 - 2 events)", &sp)))
    return rc;
  const u64 ev0 = sp.ev0, n_total = sp.n_total;
  const bool host = mem == XM_MEM_HOST;
  XM_ENTER(h);
  const size_t n = (size_t)n_frames, seq = std::min<size_t>(n, FC_GROUP);
  const size_t n_seg = (size_t)(n_total / 64) + n;  // >= the frames' ceil(n / 64) together
  Slot& s = pick_slot(h);
  hipStream_t stream = s.stream;

  // scratch: grown when a larger group arrives -- only once nothing that was enqueued earlier can still be using it
  const std::initializer_list<BufNeed> needs = {{sc.acc, seq * sizeof(FcAcc)},
                                                {sc.code, (size_t)n_total * 2},
                                                {sc.cnt, n_seg * sizeof(uint2)},
                                                {sc.off, n_seg * 4},
                                                {sc.stats, n * sizeof(FcStats)},
                                                {sc.in, host ? (size_t)n_total * 16 : 0},
                                                {sc.out, host && cloud_out ? (size_t)n_total * 12 : 0}};
  // (new accumulators are not zero yet; the zero invariant, established once -- and again behind a call that failed half way)
  rc = sc.order.enter(
      stream, any_grows(needs), seq * sizeof(FcAcc) > sc.acc.cap, [&] { return reserve_all(needs); },
      [&] {
        HIP_TRY(hipMemsetAsync(sc.acc.p, 0, sc.acc.cap, stream));
        return (int)XM_OK;
      });
  if (rc) return rc;

  const uint4* d_ev;
  if ((rc = frame_records(eventcd16, sp, host, sc.in, stream, &d_ev))) return rc;
  float* d_cloud = host && cloud_out ? (float*)sc.out.p : cloud_out;
  FcStats* d_stats = (FcStats*)sc.stats.p;
  sc.order.launching();
  const u32 max_blocks = frame_max_chunk_blocks("XM_FC_MAX_BLOCKS");
  u64 seg = 0;
  for (size_t f0 = 0; f0 < n; f0 += FC_GROUP) {  // launch sequences of at most FC_GROUP frames
    const unsigned nf = (unsigned)std::min<size_t>(FC_GROUP, n - f0);
    FcArgs a{};
    a.ev = d_ev;
    const u64 seq_max = frame_seq_fill(offsets_host, ev0, f0, nf, a.first, a.n);
    for (unsigned k = 0; k < nf; ++k) {
      a.seg0[k] = (u32)seg;
      seg += ((u64)a.n[k] + 63) / 64;
    }
    a.max_rows = 0xffffffffu;
    a.tb = h->tb;
    a.mapx = sc.mapx.get(), a.mapy = sc.mapy.get(), a.Q = sc.q;
    a.acc = (FcAcc*)sc.acc.p;
    a.code = (uint16_t*)sc.code.p;
    a.cnt = (uint2*)sc.cnt.p;
    a.off = (u32*)sc.off.p;
    a.stats = d_stats + f0;
    a.cloud = d_cloud;
    a.use_polarity = use_polarity ? 1 : 0;
    a.max_chunk_blocks = max_blocks;
    launch_frame_clouds(a, nf, seq_max, stream);
    HIP_TRY(hipGetLastError());
  }
  sc.order.launched();
  s.order.note_eager();

  if (!host) {
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(FcStats), hipMemcpyDeviceToDevice, stream));
    return sc.order.leave_async(stream);
  }
  std::vector<xm_frame_cloud_stats> st(n);
  HIP_TRY(hipMemcpyAsync(st.data(), d_stats, n * sizeof(FcStats), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sc.order.leave_sync();
  if (cloud_out) {  // only the valid rows of every frame cross the bus
    for (size_t i = 0; i < n; ++i) {
      const size_t row0 = (size_t)(offsets_host[i] - ev0) * 3;
      if (st[i].n_inliers)
        HIP_TRY(hipMemcpyAsync(cloud_out + row0, d_cloud + row0, (size_t)st[i].n_inliers * 12, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (stats_out) std::memcpy(stats_out, st.data(), n * sizeof(xm_frame_cloud_stats));
  return XM_OK;
}

}  // extern "C"
