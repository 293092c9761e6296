// xm_api_framesurface.hpp -- C-ABI: a group of frames of EventCD records -> one camera time surface per frame, in one device call
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
// The kernels, the definition's arithmetic and the zero invariant of the scratch: ../xmaps_framesurface.hpp.  The ingest runs the
// same launches as a stage of its frame stream (xm_ingest_launch.hpp, xm_api_ingest.hpp).
#pragma once

static_assert(sizeof(xm_frame_surface_stats) == sizeof(FsStats), "xm_frame_surface_stats is what k_fs_finish writes");
static_assert(XM_SURFACE_LAST == FS_SELECT_LAST && XM_SURFACE_FIRST == FS_SELECT_FIRST, "select values");

extern "C" {

int xm_frames_to_time_surfaces(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_polarity,
                               int select, int dtype, int mem, void* surfaces_out, xm_frame_surface_stats* stats_out) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  if (select != XM_SURFACE_LAST && select != XM_SURFACE_FIRST) return fail(XM_ERR_INVALID, "select must be XM_SURFACE_LAST or XM_SURFACE_FIRST");
  int rc;
  if ((rc = group_args(n_frames, mem, &dtype, "frames"))) return rc;
  if (!offsets_host || !surfaces_out) return fail(XM_ERR_INVALID, "NULL argument");
  FrameSpans sp;
  if ((rc = frame_spans(eventcd16, offsets_host, n_frames, mem, 0, "a frame holds at most 2^32 - 2 events", &sp))) return rc;
  const bool host = mem == XM_MEM_HOST;
  XM_ENTER(h);
  const DevTables& tb = h->tb;
  const size_t n = (size_t)n_frames, px = (size_t)tb.cam_w * tb.cam_h, esz = t_size(dtype);
  const size_t stride = (px + FS_CPT - 1) / FS_CPT * FS_CPT, seq = std::min<size_t>(n, FS_GROUP);
  if (px >= (1ull << 31) || n * px >= (1ull << 40)) return fail(XM_ERR_TOO_MANY, "group too large");
  FrameSurfScratch& sc = h->fsurf;
  Slot& s = pick_slot(h);
  hipStream_t stream = s.stream;

  // scratch: grown when a larger group arrives -- only once nothing that was enqueued earlier can still be using it
  const std::initializer_list<BufNeed> needs = {{sc.maps, seq * stride * 4},
                                                {sc.acc, seq * sizeof(FsAcc)},
                                                {sc.stats, n * sizeof(FsStats)},
                                                {sc.in, host ? (size_t)sp.n_total * 16 : 0},
                                                {sc.out, host ? n * px * esz : 0}};
  // (new maps / accumulators are not zero yet; the zero invariant, established once -- and again behind a call that failed half way)
  const bool zero_lost = seq * stride * 4 > sc.maps.cap || seq * sizeof(FsAcc) > sc.acc.cap;
  rc = sc.order.enter(
      stream, any_grows(needs), zero_lost, [&] { return reserve_all(needs); },
      [&] {
        HIP_TRY(hipMemsetAsync(sc.maps.p, 0, sc.maps.cap, stream));
        HIP_TRY(hipMemsetAsync(sc.acc.p, 0, sc.acc.cap, stream));
        return (int)XM_OK;
      });
  if (rc) return rc;

  const uint4* d_ev;
  if ((rc = frame_records(eventcd16, sp, host, sc.in, stream, &d_ev))) return rc;
  char* d_out = host ? (char*)sc.out.p : (char*)surfaces_out;
  FsStats* d_stats = (FsStats*)sc.stats.p;
  sc.order.launching();
  const u32 max_blocks = frame_max_chunk_blocks("XM_FS_MAX_BLOCKS");
  for (size_t f0 = 0; f0 < n; f0 += FS_GROUP) {  // launch sequences of at most FS_GROUP frames; they reuse the maps in stream order
    const unsigned nf = (unsigned)std::min<size_t>(FS_GROUP, n - f0);
    FsArgs a{};
    a.ev = d_ev;
    const u64 seq_max = frame_seq_fill(offsets_host, sp.ev0, f0, nf, a.first, a.n);
    a.map = (u32*)sc.maps.p;
    a.acc = (FsAcc*)sc.acc.p;
    a.stats = d_stats + f0;
    a.out = d_out + f0 * px * esz;
    a.cells = (u32)px, a.map_stride = (u32)stride;
    a.cam_w = tb.cam_w, a.cam_h = tb.cam_h;
    a.use_polarity = use_polarity ? 1 : 0, a.select = select;
    a.max_chunk_blocks = max_blocks;
    launch_frame_surfaces(a, nf, seq_max, dtype, stream);
    HIP_TRY(hipGetLastError());
  }
  sc.order.launched();
  s.order.note_eager();

  if (!host) {
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(FsStats), hipMemcpyDeviceToDevice, stream));
    return sc.order.leave_async(stream);
  }
  HIP_TRY(hipMemcpyAsync(surfaces_out, d_out, n * px * esz, hipMemcpyDeviceToHost, stream));
  if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(FsStats), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sc.order.leave_sync();
  return XM_OK;
}

}  // extern "C"
