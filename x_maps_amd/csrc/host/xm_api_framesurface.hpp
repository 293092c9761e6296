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
  u64 n_max = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (offsets_host[f + 1] < offsets_host[f]) return fail(XM_ERR_INVALID, "offsets must not decrease (frame %d)", f);
    n_max = std::max<u64>(n_max, offsets_host[f + 1] - offsets_host[f]);
  }
  if (n_max >= 0xffffffffull) return fail(XM_ERR_TOO_MANY, "a frame holds at most 2^32 - 2 events");
  const u64 ev0 = offsets_host[0], n_total = offsets_host[n_frames] - ev0;
  if (n_total && !eventcd16) return fail(XM_ERR_INVALID, "NULL argument");
  const bool host = mem == XM_MEM_HOST;
  if (!host && ((uintptr_t)eventcd16 & 15)) return fail(XM_ERR_INVALID, "the record array must be 16-byte aligned");
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
                                                {sc.in, host ? (size_t)n_total * 16 : 0},
                                                {sc.out, host ? n * px * esz : 0}};
  // (new maps / accumulators are not zero yet -- noted before they are made, so that a call that fails below leaves the note)
  if (seq * stride * 4 > sc.maps.cap || seq * sizeof(FsAcc) > sc.acc.cap) sc.dirty = true;
  if (any_grows(needs) && sc.last_stream) {
    HIP_TRY(hipStreamSynchronize(sc.last_stream));
    sc.last_stream = nullptr;
  }
  if ((rc = reserve_all(needs))) return rc;
  if (!sc.done) HIP_TRY(sc.done.create());
  if (sc.last_stream && sc.last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, sc.done, 0));
  if (sc.dirty) {  // the zero invariant, established once -- and again behind a call that failed half way
    HIP_TRY(hipMemsetAsync(sc.maps.p, 0, sc.maps.cap, stream));
    HIP_TRY(hipMemsetAsync(sc.acc.p, 0, sc.acc.cap, stream));
    sc.dirty = false;
  }

  const uint4* d_ev = (const uint4*)eventcd16 + (host ? 0 : ev0);
  char* d_out = (char*)surfaces_out;
  FsStats* d_stats = (FsStats*)sc.stats.p;
  if (host) {
    if (n_total) HIP_TRY(hipMemcpyAsync(sc.in.p, (const uint4*)eventcd16 + ev0, (size_t)n_total * 16, hipMemcpyHostToDevice, stream));
    d_ev = (const uint4*)sc.in.p;
    d_out = (char*)sc.out.p;
  }
  sc.dirty = true;
  const u32 max_blocks = fs_max_chunk_blocks();
  for (size_t f0 = 0; f0 < n; f0 += FS_GROUP) {  // launch sequences of at most FS_GROUP frames; they reuse the maps in stream order
    const unsigned nf = (unsigned)std::min<size_t>(FS_GROUP, n - f0);
    FsArgs a{};
    a.ev = d_ev;
    u64 seq_max = 0;
    for (unsigned k = 0; k < nf; ++k) {
      a.first[k] = offsets_host[f0 + k] - ev0;
      a.n[k] = (u32)(offsets_host[f0 + k + 1] - offsets_host[f0 + k]);
      seq_max = std::max<u64>(seq_max, a.n[k]);
    }
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
  sc.dirty = false;
  s.order.note_eager();

  if (!host) {
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(FsStats), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipEventRecord(sc.done, stream));
    sc.last_stream = stream;
    return XM_OK;
  }
  HIP_TRY(hipMemcpyAsync(surfaces_out, d_out, n * px * esz, hipMemcpyDeviceToHost, stream));
  if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, d_stats, n * sizeof(FsStats), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  sc.last_stream = nullptr;
  return XM_OK;
}

}  // extern "C"
