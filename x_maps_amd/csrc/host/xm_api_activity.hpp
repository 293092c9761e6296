// xm_api_activity.hpp -- C-ABI: the activity filter alone (xm_activity_*), and the allocation of its device state, which the
// device-side ingest shares (xm_api_ingest.hpp)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

struct ActMem {  // owner of the activity filter's device state (xmaps_ingest.hpp: ActDev holds the views the kernels take)
  DevMem<long long> last_ts; DevMem<uint2> cells;
  DevMem<unsigned char> keep; DevMem<u32> ctl;
};

// the activity filter's device state (xmaps_ingest.hpp: ActDev), for an ingest or for the filter alone (xm_activity_*)
int act_alloc(ActMem& m, ActDev* a, int cam_w, int cam_h, long long thresh, size_t max_packet, int n_sets = 1) {
  if (thresh < 0 || thresh >= (1ll << 31) - 2) return fail(XM_ERR_INVALID, "activity threshold must be in [0, 2^31 - 2) us");
  const size_t cam_px = (size_t)cam_w * cam_h;
  *a = ActDev{};
  a->thresh = thresh;
  a->cam_w = cam_w;
  a->cam_h = cam_h;
  HIP_TRY(m.last_ts.alloc(cam_px));
  HIP_TRY(m.cells.alloc(cam_px * ACT_NB * (size_t)n_sets));
  HIP_TRY(m.keep.alloc(max_packet ? max_packet : 1));
  HIP_TRY(m.ctl.alloc(4 * (size_t)n_sets));
  a->last_ts = m.last_ts.get();
  a->cells = m.cells.get();
  a->keep = m.keep.get();
  a->ctl = m.ctl.get();
  std::vector<long long> init(cam_px, ING_NO_TS);
  HIP_TRY(hipMemcpy(a->last_ts, init.data(), cam_px * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(a->cells, 0, cam_px * sizeof(uint2) * ACT_NB * (size_t)n_sets));
  HIP_TRY(hipMemset(a->ctl, 0, 4 * sizeof(u32) * (size_t)n_sets));
  HIP_TRY(hipDeviceSynchronize());  // (default-stream work: non-blocking streams do not wait for it)
  return XM_OK;
}

}  // namespace

extern "C" {

// ---- the activity filter alone ------------------------------------------------------------------------------------------
// What `act_filter.process_events(pos_events_buf, act_out_buf)` is in the reference's pipe (depth_reprojection_pipe.py:116-117)
// for a host that keeps the trigger finder on the CPU: one packet of records in, a keep flag per event out.  Same kernels and
// state as the ingest's filter (xmaps_ingest.hpp); every event handed in takes part (the pipe hands it positive events).
struct xm_activity {
  xm_handle* h = nullptr;
  int device = 0;
  Stream stream;
  size_t max_packet = 0;
  ActDev act{};    // views of act_mem
  ActMem act_mem;
  PinnedMem<uint4> h_pkt;  // pinned staging
  DevMem<uint4> d_pkt;
  PinnedMem<unsigned char> h_keep;
};

int xm_activity_create(xm_handle* h, int64_t thresh_us, size_t max_packet_events, xm_activity** out) {
  if (!h || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  XM_ENTER(h);
  Owned<xm_activity, xm_activity_destroy> f(new (std::nothrow) xm_activity());
  if (!f) return fail(XM_ERR_NOMEM, "out of host memory");
  f->h = h;
  f->device = h->cfg.device;
  f->max_packet = max_packet_events ? max_packet_events : ((size_t)1 << 19);
  if (int rc = act_alloc(f->act_mem, &f->act, h->tb.cam_w, h->tb.cam_h, thresh_us, f->max_packet)) return rc;
  HIP_TRY(f->stream.create(hipStreamNonBlocking));
  HIP_TRY(f->h_pkt.alloc(f->max_packet, hipHostMallocDefault));
  HIP_TRY(f->h_keep.alloc(f->max_packet, hipHostMallocDefault));
  HIP_TRY(f->d_pkt.alloc(f->max_packet));
  *out = f.release();
  return XM_OK;
}

int xm_activity_set_rule(xm_activity* f, int self_counts) {
  if (!f) return fail(XM_ERR_INVALID, "NULL argument");
  f->act.self_counts = self_counts ? 1 : 0;  // (by value in every launch: takes effect with the next packet)
  return XM_OK;
}

void xm_activity_destroy(xm_activity* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  delete f;
}

int xm_activity_process(xm_activity* f, const void* eventcd16, size_t n, uint8_t* keep_out, size_t* n_kept) {
  if (!f || (n && (!eventcd16 || !keep_out))) return fail(XM_ERR_INVALID, "NULL argument");
  if (n_kept) *n_kept = 0;
  HIP_TRY(hipSetDevice(f->device));
  size_t kept = 0;
  for (size_t a = 0; a < n; a += f->max_packet) {  // (a longer packet: piece by piece -- the rule does not depend on the cut)
    const size_t m = std::min(f->max_packet, n - a);
    memcpy(f->h_pkt, (const char*)eventcd16 + a * 16, m * 16);
    HIP_TRY(hipMemcpyAsync(f->d_pkt, f->h_pkt, m * 16, hipMemcpyHostToDevice, f->stream));
    const unsigned gx = (unsigned)((m + ING_THREADS - 1) / ING_THREADS);
    hipLaunchKernelGGL(k_act_first, dim3(gx), dim3(ING_THREADS), 0, f->stream, f->act, (const uint4*)f->d_pkt, (const u32*)nullptr, (u32)m, 0);
    hipLaunchKernelGGL(k_act_mark, dim3(gx), dim3(ING_THREADS), 0, f->stream, f->act, (const uint4*)f->d_pkt, (const u32*)nullptr, (u32)m, 0);
    hipLaunchKernelGGL(k_act_update, dim3(gx), dim3(ING_THREADS), 0, f->stream, f->act, (const uint4*)f->d_pkt, (u32)m, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f->h_keep, f->act.keep, m, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    memcpy(keep_out + a, f->h_keep, m);
    for (size_t i = 0; i < m; ++i) kept += f->h_keep[i] != 0;
  }
  if (n_kept) *n_kept = kept;
  return XM_OK;
}

int xm_activity_stats(xm_activity* f, uint64_t* sequential_packets) {
  if (!f) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipStreamSynchronize(f->stream));
  u32 c[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(c, f->act.ctl, sizeof c, hipMemcpyDeviceToHost));
  if (sequential_packets) *sequential_packets = c[2];
  return XM_OK;
}

int xm_activity_reset(xm_activity* f) {
  if (!f) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(f->device));
  HIP_TRY(hipStreamSynchronize(f->stream));
  std::vector<long long> init((size_t)f->act.cam_w * f->act.cam_h, ING_NO_TS);
  HIP_TRY(hipMemcpyAsync(f->act.last_ts, init.data(), init.size() * 8, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipStreamSynchronize(f->stream));
  return XM_OK;
}

}  // extern "C"
