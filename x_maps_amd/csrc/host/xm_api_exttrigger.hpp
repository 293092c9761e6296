// xm_api_exttrigger.hpp -- C-ABI: a recording's EXT_TRIGGER words -> trigger records beside the decoder's events
// (xm_evt_set_ext_triggers / xm_evt_last_ext_triggers: the two launches evt3_run issues behind the emit kernel when the decoder
// has them on), and the frames cut at them: xm_trigframes, a device-resident buffer of EventCD records whose frames are handed
// to the frame entries as (device records, host offsets).  Kernels: ../xmaps_exttrigger.hpp; the cut rule: xm_trigger_cut.hpp.
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

#include "xm_trigger_cut.hpp"

static_assert(sizeof(xm_ext_trigger) == sizeof(uint4), "the kernels store a trigger record as one uint4");

struct xm_trigframes {
  int device = 0;
  TrigCutter cut;
  DevMem<uint4> d_buf;         // cfg.cap_events records
  DevMem<u32> d_counts;        // the append's per-block keep counts, + the kept total behind them
  DevMem<u32> d_remap;         // the chunk's trigger indices in kept records
  PinnedMem<u32> h_remap;      // ... back on the host, [n_remap] = the kept total
  std::vector<xm_ext_trigger> trig;  // the chunk's triggers (host)
  size_t n_counts = 0, n_remap = 0;
};

namespace {

int evt_ext_enqueue(xm_evt3* d, u32 n, u32 nb, hipStream_t stream) {
  const Evt3State* st_in = d->d_state + d->cur;
  const u32 cap = (u32)std::min<size_t>(d->max_triggers, 0xffffffffu);
  u32* counts = d->d_trig_counts;
  if (d->format == 2) {
    const u32* w32 = reinterpret_cast<const u32*>(d->d_words.get());
    const Evt2Scan* agg = reinterpret_cast<const Evt2Scan*>(d->d_agg.get());
    hipLaunchKernelGGL(k_evt2_trig_count, dim3(nb), dim3(EVT_THREADS), 0, stream, w32, n, agg, st_in, counts, d->wait_tb);
    hipLaunchKernelGGL(k_evt2_trig_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, w32, n, agg, st_in, counts, d->d_trig.get(), cap, d->wait_tb);
  } else if (d->format == EVT_FMT_21) {
    const unsigned long long* w64 = reinterpret_cast<const unsigned long long*>(d->d_words.get());
    const Evt21Scan* agg = reinterpret_cast<const Evt21Scan*>(d->d_agg.get());
    hipLaunchKernelGGL(k_evt21_trig_count, dim3(nb), dim3(EVT_THREADS), 0, stream, w64, n, agg, st_in, counts, d->wait_tb, d->legacy_halves);
    hipLaunchKernelGGL(k_evt21_trig_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, w64, n, agg, st_in, counts, d->d_trig.get(), cap, d->wait_tb,
                       d->legacy_halves);
  } else {
    const uint16_t* w16 = d->d_words;
    const Evt3Scan* agg = d->d_agg;
    hipLaunchKernelGGL(k_evt3_trig_count, dim3(nb), dim3(EVT_THREADS), 0, stream, w16, n, agg, st_in, counts, d->wait_tb);
    hipLaunchKernelGGL(k_evt3_trig_emit, dim3(nb), dim3(EVT_THREADS), 0, stream, w16, n, agg, st_in, counts, d->d_trig.get(), cap, d->wait_tb);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(d->h_trig_n, counts + nb, sizeof(u32), hipMemcpyDeviceToHost, stream));
  return XM_OK;
}

int evt_ext_collect(xm_evt3* d, hipStream_t stream) {
  const size_t n = *d->h_trig_n;
  if (n) {
    HIP_TRY(hipMemcpyAsync(d->h_trig, d->d_trig, n * sizeof(uint4), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  d->n_trig = n;
  return XM_OK;
}

// `n` records from `from` to the front of the buffer, as copies that never overlap their source (pieces of at most `from` records)
int trig_move_front(uint4* buf, uint64_t from, uint64_t n, hipStream_t stream) {
  for (uint64_t a = 0; a < n; a += from) {
    const uint64_t m = std::min<uint64_t>(from, n - a);
    HIP_TRY(hipMemcpyAsync(buf + a, buf + from + a, m * sizeof(uint4), hipMemcpyDeviceToDevice, stream));
  }
  return XM_OK;
}

}  // namespace

extern "C" {

int xm_evt_set_ext_triggers(xm_evt3* d, size_t max_triggers) {
  if (!d) return fail(XM_ERR_INVALID, "NULL argument");
  if (d->format == EVT_FMT_DAT) return fail(XM_ERR_INVALID, "CD DAT records carry no trigger words");
  if (max_triggers >= 0x7fffffffull) return fail(XM_ERR_INVALID, "max_triggers must be < 2^31");
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->n_trig = 0;
  if (max_triggers == d->max_triggers) return XM_OK;
  d->max_triggers = 0;
  d->d_trig_counts.reset(), d->d_trig.reset(), d->h_trig_n.reset(), d->h_trig.reset();
  if (!max_triggers) return XM_OK;
  HIP_TRY(d->d_trig_counts.alloc(grid_for(d->max_words, EVT_PER_BLOCK) + 1));
  HIP_TRY(d->d_trig.alloc(max_triggers));
  HIP_TRY(d->h_trig_n.alloc(1, hipHostMallocDefault));
  HIP_TRY(d->h_trig.alloc(max_triggers, hipHostMallocDefault));
  *d->h_trig_n = 0;
  d->max_triggers = max_triggers;
  return XM_OK;
}

int xm_evt_last_ext_triggers(xm_evt3* d, xm_ext_trigger* out_host, size_t cap, size_t* n) {
  if (!d || !n || (cap && !out_host)) return fail(XM_ERR_INVALID, "NULL argument");
  *n = d->max_triggers ? d->n_trig : 0;
  if (*n) memcpy(out_host, d->h_trig.get(), std::min(cap, *n) * sizeof(xm_ext_trigger));
  return XM_OK;
}

int xm_trigframes_create(xm_handle* h, const xm_trigframes_config* cfg, xm_trigframes** out) {
  if (!h || !cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(xm_trigframes_config)) return fail(XM_ERR_INVALID, "xm_trigframes_config.struct_size mismatch");
  if (cfg->edge < XM_TRIG_RISING || cfg->edge > XM_TRIG_BOTH) return fail(XM_ERR_INVALID, "edge must be one of XM_TRIG_*");
  if (cfg->max_frames_ready < 0) return fail(XM_ERR_INVALID, "max_frames_ready must be >= 0");
  XM_ENTER(h);
  Owned<xm_trigframes, xm_trigframes_destroy> tf(new (std::nothrow) xm_trigframes());
  if (!tf) return fail(XM_ERR_NOMEM, "out of host memory");
  tf->device = h->cfg.device;
  tf->cut.cfg = *cfg;
  if (!tf->cut.cfg.cap_events) tf->cut.cfg.cap_events = (uint64_t)1 << 22;
  if (tf->cut.cfg.cap_events >= 0x7fffffffull) return fail(XM_ERR_INVALID, "cap_events must be < 2^31");
  HIP_TRY(tf->d_buf.alloc(tf->cut.cfg.cap_events));
  *out = tf.release();
  return XM_OK;
}

void xm_trigframes_destroy(xm_trigframes* tf) {
  if (!tf) return;
  (void)hipSetDevice(tf->device);
  (void)hipDeviceSynchronize();
  delete tf;
}

int xm_trigframes_reset(xm_trigframes* tf) {
  if (!tf) return fail(XM_ERR_INVALID, "NULL argument");
  tf->cut.reset();
  return XM_OK;
}

int xm_trigframes_push(xm_trigframes* tf, xm_evt3* d, const void* words_host, size_t n_words, int words_pinned, int* n_ready) {
  if (!tf || !d || (n_words && !words_host)) return fail(XM_ERR_INVALID, "NULL argument");
  if (d->device != tf->device) return fail(XM_ERR_INVALID, "decoder and buffer live on different devices");
  if (!d->max_triggers) return fail(XM_ERR_INVALID, "the decoder does not extract trigger words (xm_evt_set_ext_triggers)");
  HIP_TRY(hipSetDevice(d->device));
  size_t n_in = 0;
  int rc = evt3_run(d, words_host, n_words, words_pinned != 0, d->d_out, d->max_events, d->stream, &n_in, true);
  if (rc) return rc;
  TrigCutter& cut = tf->cut;
  if (n_in > cut.cfg.cap_events) return fail(XM_ERR_TOO_MANY, "the chunk decodes to %zu events, the buffer holds %llu", n_in, (unsigned long long)cut.cfg.cap_events);
  const TrigRoom room = cut.room(n_in);
  if (room.rc) return fail(XM_ERR_TOO_MANY, "%zu ready frames leave no room for a chunk of %zu events (release them first)", cut.ready.size(), n_in);
  if (room.move_n) {
    rc = trig_move_front(tf->d_buf, room.move_from, room.move_n, d->stream);
    if (rc) return rc;
  }
  const size_t n_trig = d->n_trig;
  const xm_ext_trigger* src = reinterpret_cast<const xm_ext_trigger*>(d->h_trig.get());
  tf->trig.assign(src, src + n_trig);
  size_t n_kept = n_in;
  uint4* dst = tf->d_buf + room.dst;
  if (n_in && cut.cfg.positive_only) {
    const u32 nb = (u32)grid_for(n_in, EVT_PER_BLOCK);
    if (tf->n_counts < (size_t)nb + 1) {
      HIP_TRY(tf->d_counts.alloc((size_t)nb + 1));
      tf->n_counts = (size_t)nb + 1;
    }
    if (tf->n_remap < n_trig + 1) {
      HIP_TRY(tf->d_remap.alloc(n_trig + 1));
      HIP_TRY(tf->h_remap.alloc(n_trig + 1, hipHostMallocDefault));
      tf->n_remap = n_trig + 1;
    }
    hipLaunchKernelGGL(k_trig_keep_count, dim3(nb), dim3(EVT_THREADS), 0, d->stream, (const uint4*)d->d_out, (u32)n_in, tf->d_counts.get());
    hipLaunchKernelGGL(k_trig_keep_write, dim3(nb), dim3(EVT_THREADS), 0, d->stream, (const uint4*)d->d_out, (u32)n_in, tf->d_counts.get(), dst,
                       (u32)(cut.cfg.cap_events - room.dst), (const uint4*)d->d_trig, (u32)n_trig, tf->d_remap.get());
    HIP_TRY(hipGetLastError());
    if (n_trig) HIP_TRY(hipMemcpyAsync(tf->h_remap, tf->d_remap, n_trig * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipMemcpyAsync(tf->h_remap + n_trig, tf->d_counts + nb, sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    n_kept = tf->h_remap[n_trig];
    for (size_t j = 0; j < n_trig; ++j) tf->trig[j].event_index = tf->h_remap[j];
  } else {
    if (n_in) HIP_TRY(hipMemcpyAsync(dst, d->d_out, n_in * sizeof(uint4), hipMemcpyDeviceToDevice, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
  }
  cut.append(n_in, n_kept, tf->trig.data(), n_trig);
  if (n_ready) *n_ready = (int)cut.ready.size();
  return XM_OK;
}

int xm_trigframes_ready(xm_trigframes* tf, const void** events_dev, uint64_t* offsets_host, int cap_frames, int* n_frames, xm_ext_trigger* opening) {
  if (!tf || !events_dev || !offsets_host || !n_frames || cap_frames < 0) return fail(XM_ERR_INVALID, "NULL argument");
  *events_dev = tf->d_buf.get();
  const int n = tf->cut.run(cap_frames);
  *n_frames = n;
  offsets_host[0] = n ? tf->cut.ready[0].begin : 0;
  for (int f = 0; f < n; ++f) {
    offsets_host[f + 1] = tf->cut.ready[f].end;
    if (opening) opening[f] = tf->cut.ready[f].opening;
  }
  return XM_OK;
}

int xm_trigframes_release(xm_trigframes* tf, int n_frames) {
  if (!tf) return fail(XM_ERR_INVALID, "NULL argument");
  if (n_frames < 0 || (size_t)n_frames > tf->cut.ready.size()) return fail(XM_ERR_INVALID, "%d frames to release, %zu are ready", n_frames, tf->cut.ready.size());
  tf->cut.release(n_frames);
  return XM_OK;
}

int xm_trigframes_stats(xm_trigframes* tf, xm_trigframes_counters* out) {
  if (!tf || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = tf->cut.st;
  return XM_OK;
}

}  // extern "C"
