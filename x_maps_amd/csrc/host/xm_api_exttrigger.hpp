// xm_api_exttrigger.hpp -- C-ABI: a recording's EXT_TRIGGER words -> trigger records beside the decoder's events
// (xm_evt_set_ext_triggers / xm_evt_last_ext_triggers: the two launches evt3_run issues behind the emit kernel when the decoder
// has them on), and the frames cut at them: xm_trigframes, a device-resident buffer of EventCD records whose frames are handed
// to the frame entries as (device records, host offsets).  Kernels: ../xmaps_exttrigger.hpp; the cut rule: xm_trigger_cut.hpp.
// The chain's two filters (../xmaps_trigfilter.hpp): the activity filter as a stage of the push (xm_trigframes_set_activity), the
// frame event filters as a stage on runs of ready frames (xm_trigframes_set_frame_filter / xm_trigframes_ready_filtered).  Both
// off by default: a push then issues what it always issued.
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
  const xm_handle* h = nullptr;  // the rig: sensor size, rectify LUT (outlives the buffer, as it outlives the decoder)
  // stage 1: the activity filter (act.last_ts == NULL: never switched on)
  bool act_on = false;
  ActDev act{};                // views of act_mem; .keep = d_keep
  ActMem act_mem;
  DevMem<unsigned char> d_keep;  // the chunk's keep bytes: n_keep of them, whole blocks of EVT_PER_BLOCK (grows with the chunk, as d_counts)
  size_t n_keep = 0;
  DevMem<unsigned long long> d_fstats;  // [0] p == 1 records of the chunks judged
  uint64_t events_active = 0;
  // stage 2: the frame event filters (ff_filter == 0: none)
  int ff_filter = 0, ff_intended = 0, ff_max_frames = 0;
  TrigFilterDev ff{};          // views of the scratch below, sized for ff_max_frames frames of ff_cells cells
  size_t ff_cells = 0;         // cells per frame the scratch was allocated for
  DevMem<u32> d_last, d_first, d_sums, d_xr, d_dropped, d_result;
  DevMem<u64> d_offs;
  DevMem<uint4> d_surv;
  PinnedMem<u32> h_result;
  PinnedMem<u64> h_offs;
  Stream ff_stream;
  uint64_t frames_filtered = 0, events_after_ff = 0, index_errors = 0;
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

// an empty history (the ingest's xm_activity_reset); the caller has set the device
int trig_act_clear(xm_trigframes* tf) {
  std::vector<long long> init((size_t)tf->act.cam_w * tf->act.cam_h, ING_NO_TS);
  HIP_TRY(hipMemcpy(tf->act.last_ts, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
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
  tf->h = h;
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
  if (tf->act.last_ts) {  // the history goes with the stream (the cells and ctl[0] are clean between pushes)
    HIP_TRY(hipSetDevice(tf->device));
    if (int rc = trig_act_clear(tf)) return rc;
  }
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
  const bool act = tf->act_on && cut.cfg.positive_only;
  if (n_in && cut.cfg.positive_only) {
    const u32 nb = (u32)grid_for(n_in, EVT_PER_BLOCK);
    if (act && tf->n_keep < (size_t)nb * EVT_PER_BLOCK) {
      HIP_TRY(tf->d_keep.alloc((size_t)nb * EVT_PER_BLOCK));
      tf->n_keep = (size_t)nb * EVT_PER_BLOCK;
    }
    if (tf->n_counts < (size_t)nb + 1) {
      HIP_TRY(tf->d_counts.alloc((size_t)nb + 1));
      tf->n_counts = (size_t)nb + 1;
    }
    if (tf->n_remap < n_trig + 1) {
      HIP_TRY(tf->d_remap.alloc(n_trig + 1));
      HIP_TRY(tf->h_remap.alloc(n_trig + 1, hipHostMallocDefault));
      tf->n_remap = n_trig + 1;
    }
    if (act) {  // (xmaps_trigfilter.hpp, stage 1: four launches in place of the two)
      tf->act.keep = tf->d_keep;
      const uint4* ev = (const uint4*)d->d_out;
      hipLaunchKernelGGL(k_act_first, dim3((unsigned)grid_for(n_in, ING_THREADS)), dim3(ING_THREADS), 0, d->stream, tf->act, ev, (const u32*)nullptr, (u32)n_in, 1);
      hipLaunchKernelGGL(k_trigact_seq, dim3(1), dim3(ACT_GROUP), 0, d->stream, tf->act, ev, (u32)n_in);
      hipLaunchKernelGGL(k_trigact_count, dim3(nb), dim3(EVT_THREADS), 0, d->stream, tf->act, ev, (u32)n_in, tf->d_counts.get(), tf->d_fstats.get());
      hipLaunchKernelGGL(k_trigact_write, dim3(nb), dim3(EVT_THREADS), 0, d->stream, tf->act, ev, (u32)n_in, tf->d_counts.get(), dst,
                         (u32)(cut.cfg.cap_events - room.dst), (const uint4*)d->d_trig, (u32)n_trig, tf->d_remap.get());
    } else {
      hipLaunchKernelGGL(k_trig_keep_count, dim3(nb), dim3(EVT_THREADS), 0, d->stream, (const uint4*)d->d_out, (u32)n_in, tf->d_counts.get());
      hipLaunchKernelGGL(k_trig_keep_write, dim3(nb), dim3(EVT_THREADS), 0, d->stream, (const uint4*)d->d_out, (u32)n_in, tf->d_counts.get(), dst,
                         (u32)(cut.cfg.cap_events - room.dst), (const uint4*)d->d_trig, (u32)n_trig, tf->d_remap.get());
    }
    HIP_TRY(hipGetLastError());
    if (n_trig) HIP_TRY(hipMemcpyAsync(tf->h_remap, tf->d_remap, n_trig * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipMemcpyAsync(tf->h_remap + n_trig, tf->d_counts + nb, sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    n_kept = tf->h_remap[n_trig];
    for (size_t j = 0; j < n_trig; ++j) tf->trig[j].event_index = tf->h_remap[j];
    if (act) tf->events_active += n_kept;
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

// ---- the chain's two filters (../xmaps_trigfilter.hpp) --------------------------------------------------------------------------
int xm_trigframes_set_activity(xm_trigframes* tf, int64_t thresh_us, int self_counts) {
  if (!tf) return fail(XM_ERR_INVALID, "NULL argument");
  if (thresh_us < 0) {  // off: the state stays allocated, the next switch-on empties it
    tf->act_on = false;
    return XM_OK;
  }
  if (!tf->cut.cfg.positive_only) return fail(XM_ERR_INVALID, "the activity filter judges positive events: the buffer was created without positive_only");
  HIP_TRY(hipSetDevice(tf->device));
  if (!tf->act.last_ts || tf->act.thresh != (long long)thresh_us) {
    ActDev a{};
    ActMem m;
    if (int rc = act_alloc(m, &a, tf->h->tb.cam_w, tf->h->tb.cam_h, (long long)thresh_us, 8)) return rc;  // (the range check is act_alloc's)
    if (!tf->d_fstats) {
      HIP_TRY(tf->d_fstats.alloc(1));
      HIP_TRY(hipMemset(tf->d_fstats, 0, sizeof(unsigned long long)));
      HIP_TRY(hipDeviceSynchronize());
    }
    if (tf->act.last_ts) {  // chunks judged sequentially under the threshold before: the count is the buffer's, not the state's
      u32 c[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemcpy(c, tf->act.ctl, sizeof c, hipMemcpyDeviceToHost));
      c[0] = c[1] = c[3] = 0;
      HIP_TRY(hipMemcpy(a.ctl, c, sizeof c, hipMemcpyHostToDevice));
    }
    tf->act_mem = std::move(m);
    tf->act = a;
  } else if (!tf->act_on) {
    if (int rc = trig_act_clear(tf)) return rc;  // switching it on starts from an empty history
  }
  tf->act.self_counts = self_counts ? 1 : 0;  // (by value in every launch)
  tf->act_on = true;
  return XM_OK;
}

int xm_trigframes_filter_stats(xm_trigframes* tf, xm_trigframes_filter_counters* out) {
  if (!tf || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = xm_trigframes_filter_counters{};
  if (tf->act.last_ts) {  // (pushes are synchronous: nothing of stage 1 is in flight)
    HIP_TRY(hipSetDevice(tf->device));
    u32 c[4] = {0, 0, 0, 0};
    unsigned long long pos = 0;
    HIP_TRY(hipMemcpy(c, tf->act.ctl, sizeof c, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&pos, tf->d_fstats, sizeof pos, hipMemcpyDeviceToHost));
    out->events_positive = pos;
    out->chunks_sequential = c[2];
  }
  out->events_active = tf->events_active;
  out->frames_filtered = tf->frames_filtered;
  out->events_after_frame_filter = tf->events_after_ff;
  out->index_errors = tf->index_errors;
  return XM_OK;
}

int xm_trigframes_set_frame_filter(xm_trigframes* tf, int filter, int intended_semantics, int max_frames) {
  if (!tf) return fail(XM_ERR_INVALID, "NULL argument");
  if (filter != 0 && (filter < FILTER_FIRST_PER_YT || filter > FILTER_MEAN_PER_XY)) return fail(XM_ERR_INVALID, "unknown filter %d", filter);
  if (!filter) {
    tf->ff_filter = 0;
    return XM_OK;
  }
  if (max_frames < 1 || max_frames > 4096) return fail(XM_ERR_INVALID, "max_frames must lie in 1 .. 4096");
  const xm_handle* h = tf->h;
  const bool yt = filter == FILTER_FIRST_PER_YT;
  const int yt_w = h->plan().cols.xr_max + 1;
  const u64 cells_yt = yt_w > 0 ? (u64)yt_w * (u64)h->tb.cam_h : 0;
  if (yt && !(cells_yt > 0 && cells_yt <= (u64)XM_INGEST_YT_MAX_CELLS))
    return fail(XM_ERR_INVALID, "FirstEventPerYT: a cell map of %d rows x %d columns (the rectify LUT's largest entry + 1) exceeds %llu cells",
                h->tb.cam_h, yt_w, (unsigned long long)XM_INGEST_YT_MAX_CELLS);
  const size_t cells = yt ? (size_t)cells_yt : (size_t)h->tb.cam_w * (size_t)h->tb.cam_h;
  HIP_TRY(hipSetDevice(tf->device));
  if (!tf->ff_stream) HIP_TRY(tf->ff_stream.create(hipStreamNonBlocking));
  if (cells > tf->ff_cells || max_frames > tf->ff_max_frames) {  // the scratch: sized for the larger of what has been asked for so far
    const size_t mf = (size_t)std::max(max_frames, tf->ff_max_frames), nc = std::max(cells, tf->ff_cells);
    const size_t blocks = (nc + FF_BLOCK - 1) / FF_BLOCK, surv = std::min<size_t>(mf * nc, (size_t)tf->cut.cfg.cap_events);
    tf->ff_cells = 0, tf->ff_max_frames = 0, tf->ff_filter = 0;  // (a failed allocation leaves the stage off)
    HIP_TRY(tf->d_last.alloc(mf * nc));
    HIP_TRY(tf->d_first.alloc(mf * nc));
    HIP_TRY(tf->d_sums.alloc(mf * blocks));
    HIP_TRY(tf->d_xr.alloc(mf));
    HIP_TRY(tf->d_dropped.alloc(mf));
    HIP_TRY(tf->d_result.alloc(2 * mf));
    HIP_TRY(tf->d_offs.alloc(mf + 1));
    HIP_TRY(tf->d_surv.alloc(surv ? surv : 1));
    HIP_TRY(tf->h_result.alloc(2 * mf, hipHostMallocDefault));
    HIP_TRY(tf->h_offs.alloc(mf + 1, hipHostMallocDefault));
    HIP_TRY(hipMemset(tf->d_last, 0, mf * nc * sizeof(u32)));
    HIP_TRY(hipMemset(tf->d_first, 0, mf * nc * sizeof(u32)));
    HIP_TRY(hipMemset(tf->d_xr, 0, mf * sizeof(u32)));
    HIP_TRY(hipMemset(tf->d_dropped, 0, mf * sizeof(u32)));
    HIP_TRY(hipDeviceSynchronize());  // (default-stream memsets: the stage's non-blocking stream does not wait for them)
    tf->ff_cells = nc, tf->ff_max_frames = (int)mf;
    tf->ff.surv_cap = (u32)std::min<size_t>(surv, 0xffffffffu);
  }
  TrigFilterDev& f = tf->ff;
  f.buf = tf->d_buf;
  f.offsets = tf->d_offs;
  f.last = tf->d_last, f.first = tf->d_first, f.sums = tf->d_sums, f.xr_enc = tf->d_xr, f.dropped = tf->d_dropped, f.result = tf->d_result;
  f.survivors = tf->d_surv;
  f.lut = h->tb.lut;
  f.max_frames = (u32)tf->ff_max_frames;
  f.cam_w = h->tb.cam_w, f.cam_h = h->tb.cam_h;
  f.map_w = yt ? yt_w : h->tb.cam_w;
  f.n_cells = (u32)cells;  // (the maps' frame stride: frames lie n_cells apart, whatever the scratch was sized for)
  f.filter = filter;
  f.use_first = intended_semantics && filter != FILTER_LAST_PER_XY;
  f.wrap = yt && h->plan().cols.xr_min < 0;
  tf->ff_filter = filter, tf->ff_intended = intended_semantics ? 1 : 0;
  return XM_OK;
}

int xm_trigframes_ready_filtered(xm_trigframes* tf, const void** events_dev, uint64_t* offsets_host, int cap_frames, int* n_frames,
                                 xm_ext_trigger* opening, uint64_t* n_index_errors) {
  if (!tf || !events_dev || !offsets_host || !n_frames || cap_frames < 0) return fail(XM_ERR_INVALID, "NULL argument");
  if (!tf->ff_filter) {
    const int rc = xm_trigframes_ready(tf, events_dev, offsets_host, cap_frames, n_frames, opening);
    if (!rc && n_index_errors) std::fill(n_index_errors, n_index_errors + *n_frames, (uint64_t)0);
    return rc;
  }
  const int n = tf->cut.run(std::min(cap_frames, tf->ff_max_frames));
  *events_dev = tf->d_surv.get();
  *n_frames = n;
  offsets_host[0] = 0;
  if (!n) return XM_OK;
  const TrigFilterDev& f = tf->ff;
  uint64_t longest = 0;
  tf->h_offs[0] = tf->cut.ready[0].begin;
  for (int i = 0; i < n; ++i) {
    tf->h_offs[i + 1] = tf->cut.ready[i].end;
    longest = std::max<uint64_t>(longest, tf->cut.ready[i].end - tf->cut.ready[i].begin);
    if (opening) opening[i] = tf->cut.ready[i].opening;
  }
  HIP_TRY(hipSetDevice(tf->device));
  hipStream_t s = tf->ff_stream;
  HIP_TRY(hipMemcpyAsync(tf->d_offs, tf->h_offs, (size_t)(n + 1) * sizeof(u64), hipMemcpyHostToDevice, s));
  const dim3 ge((unsigned)grid_for(longest < 1 ? 1 : longest, FF_THREADS), (unsigned)n), gc((unsigned)grid_for(f.n_cells, FF_BLOCK), (unsigned)n);
  if (f.wrap) hipLaunchKernelGGL(k_tff_width, ge, dim3(FF_THREADS), 0, s, f);
  hipLaunchKernelGGL(k_tff_scatter, ge, dim3(FF_THREADS), 0, s, f);
  hipLaunchKernelGGL(k_tff_count, gc, dim3(FF_BLOCK), 0, s, f);
  hipLaunchKernelGGL(k_tff_emit, gc, dim3(FF_BLOCK), 0, s, f);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(tf->h_result, tf->d_result, 2 * (size_t)f.max_frames * sizeof(u32), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int i = 0; i < n; ++i) {
    const uint64_t kept = tf->h_result[i], bad = tf->h_result[f.max_frames + i];
    offsets_host[i + 1] = offsets_host[i] + kept;
    if (n_index_errors) n_index_errors[i] = bad;
    tf->events_after_ff += kept;
    tf->index_errors += bad;
  }
  tf->frames_filtered += (uint64_t)n;
  return XM_OK;
}

}  // extern "C"
