// xm_api_engine.hpp -- C-ABI: lifetime (xm_create / xm_destroy), synchronisation, the fused hot path (frames, groups, adaptive batching), profiling
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

// =====================================================================================================
extern "C" {

int xm_api_version(void) { return XM_API_VERSION; }
const char* xm_last_error(void) { return g_err.c_str(); }

int xm_create(const xm_config* cfg, xm_handle** out) {
  if (!cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (int rc = validate_config(cfg)) return rc;
  HIP_TRY(hipSetDevice(cfg->device));

  Owned<xm_handle, xm_destroy> h(new (std::nothrow) xm_handle());
  if (!h) return fail(XM_ERR_NOMEM, "out of host memory");
  h->cfg = *cfg;
  h->cfg.n_slots = cfg->n_slots > 0 ? cfg->n_slots : 1;
  h->cfg.xmap_height = cfg->xmap_height > 0 ? cfg->xmap_height : cfg->rect_height;
  RigPlan& plan = h->plan_in_create();
  plan.modes.time_sorted = (cfg->flags & XM_FLAG_TIME_SORTED) != 0;
  // default: the verified (t[0], t[n-1]) shortcut with automatic redo (exact for any event order); XM_FLAG_GENERAL forces the
  // extrema pass on every frame
  plan.modes.try_sorted = !plan.modes.time_sorted && !(cfg->flags & XM_FLAG_GENERAL);
  if ((cfg->flags & XM_FLAG_ADAPTIVE_BATCH) && h->cfg.n_slots >= 8) h->ab_max = std::min(h->cfg.n_slots / 4, 32);  // (four groups' worth of slots)

  CreateOpts o;
  read_create_options(plan, o);
  int rc;
  if ((rc = upload_tables(h.get()))) return rc;
  if ((rc = build_k2_tables(h.get(), o))) return rc;
  if ((rc = classify_rig(h.get(), o))) return rc;
  apply_k1_windows(plan, o);
  const RigPlan& done = h->plan();  // the plan is finished: read-only from here on
  if ((rc = build_k2_live(h.get(), done, o))) return rc;
  if ((rc = create_slots(h.get(), done, o))) return rc;
  if ((rc = create_batch_rings(h.get()))) return rc;
  start_workers(h.get(), o);
  *out = h.release();
  return XM_OK;
}

// Shutdown order only (xm_res.hpp): everything the handle owns is released by its members, after every stream has been synchronised.
void xm_destroy(xm_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  if (!h->pending.empty()) (void)flush_pending(h);  // XM_FLAG_ADAPTIVE_BATCH: frames still held back are submitted, not dropped
  for (auto& w : h->workers) {
    Job stop;
    stop.kind = Job::STOP;
    w->q.post(stop);
  }
  for (auto& w : h->workers)
    if (w->th.joinable()) w->th.join();
  h->workers.clear();
  for (hipStream_t gs : h->gstreams) if (gs) (void)hipStreamSynchronize(gs);
  for (Slot& s : h->slots) if (s.stream) (void)hipStreamSynchronize(s.stream);
  delete h;
}

int xm_path_counts(xm_handle* h, uint64_t counts[4]) {
  if (!h || !counts) return fail(XM_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 4; ++i) counts[i] = h->path_counts[i].load(std::memory_order_relaxed);
  return XM_OK;
}

int xm_cols_info(xm_handle* h, int32_t info[12]) {
  if (!h || !info) return fail(XM_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 12; ++i) info[i] = 0;
  const RigPlan& p = h->plan();
  info[0] = !p.cols.ok ? 0 : p.cols.own_mode ? 2 : 1;
  if (p.cols.ok && p.cols.own_mode) {
    const RigPlan::Own& os = p.own[0];  // (the plan frames take by default; [10], [11]: width and halo of the one for denser frames)
    info[1] = os.w;
    info[2] = os.halo;
    info[3] = os.nxs_max;
    info[4] = h->tb.shear_m;
    info[5] = h->tb.shear_extra;
    info[6] = os.r_lo;
    info[7] = os.hr;
    info[8] = os.extras;
    info[9] = os.extra_max;
    for (int i = 1; i < OWN_PLANS; ++i)  // (the narrowest plan: the one the densest frames take)
      if (p.own[i].ok) {
        info[10] = p.own[i].w;
        info[11] = p.own[i].halo;
      }
  }
  return XM_OK;
}

int xm_own_plan_info(const xm_config* cfg, int32_t info[12]) {
  if (!cfg || !info) return fail(XM_ERR_INVALID, "NULL argument");
  if (cfg->struct_size != sizeof(xm_config)) return fail(XM_ERR_INVALID, "xm_config.struct_size");
  if (!cfg->cam_mapx_i16 || !cfg->cam_mapy_i16 || !cfg->proj_x_map || cfg->cam_width <= 0 || cfg->cam_height <= 0 ||
      cfg->xmap_width <= 1 || cfg->rect_width <= 0 || cfg->rect_height <= 0)
    return fail(XM_ERR_INVALID, "bad tables");
  for (int i = 0; i < 12; ++i) info[i] = 0;
  const int xmap_h = cfg->xmap_height > 0 ? cfg->xmap_height : cfg->rect_height;
  const int xr_min = table_extrema(cfg->cam_mapx_i16, (size_t)cfg->cam_width * cfg->cam_height, cfg->proj_x_map, 0).xr_min;
  OwnPlan pls[OWN_PLANS];
  own_plans(cfg, xmap_h, xr_min, pls);
  const OwnPlan& pl = pls[0];  // (the plan frames take by default)
  if (!pl.ok) return XM_OK;
  info[0] = 2; info[1] = pl.W; info[2] = pl.halo; info[3] = pl.nxs_max; info[4] = pl.m; info[5] = pl.extra_cols; info[6] = pl.r_lo;
  info[7] = pl.hr; info[8] = (int)pl.extra_flat.size() - 1; info[9] = pl.extra_max; info[10] = pl.delta_max;
  info[11] = (int)own_plan_lds_bytes(pl.nxs_max, pl.rp, pl.hrp, pl.extra_max, pl.grouped);
  return XM_OK;
}

int xm_sorted_fallbacks(xm_handle* h, uint64_t* count) {
  if (!h || !count) return fail(XM_ERR_INVALID, "NULL argument");
  *count = h->sorted_fallbacks;
  return XM_OK;
}

// Wait for a stream: poll it for a while before blocking.  A blocking hipStreamSynchronize wakes up tens of microseconds
// after the stream has drained (interrupt path); the hot loop's frames are ~10 us, so a caller that brackets short bursts with
// xm_sync() (bench.py --steps 20: 0.2 ms of work) would spend a quarter of its time asleep.
static int wait_stream(hipStream_t st) {
  const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
  unsigned spins = 0;
  for (;;) {
    const hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess) return XM_OK;
    if (q != hipErrorNotReady) HIP_TRY(q);
    __builtin_ia32_pause();
    if ((++spins & 0xff) == 0 && std::chrono::steady_clock::now() > give_up) break;
  }
  HIP_TRY(hipStreamSynchronize(st));
  return XM_OK;
}

int xm_sync(xm_handle* h) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  XM_ENTER(h);
  for (hipStream_t st : h->streams) {
    int rcw = wait_stream(st);
    if (rcw) return rcw;
  }
  for (hipStream_t gs : h->gstreams) {  // graph replays run on streams of their own
    int rcw = wait_stream(gs);
    if (rcw) return rcw;
  }
  for (Slot& s : h->slots) s.order.forget();  // every stream is idle: nothing left to order against
  if (h->plan().modes.try_sorted) {  // frames whose shortcut failed are redone now, then waited for
    for (Slot& s : h->slots) {
      bool redone = false;
      int rc = resolve_prev(h, s, &redone);
      if (rc) return rc;
      if (redone) {
        if ((rc = drain_workers(h))) return rc;
        HIP_TRY(hipStreamSynchronize(s.stream));
      }
    }
  }
  if (h->plan().modes.time_sorted) {  // any asynchronously processed frame that was not sorted after all?
    u32 bad = 0;
    // one copy of all slot states (3 KB each) instead of one synchronous 4-byte copy per slot (60 slots: 0.9 ms)
    std::vector<SlotState> hs(h->slots.size());
    HIP_TRY(hipMemcpy(hs.data(), h->d_states, sizeof(SlotState) * hs.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hs.size(); ++i) {
      if (hs[i].unsorted_sticky) {
        bad += hs[i].unsorted_sticky;
        HIP_TRY(hipMemset(&h->slots[i].st->unsorted_sticky, 0, sizeof(u32)));
      }
    }
    if (bad) HIP_TRY(hipDeviceSynchronize());  // (a memset of device memory may return early; the slots' streams do not wait for the default one)
    if (bad) return fail(XM_ERR_UNSORTED, "XM_FLAG_TIME_SORTED: %u wavefront(s) saw events outside [t[0], t[n-1]] -- a frame "
                         "processed since the last xm_sync was not time-sorted, its output is invalid", bad);
  }
  return XM_OK;
}

#ifdef XM_ABLATE
// experiments only: copy out the s_memtime timeline written by k_scatter_tiled
int xm_debug_timeline(unsigned long long* out /*[64][16]*/) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(xm::g_timeline), sizeof(unsigned long long) * 64 * 16));
  return XM_OK;
}
#endif

// tests: the column-tile path's integer time thresholds of a frame with the given first / last stamp (thr[0 .. xmap_w])
int xm_debug_cols_thresholds(xm_handle* h, long long t_first, long long t_last, uint32_t* out_host) {
  if (!h || !out_host) return fail(XM_ERR_INVALID, "NULL argument");
  if ((unsigned long long)(t_last - t_first) >= 0xffffffffull && t_last >= t_first)
    return fail(XM_ERR_INVALID, "frames of 2^32 us or more do not take the column tiles");
  XM_ENTER(h);
  const int n = h->tb.xmap_w + 1;
  DevMem<u32> d;
  HIP_TRY(d.alloc(n));
  hipLaunchKernelGGL(k_debug_cols_thresholds, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, h->slots[0].stream, t_first, t_last,
                     h->tb.t_px_scale, h->tb.xmap_w, d.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->slots[0].stream));  // (d is released on return: the kernel has run by then either way)
  HIP_TRY(hipMemcpy(out_host, d, sizeof(u32) * n, hipMemcpyDeviceToHost));
  return XM_OK;
}

// tests: the u16 disparity frame the column / owner tiles left in the slot of the handle's last frame (A3's output before K2),
// un-sheared, as [rect_h][rect_w] row-major like the reference's disp_map.  Meaningful only if that frame took the tiles
// (xm_path_counts) and was not redone.
int xm_debug_last_disp_frame(xm_handle* h, uint16_t* out_host) {
  if (!h || !out_host) return fail(XM_ERR_INVALID, "NULL argument");
  XM_ENTER(h);
  Slot& s = h->slots[h->last_slot];
  if (!s.frame16) return fail(XM_ERR_INVALID, "this handle has no column-tile frames");
  if (int rc = s.order.host_wait()) return rc;
  const size_t cells = frame16_cells(h->tb);
  std::vector<uint16_t> raw(cells);
  HIP_TRY(hipMemcpy(raw.data(), s.frame16, cells * sizeof(uint16_t), hipMemcpyDeviceToHost));
  const int rw = h->tb.rect_w, rh = h->tb.rect_h;
  for (int r = 0; r < rh; ++r)
    for (int x = 0; x < rw; ++x) out_host[(size_t)r * rw + x] = raw[(size_t)frame16_col(h->tb, x, r) * rh + r];
  return XM_OK;
}

// tests: frames finished by the software-pipelined K2 (k_frame_proj_pipe) since xm_create
int xm_debug_k2_pipe_frames(xm_handle* h, uint64_t* count) {
  if (!h || !count) return fail(XM_ERR_INVALID, "NULL argument");
  XM_ENTER(h);
  *count = h->k2_pipe_frames;
  return XM_OK;
}

// tests: the group frame kernel (launch_k2_batch<2>: the pipelined K2, or k_frame_proj_tiled_batch<2> where that one does not take
// the group) on caller-supplied disparity frames, plain [rect_w][rect_h] column-major like xm_shard_finish_u16's.  Every frame gets
// a device buffer of its own in the slot layout (cell (x, row) at column frame16_col: the inverse of xm_debug_last_disp_frame;
// cells no (x, row) maps to are zero) and a zeroed scratch SlotState of its own (tag_a = 0, no host flags): no slot's state, tag
// or frame is touched.  valid_host[f] == 0: FrameDesc.valid = 0, the frame is not run.  Frame f writes depth_out + f * H * W and
// bgr_out + f * H * W * 3 (device pointers; either may be NULL).  Synchronous.
int xm_debug_k2_group_u16(xm_handle* h, const uint16_t* frames_host, int n_frames, const uint8_t* valid_host, float* depth_out,
                          uint8_t* bgr_out) {
  if (!h || !frames_host) return fail(XM_ERR_INVALID, "NULL argument");
  if (n_frames < 1 || n_frames > 64) return fail(XM_ERR_INVALID, "n_frames must be in [1, 64]");
  if (!h->plan().dims.projector || h->plan().modes.k2_direct || !h->plan().k2.has_tables)
    return fail(XM_ERR_INVALID, "xm_debug_k2_group_u16 needs a projector-view handle with the tiled frame kernel");
  XM_ENTER(h);
  const int rw = h->tb.rect_w, rh = h->tb.rect_h;
  const size_t cells = frame16_cells(h->tb), px = (size_t)h->tb.proj_w * h->tb.proj_h;
  hipStream_t stream = h->slots[0].stream;
  DevMem<uint16_t> d_frames;
  DevMem<SlotState> d_st;
  DevMem<FrameDesc> d_descs;
  HIP_TRY(d_frames.alloc(cells * (size_t)n_frames, 64));
  HIP_TRY(d_st.alloc((size_t)n_frames));
  HIP_TRY(d_descs.alloc((size_t)n_frames));
  std::vector<uint16_t> raw(cells * (size_t)n_frames, (uint16_t)0);
  std::vector<FrameDesc> descs((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) {
    const uint16_t* src = frames_host + (size_t)f * rw * rh;
    uint16_t* dst = raw.data() + (size_t)f * cells;
    for (int x = 0; x < rw; ++x)
      for (int r = 0; r < rh; ++r) {
        const int col = frame16_col(h->tb, x, r);
        if (col < 0 || (size_t)col * rh + r >= cells) return fail(XM_ERR_INVALID, "cell (%d, %d) has no place in the sheared frame", x, r);
        dst[(size_t)col * rh + r] = src[(size_t)x * rh + r];
      }
    FrameDesc& d = descs[f];
    std::memset(&d, 0, sizeof d);
    d.key_frame = reinterpret_cast<u64*>(d_frames.get() + (size_t)f * cells);
    d.st = d_st.get() + f;
    d.depth = depth_out ? depth_out + (size_t)f * px : nullptr;
    d.bgr = bgr_out ? bgr_out + (size_t)f * px * 3 : nullptr;
    d.valid = valid_host && !valid_host[f] ? 0u : 1u;
  }
  HIP_TRY(hipMemsetAsync(d_frames.get(), 0, cells * (size_t)n_frames * sizeof(uint16_t) + 64, stream));
  HIP_TRY(hipMemsetAsync(d_st.get(), 0, sizeof(SlotState) * (size_t)n_frames, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(d_frames.get(), raw.data(), raw.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_descs.get(), descs.data(), descs.size() * sizeof(FrameDesc), hipMemcpyHostToDevice));
  launch_k2_batch<2>(h, stream, d_descs.get(), n_frames);
  const hipError_t launched = hipGetLastError();
  HIP_TRY(hipStreamSynchronize(stream));  // (the buffers are released on return: the kernel has run by then either way)
  HIP_TRY(launched);
  return XM_OK;
}

void* xm_stream(xm_handle* h, int slot) {
  if (!h || slot < 0 || slot >= (int)h->slots.size()) return nullptr;
  return (void*)h->slots[slot].stream;
}

int xm_process_frame(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n,
                     int t_dtype, int mem, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats) {
  EventsView ev;
  ev.x = x; ev.y = y; ev.t = t; ev.p = p; ev.n = n; ev.t_dtype = t_dtype; ev.use_p = p != nullptr;
  return process_common(h, ev, mem, depth_out, bgr_out, stats, false);
}

int xm_process_frame_aos(xm_handle* h, const void* eventcd16, size_t n, int use_polarity, int mem, float* depth_out,
                         uint8_t* bgr_out, xm_frame_stats* stats) {
  if (n && !eventcd16) return fail(XM_ERR_INVALID, "NULL event buffer");
  EventsView ev;
  static const uint4 dummy = {0, 0, 0, 0};
  ev.aos = eventcd16 ? eventcd16 : (const void*)&dummy;
  ev.n = n; ev.t_dtype = XM_T_INT64; ev.use_p = use_polarity != 0;
  if (mem == XM_MEM_DEVICE && n == 0) ev.aos = h ? (const void*)h->d_lut : ev.aos;  // any valid device address
  return process_common(h, ev, mem, depth_out, bgr_out, stats, false);
}

int xm_profile_frame(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n,
                     int t_dtype, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats) {
  EventsView ev;
  ev.x = x; ev.y = y; ev.t = t; ev.p = p; ev.n = n; ev.t_dtype = t_dtype; ev.use_p = p != nullptr;
  return process_common(h, ev, XM_MEM_DEVICE, depth_out, bgr_out, stats, true);
}

int xm_last_frame_stats(xm_handle* h, xm_frame_stats* stats) {
  if (!h || !stats) return fail(XM_ERR_INVALID, "NULL argument");
  XM_ENTER(h);
  Slot& s = h->slots[h->last_slot];
  if (int rc = s.order.host_wait()) return rc;  // (its last frame may have run inside a group / a graph replay on another stream)
  return fetch_stats(h, s, s.last.t_dtype, stats);
}

int xm_profile_event_overhead(xm_handle* h, int reps, float* ms_out) {
  if (!h || !ms_out || reps <= 0) return fail(XM_ERR_INVALID, "bad argument");
  XM_ENTER(h);
  Slot& s = h->slots[0];
  std::vector<float> v;
  for (int i = 0; i < reps; ++i) {
    HIP_TRY(hipEventRecord(h->prof_ev[0], s.stream));
    HIP_TRY(hipEventRecord(h->prof_ev[1], s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->prof_ev[0], h->prof_ev[1]));
    v.push_back(ms);
  }
  std::sort(v.begin(), v.end());
  *ms_out = v[v.size() / 2];
  return XM_OK;
}

// ---- a group of frames in one set of multi-frame launches ---------------------------------------------------
static int submit_group(xm_handle* h, const BatchViews& v, float* gpu_ms, hipEvent_t* done_out = nullptr);

static int process_batch_impl(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                              const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out, float* gpu_ms,
                              const void* aos = nullptr) {
  if (!h || !offsets_host || n_frames <= 0) return fail(XM_ERR_INVALID, "bad argument");
  const int ns = (int)h->slots.size();
  if (n_frames > ns) return fail(XM_ERR_INVALID, "a batch of %d frames needs n_slots >= %d (handle has %d)", n_frames, n_frames, ns);
  XM_ENTER(h);
  BatchViews v;
  if (int rc = batch_views(h->plan(), x, y, t, p, t_dtype, aos, offsets_host, n_frames, depth_out, bgr_out, v)) return rc;
  return submit_group(h, v, gpu_ms);
}

// frames v.evs[f] -> outputs v.dep[f] / v.bg[f] (device pointers) as ONE group on the next n slots: one set of multi-frame launches
static int submit_group(xm_handle* h, const BatchViews& v, float* gpu_ms, hipEvent_t* done_out) {
  const int n_frames = (int)v.evs.size(), ns = (int)h->slots.size();
  std::vector<int> idx(n_frames);
  for (int f = 0; f < n_frames; ++f) {
    idx[f] = (h->next_slot + f) % ns;
    int rc = resolve_prev(h, h->slots[idx[f]]);  // try-sorted verdict of the slot's previous frame (may redo it)
    if (rc) return rc;
  }
  h->next_slot = (h->next_slot + n_frames) % ns;
  h->last_slot = idx[n_frames - 1];
  // the group's stream: groups rotate over the distinct slot streams, so that the tail of one group's launches overlaps
  // the head of the next group's (whose slots are different ones)
  const int si = (int)(h->batch_counter++ % h->streams.size());
  hipStream_t stream = h->streams[si];
  const int k = h->desc_next;
  h->desc_next = (k + 1) % xm_handle::DESC_RING;
  if (h->desc_used[k]) HIP_TRY(hipEventSynchronize(h->desc_ev[k]));  // the ring entry's previous batch has long finished
  FrameDesc* hd = h->h_descs + (size_t)k * ns;
  FrameDesc* dd = h->d_descs + (size_t)k * ns;
  int kinds[2] = {-1, -1};  // (stay -1 when the group fell back to frame-by-frame launches: nothing was attached then)
  int rc = enqueue_batch(h, idx.data(), v.evs.data(), v.dep.data(), v.bg.data(), n_frames, stream, hd, dd, true, true,
                         gpu_ms ? h->prof_ev : nullptr, kinds);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h->desc_ev[k], stream));
  h->desc_used[k] = true;
  hipEvent_t done = h->batch_ev[si][h->batch_ev_next[si]++ % 8];
  HIP_TRY(hipEventRecord(done, stream));
  if (done_out) *done_out = done;
  for (int f = 0; f < n_frames; ++f) {
    Slot& s = h->slots[idx[f]];
    s.order.note_group(done, stream);
    if (s.h_flags)  // slot gate + try-sorted verdict, read when the slot comes round again or in xm_sync
      s.prev.set(v.evs[f], v.dep[f], v.bg[f], nullptr, nullptr, s.last.host_tag, stream, h->plan().modes.try_sorted && s.last.sorted);
  }
  if (gpu_ms) {  // profile mode: durations of the group's dispatches (the events were attached to the dispatch packets)
    HIP_TRY(hipStreamSynchronize(stream));
    gpu_ms[0] = gpu_ms[1] = gpu_ms[2] = gpu_ms[3] = 0.0f;
    const int first = kinds[0] > 0 ? 0 : 1;  // no K0 / K0b launch on the verified-sorted keyed paths
    if (kinds[1] >= 0) {
      for (int i = first; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&gpu_ms[i], h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
      HIP_TRY(hipEventElapsedTime(&gpu_ms[3], h->prof_ev[2 * first], h->prof_ev[5]));
    }
  }
  return XM_OK;
}

}  // extern "C"

// XM_FLAG_ADAPTIVE_BATCH: everything on the pending list goes out as one group (at most ab_max = n_slots / 4 frames)
int flush_pending(xm_handle* h) {
  if (h->pending.empty()) return XM_OK;
  const size_t n = h->pending.size();
  BatchViews v;
  v.evs.reserve(n), v.dep.reserve(n), v.bg.reserve(n);
  for (const xm_handle::Deferred& d : h->pending) {
    v.evs.push_back(d.ev);
    v.dep.push_back(d.depth);
    v.bg.push_back(d.bgr);
  }
  h->pending.clear();  // (first: submit_group's callees pass through XM_ENTER-free paths only, but keep re-entry harmless)
  hipEvent_t done = nullptr;
  int rc = submit_group(h, v, nullptr, &done);
  if (rc) return rc;
  h->ab_inflight[h->ab_groups & 3] = done;
  h->ab_groups += 1;
  h->ab_frames += n;
  return XM_OK;
}

extern "C" {

int xm_process_batch(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                     const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out) {
  return process_batch_impl(h, x, y, t, p, t_dtype, offsets_host, n_frames, depth_out, bgr_out, nullptr);
}

int xm_process_batch_aos(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, float* depth_out,
                         uint8_t* bgr_out) {
  if (!eventcd16) return fail(XM_ERR_INVALID, "NULL event buffer");
  return process_batch_impl(h, nullptr, nullptr, nullptr, nullptr, XM_T_INT64, offsets_host, n_frames, depth_out, bgr_out, nullptr,
                            eventcd16);
}

int xm_profile_batch(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                     const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out, float gpu_ms[4]) {
  if (!gpu_ms) return fail(XM_ERR_INVALID, "NULL argument");
  return process_batch_impl(h, x, y, t, p, t_dtype, offsets_host, n_frames, depth_out, bgr_out, gpu_ms);
}

}  // extern "C"
