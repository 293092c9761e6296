// xm_api_ingest.hpp -- C-ABI: device-side ingest (N2): raw camera packets in, frames cut and processed on the device.
// The C entry points only; they run on the CALLER's thread (one call at a time per ingest, by the API's contract).  The state
// and who owns which part of it: xm_ingest_state.hpp; the out side and the frame pool: xm_ingest_out.hpp; the launch and copy
// sides: xm_ingest_launch.hpp; the stages of xm_ingest_create: xm_ingest_create.hpp
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

extern "C" {

int xm_ingest_create(xm_handle* h, const xm_ingest_config* cfg, xm_ingest** out) {
  if (!h || !cfg || !out) return fail(XM_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(xm_ingest_config)) return fail(XM_ERR_INVALID, "xm_ingest_config.struct_size mismatch");
  if (cfg->projector_fps <= 0) return fail(XM_ERR_INVALID, "projector_fps must be positive");
  XM_ENTER(h);
  Owned<xm_ingest, xm_ingest_destroy> owner(new (std::nothrow) xm_ingest());
  xm_ingest* const g = owner.get();
  if (!g) return fail(XM_ERR_NOMEM, "out of host memory");
  int rc = ingest_read_options(g->fx, h, cfg);
  if (!rc) rc = ingest_create_streams(g->fx, g);
  if (!rc) rc = ingest_create_device_rings(g->fx);
  if (!rc) rc = ingest_create_result_ring(g->fx, g->sh);
  if (rc) return rc;
  ingest_start_threads(g);
  *out = owner.release();
  return XM_OK;
}

void xm_ingest_destroy(xm_ingest* g) {
  if (!g) return;
  const IngestFixed& fx = g->fx;
  (void)hipSetDevice(fx.h->cfg.device);
  // the three threads leave through their queues, in this order: copy (forwards the stop behind everything else), launch, out
  // (behind the launch thread: nobody posts any more, and the stop comes behind every posted frame)
  if (fx.threaded) {
    IngestJob stop;
    stop.kind = JobKind::stop;
    ingest_post(g, stop);
    if (g->copy_th.joinable()) g->copy_th.join();
    if (g->th.joinable()) g->th.join();
  }
  if (fx.out_threaded) {
    OutJob stop;
    stop.stop = true;
    g->out.q.post(stop);
    if (g->out_th.joinable()) g->out_th.join();
  }
  if (fx.copy_stream) (void)hipStreamSynchronize(fx.copy_stream);
  if (fx.stream) (void)hipStreamSynchronize(fx.stream);
  if (fx.frame_stream) (void)hipStreamSynchronize(fx.frame_stream);
  if (fx.out_stream) (void)hipStreamSynchronize(fx.out_stream);
  if (fx.opt_trace) {  // (every thread has been joined: their counters can be read)
    const IngestLaunch& la = g->la;
    fprintf(stderr, "[ingest] %llu packets, %llu frames, ahead %d: launch side %.3f ms in jobs, of which %.3f ms waiting for verdicts and %.3f ms "
            "issuing frames; caller %.3f ms in push, %.3f ms of it waiting for staging entries\n", (unsigned long long)la.issued,
            (unsigned long long)la.frames_issued, fx.ahead, la.t_jobs_s * 1e3, la.t_block_s * 1e3, la.t_frames_s * 1e3, g->ca.push_host_s * 1e3,
            g->ca.push_wait_s * 1e3);
    fprintf(stderr, "[ingest] out side (%s): %.3f ms enqueuing %llu frames' copies + sequence numbers; the launch side waited %.3f ms for it\n",
            fx.cfg.flags & XM_INGEST_NO_LAUNCH_THREAD ? "inline" : "a thread of its own", (g->out.t_out_s + la.t_out_s) * 1e3,
            (unsigned long long)la.frames_issued, la.t_out_wait_s * 1e3);
  }
  for (auto p : g->sh.h_depth) ring_buf_free(p);
  for (auto p : g->sh.h_bgr) ring_buf_free(p);
  if (g->ca.pool) pool_close(g->ca.pool);
  ingest_stream_release(fx.h->cfg.device, g);
  delete g;
}

static int ingest_push(xm_ingest* g, const void* eventcd16, size_t n, bool pinned) {
  if (!g || (n && !eventcd16)) return fail(XM_ERR_INVALID, "NULL argument");
  const double c0 = ingest_now();
  const IngestFixed& fx = g->fx;
  if (n > fx.max_packet) return fail(XM_ERR_TOO_MANY, "packet of %zu events exceeds max_packet_events %llu", n, (unsigned long long)fx.max_packet);
  int rc = ingest_take_error(g);  // an earlier packet's launches failed
  if (rc) return rc;
  if (!fx.threaded) HIP_TRY(hipSetDevice(fx.h->cfg.device));
  IngestJob j;
  j.kind = JobKind::records;
  j.k = g->ca.pkt_next;
  j.n = n;
  if (!pinned && n && !g->ca.h_pkt[j.k]) {
    // the pinned twins of the staging entries, ALL of them at the first pageable push (one page-locking pause of the stream's
    // first packet instead of one on each of its first 16 packets); callers that push pinned packets or RAW words never pay
    HIP_TRY(hipSetDevice(fx.h->cfg.device));
    for (PinnedMem<uint4>& p : g->ca.h_pkt)
      if (!p) HIP_TRY(p.alloc(fx.max_packet, hipHostMallocDefault));
  }
  j.host = pinned ? eventcd16 : (const void*)g->ca.h_pkt[j.k];
  if ((rc = ingest_wait_entry(g, j.k))) return rc;
  if (n && !pinned) memcpy(g->ca.h_pkt[j.k], eventcd16, n * 16);  // pageable memory: through the pinned staging ring
  return ingest_accept_push(g, j, c0, false);
}

int xm_ingest_push(xm_ingest* g, const void* eventcd16, size_t n) { return ingest_push(g, eventcd16, n, false); }
int xm_ingest_push_pinned(xm_ingest* g, const void* eventcd16_pinned, size_t n) { return ingest_push(g, eventcd16_pinned, n, true); }

// The chunk is decoded on the DECODER's stream into the packet slot (free: its previous packet has been consumed) while the frame
// kernels of the packets before it keep running on the ingest's stream.  n_events != NULL: the decoding is waited for and the
// chunk's event count returned (and checked against max_packet_events: XM_ERR_TOO_MANY leaves decoder and ingest as they were).
// n_events == NULL: nothing is waited for -- the ingest's kernels read the count from device memory (round 4); a chunk that
// decodes to more than max_packet_events events is truncated to that many and the excess counted in the frames' `overflow`;
// the words are handed to the ingest's launch thread like a packet of records (pageable words: the call returns once they have been copied).
static int ingest_push_words(xm_ingest* g, xm_evt3* d, int format, const void* words_host, size_t n_words, int words_pinned, size_t* n_events) {
  if (!g || !d || (n_words && !words_host)) return fail(XM_ERR_INVALID, "NULL argument");
  if (d->format != format) return fail(XM_ERR_INVALID, "this decoder was created for %s", evt_format_name(d->format));
  if (g->fx.h != d->h) return fail(XM_ERR_INVALID, "the decoder and the ingest belong to different handles");
  if (n_words > d->max_words) return fail(XM_ERR_TOO_MANY, "chunk of %zu words exceeds max_words %zu", n_words, d->max_words);
  const double c0 = ingest_now();
  HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
  int rc = ingest_take_error(g);
  if (rc) return rc;
  IngestJob j;
  j.k = g->ca.pkt_next;
  if ((rc = ingest_wait_entry(g, j.k))) return rc;  // the staging entry's previous packet has been consumed
  if (n_events) {
    // the decoder runs here, on its own stream -- once the launch thread is done with every chunk handed to it before (those
    // use the same decoder: its state index and buffers are not to be touched from two threads) -- and the records then go to
    // the launch side like a packet that is already on the device
    if (g->fx.threaded) {
      g->sh.launch_q.wait_done(ingest_posted(g), &g->sh.err);
      if ((rc = ingest_take_error(g))) return rc;
    }
    size_t n = 0;
    rc = evt3_run(d, words_host, n_words, words_pinned != 0, g->fx.d_pkt[j.k], (size_t)g->fx.max_packet, d->stream, &n);
    *n_events = n;
    if (rc) return rc;  // (XM_ERR_TOO_MANY: neither the decoder nor the ingest has advanced -- push the chunk again in halves)
    j.kind = JobKind::on_device; j.n = n;
  } else {
    j.kind = JobKind::words; j.n = n_words; j.host = words_host; j.dec = d; j.pinned = words_pinned != 0;
  }
  // (pageable words are copied by the launch side: wait until it has done so)
  return ingest_accept_push(g, j, c0, j.kind == JobKind::words && !j.pinned);
}

int xm_ingest_push_evt3(xm_ingest* g, xm_evt3* d, const uint16_t* words_host, size_t n_words, int words_pinned, size_t* n_events) {
  return ingest_push_words(g, d, 3, words_host, n_words, words_pinned, n_events);
}
int xm_ingest_push_evt2(xm_ingest* g, xm_evt3* d, const uint32_t* words_host, size_t n_words, int words_pinned, size_t* n_events) {
  return ingest_push_words(g, d, 2, words_host, n_words, words_pinned, n_events);
}
int xm_ingest_push_evt21(xm_ingest* g, xm_evt3* d, const uint64_t* words_host, size_t n_words, int words_pinned, size_t* n_events) {
  return ingest_push_words(g, d, EVT_FMT_21, words_host, n_words, words_pinned, n_events);
}
int xm_ingest_push_dat(xm_ingest* g, xm_evt3* d, const void* records_host, size_t n_records, int records_pinned, size_t* n_events) {
  return ingest_push_words(g, d, EVT_FMT_DAT, records_host, n_records, records_pinned, n_events);
}

static int ingest_poll(xm_ingest* g, xm_ingest_frame* out, bool owned) {
  if (!g || !out) return fail(XM_ERR_INVALID, "NULL argument");
  const IngestFixed& fx = g->fx;
  IngestCaller& ca = g->ca;
  if (!fx.threaded && g->la.next_verdict <= g->la.issued) {  // (no launch thread: a frame whose verdict has arrived meanwhile goes out now)
    int rc = ingest_handle_verdicts(g, 0);
    if (rc) return rc;
  }
  const int slot = (int)(ca.next_seq % (uint64_t)fx.ring);
  const IngestStatus* st = fx.h_status + slot;
  const uint64_t want = ca.next_seq + 1;  // the entry's seq once frame next_seq has been published
  const uint64_t seq = __atomic_load_n(&st->seq, __ATOMIC_ACQUIRE);
  if (seq < want) return 0;  // not there yet
  IngestStatus v;
  memcpy(&v, st, sizeof v);
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  const uint64_t seq2 = __atomic_load_n(&st->seq, __ATOMIC_ACQUIRE);  // did the producer rewrite the entry while it was read?
  bool lapped = seq > want || seq2 != seq;  // the ring holds a later frame here (or is being rewritten): this one is lost
  uint64_t newest_slot = 0;
  memset(out, 0, sizeof *out);
  out->seq = ca.next_seq;
  if (!lapped) {  // (the caller's thread swaps these pointers, below: it may read them without res_mu)
    out->depth = g->sh.h_depth[slot];
    out->bgr = g->sh.h_bgr[slot];
  }
  const bool wants[2] = {out->depth != nullptr, out->bgr != nullptr};
  void* spare[2] = {nullptr, nullptr};
  if (!lapped && owned && (wants[0] || wants[1]) && pool_take_spares(g, wants, spare)) {
    // The slot's buffers leave with the frame and the slot gets spare ones -- in one step with the out side's "these are the
    // buffers of frame f" (res_mu): a slot that says another frame by now has been lapped, its buffers are a DMA's target.
    {
      std::lock_guard<std::mutex> lk(g->sh.res_mu);
      newest_slot = g->sh.slot_frame[slot];
      if (newest_slot == want) {
        if (wants[0]) g->sh.h_depth[slot] = (float*)spare[0];
        if (wants[1]) g->sh.h_bgr[slot] = (uint8_t*)spare[1];
        out->owned = 1;
      } else {
        lapped = true;
      }
    }
    pool_give_back(ca.pool, spare, out->owned ? (int)wants[0] + (int)wants[1] : 0);
  }
  out->lost = lapped ? 1 : 0;
  if (lapped) {
    out->depth = nullptr;
    out->bgr = nullptr;
    if (fx.opt_trace) fprintf(stderr, "[ingest] lapped: slot %d want %llu seq %llu seq2 %llu (frames issued %llu, packets handled %llu)\n", slot,
                              (unsigned long long)want, (unsigned long long)seq, (unsigned long long)seq2,
                              (unsigned long long)g->sh.frames_issued_pub.load(), (unsigned long long)g->sh.handled.load());
    // Nothing of the entry can be trusted for frame next_seq (no statistics, no images: depth / bgr stay NULL).
    // Resume with the oldest frame the ring may still hold intact.
    const uint64_t newest = std::max(std::max(seq, seq2), newest_slot);  // >= want + ring - 1
    ca.next_seq = std::max<uint64_t>(ca.next_seq + 1, newest >= (uint64_t)fx.ring ? newest - (uint64_t)fx.ring : 0);
    return 1;
  }
  out->n_events = v.n_events;
  out->t_first = v.t_first;
  out->t_last = v.t_last;
  out->n_inliers = v.n_inliers;
  out->n_index_errors = v.n_index_errors;
  out->live_after = v.live_after;
  out->overflow = v.overflow;
  out->push_seq = v.push_seq;
  out->push_to_publish_us = v.latency_us;
  ca.last_kept = v.n_used;
  ca.next_seq += 1;
  return 1;
}

int xm_ingest_poll(xm_ingest* g, xm_ingest_frame* out) { return ingest_poll(g, out, false); }

int xm_ingest_poll_owned(xm_ingest* g, xm_ingest_frame* out, xm_frame_pool** pool) {
  const int rc = ingest_poll(g, out, true);
  if (pool) *pool = rc == 1 && out->owned ? g->ca.pool : nullptr;
  return rc;
}

// A call of the caller's thread, like push and poll: `posted` and `next_seq` are its own counts, the launch side's progress comes
// through the two atomics (without a launch thread the caller IS the launch side and reads its `issued` directly)
int xm_ingest_backlog(xm_ingest* g, int wait_below, uint64_t* backlog) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  const bool threaded = g->fx.threaded;
  uint64_t posted = 0, hd = 0;
  const auto now = [&]() -> uint64_t {
    posted = threaded ? g->ca.posted : g->la.issued;
    // (handled first: a frame is counted in frames_issued_pub before its packet is in handled)
    hd = g->sh.handled.load(std::memory_order_acquire);
    const uint64_t fi = g->sh.frames_issued_pub.load(std::memory_order_acquire);
    return (fi - std::min(fi, g->ca.next_seq)) + (posted - std::min(posted, hd));
  };
  uint64_t b = now();
  if (wait_below > 0) {
    const double c0 = ingest_now();
    bool waited = false;
    while (b >= (uint64_t)wait_below && hd < posted) {  // (until there is room, or nothing is left in flight that waiting could settle)
      if (!threaded) {
        int rc = ingest_handle_verdicts(g, g->la.next_verdict);
        if (rc) return rc;
      } else {
        if (g->sh.err.code(std::memory_order_relaxed)) return ingest_take_error(g);
        for (int k = 0; k < 64; ++k) __builtin_ia32_pause();
      }
      waited = true;
      b = now();
    }
    if (waited) {  // (counted like a push that waited for a staging entry: the caller's time, spent waiting for the GPU)
      const double dt = ingest_now() - c0;
      g->ca.stage_waits += 1;
      g->ca.push_wait_s += dt;
      g->ca.push_host_s += dt;
    }
  }
  if (backlog) *backlog = b;
  return XM_OK;
}

int xm_ingest_frame_valid(xm_ingest* g, uint64_t seq) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  // (k_ing_publish zeroes the slot's sequence number before anything of the next frame is written into the slot's buffers: the
  //  frame kernels' K2 writes device memory, the copy into this slot comes behind k_ing_publish on the frame stream's event)
  return __atomic_load_n(&g->fx.h_status[seq % (uint64_t)g->fx.ring].seq, __ATOMIC_ACQUIRE) == seq + 1 ? 1 : 0;
}

int xm_ingest_last_frame_kept(xm_ingest* g, uint64_t* n_kept) {
  if (!g || !n_kept) return fail(XM_ERR_INVALID, "NULL argument");
  *n_kept = g->ca.last_kept;
  return XM_OK;
}

// the frame-filter stage's scratch, once (IngestFrameFilter): sized for every filter the rig's LUT allows
static int ingest_frame_filter_alloc(xm_ingest* g) {
  IngestFrameFilter& ff = g->ff;
  const IngestFixed& fx = g->fx;
  const xm_handle* h = fx.h;
  ff.cells_xy = (u32)h->tb.cam_w * (u32)h->tb.cam_h;
  ff.yt_w = h->plan().cols.xr_max + 1;
  ff.yt_wrap = h->plan().cols.xr_min < 0;
  const u64 cells_yt = ff.yt_w > 0 ? (u64)ff.yt_w * (u64)h->tb.cam_h : 0;
  ff.yt_ok = cells_yt > 0 && cells_yt <= ING_YT_MAX_CELLS;
  ff.cells_yt = ff.yt_ok ? (u32)cells_yt : 0u;
  const size_t cells = std::max(ff.cells_xy, ff.cells_yt), blocks = (cells + FF_BLOCK - 1) / FF_BLOCK;
  HIP_TRY(hipSetDevice(h->cfg.device));
  for (Event& e : ff.read_ev) HIP_TRY(e.create());
  HIP_TRY(ff.d_last.alloc(cells));
  HIP_TRY(ff.d_first.alloc(cells));
  HIP_TRY(ff.d_sums.alloc(blocks));
  HIP_TRY(ff.d_survivors.alloc(std::max<size_t>((size_t)fx.dev.mirror, cells)));
  HIP_TRY(ff.d_descs.alloc(ING_VRING));
  HIP_TRY(ff.d_infos.alloc(ING_VRING));
  HIP_TRY(ff.d_ctl.alloc(1));
  HIP_TRY(hipMemset(ff.d_last, 0, cells * sizeof(u32)));
  HIP_TRY(hipMemset(ff.d_first, 0, cells * sizeof(u32)));
  HIP_TRY(hipMemset(ff.d_sums, 0, blocks * sizeof(u32)));
  HIP_TRY(hipMemset(ff.d_descs, 0, sizeof(FrameDesc) * ING_VRING));
  HIP_TRY(hipMemset(ff.d_infos, 0, sizeof(FrameFilterInfo) * ING_VRING));
  HIP_TRY(hipMemset(ff.d_ctl, 0, sizeof(FrameFilterCtl)));
  HIP_TRY(hipDeviceSynchronize());  // (default-stream memsets: the ingest's non-blocking streams do not wait for them)
  ff.ready = true;
  return XM_OK;
}

int xm_ingest_set_frame_filter(xm_ingest* g, int filter, int intended_semantics) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (filter != 0 && (filter < FILTER_FIRST_PER_YT || filter > FILTER_MEAN_PER_XY)) return fail(XM_ERR_INVALID, "unknown filter %d", filter);
  int rc = ingest_take_error(g);
  if (rc) return rc;
  if (filter && !g->ff.ready && (rc = ingest_frame_filter_alloc(g))) return rc;
  if (filter == FILTER_FIRST_PER_YT && !g->ff.yt_ok)
    return fail(XM_ERR_INVALID, "FirstEventPerYT: a cell map of %d rows x %d columns (the rectify LUT's largest entry + 1) exceeds %llu cells",
                g->fx.h->tb.cam_h, g->ff.yt_w, (unsigned long long)ING_YT_MAX_CELLS);
  // ordered like a push: the packets handed in before this call keep the filter they were pushed under
  IngestJob j;
  j.kind = JobKind::set_filter;
  j.filter = filter;
  j.intended = intended_semantics ? 1 : 0;
  return ingest_submit(g, j, false);
}

// the surface stage's scratch and ring, once (IngestSurface)
static int ingest_surface_alloc(xm_ingest* g, int ring) {
  IngestSurface& sf = g->sf;
  const xm_handle* h = g->fx.h;
  sf.cells = (size_t)h->tb.cam_w * h->tb.cam_h;
  sf.stride = (sf.cells + FS_CPT - 1) / FS_CPT * FS_CPT;
  sf.max_chunk_blocks = frame_max_chunk_blocks("XM_FS_MAX_BLOCKS");
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(sf.d_map.alloc(sf.stride));
  HIP_TRY(sf.d_acc.alloc(1));
  HIP_TRY(sf.d_ring.alloc((size_t)ring * sf.cells * 8));
  if (int rc = sf.r.alloc(ring)) return rc;
  HIP_TRY(hipMemset(sf.d_map, 0, sf.stride * sizeof(u32)));
  HIP_TRY(hipMemset(sf.d_acc, 0, sizeof(FsAcc)));
  HIP_TRY(hipDeviceSynchronize());  // (default-stream memsets: the ingest's non-blocking streams do not wait for them)
  sf.r.ready = true;
  return XM_OK;
}

int xm_ingest_set_surface_output(xm_ingest* g, int select, int dtype, int ring) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (select != 0 && select != XM_SURFACE_LAST && select != XM_SURFACE_FIRST)
    return fail(XM_ERR_INVALID, "select must be 0 (off), XM_SURFACE_LAST or XM_SURFACE_FIRST");
  if (select && dtype != XM_T_FLOAT32 && dtype != XM_T_FLOAT64) return fail(XM_ERR_INVALID, "a time surface is XM_T_FLOAT32 or XM_T_FLOAT64");
  if (ring < 0 || ring > 65536) return fail(XM_ERR_INVALID, "ring must lie in 0 .. 65536");
  int rc = ingest_take_error(g);
  if (rc) return rc;
  if (select) {
    const int want = g->sf.r.want_ring(ring, g->fx.ring);
    if (!g->sf.r.ready && (rc = ingest_surface_alloc(g, want))) return rc;
    if (g->sf.r.ring != want) return fail(XM_ERR_INVALID, "the surface ring holds %d entries since the first call that switched the stage on", g->sf.r.ring);
  }
  // ordered like a push: the packets handed in before this call keep the setting they were pushed under
  IngestJob j;
  j.kind = JobKind::set_surface;
  j.surf_select = select;
  j.surf_dtype = select ? dtype : 0;
  return ingest_submit(g, j, false);
}

int xm_ingest_surface_dtype(xm_ingest* g, uint64_t seq) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  const IngestSurface& sf = g->sf;
  if (!sf.r.ready) return 0;
  const u64 t = __atomic_load_n(sf.r.h_tag + sf.r.entry(seq), __ATOMIC_ACQUIRE);
  return surface_tag_names(t, seq) ? surface_tag_dtype(t) : 0;
}

int xm_ingest_copy_surface(xm_ingest* g, uint64_t seq, void* dst, int mem, xm_frame_surface_stats* stats) {
  if (!g || !dst) return fail(XM_ERR_INVALID, "NULL argument");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  const IngestSurface& sf = g->sf;
  return sf.r.read(
      seq, [&](u64 t) { return surface_tag_names(t, seq); },
      [&](size_t e, u64 t, const FsStats&) {
        HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
        HIP_TRY(hipMemcpy(dst, sf.d_ring + e * sf.cells * 8, sf.cells * t_size(surface_tag_dtype(t)),
                          mem == XM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        if (mem == XM_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(nullptr));
        return (int)XM_OK;
      },
      stats);
}

// the cloud stage's scratch and ring, once (IngestCloud)
static int ingest_cloud_alloc(xm_ingest* g, size_t max_points, int ring) {
  IngestCloud& cl = g->cl;
  const xm_handle* h = g->fx.h;
  cl.max_points = max_points;
  cl.cap = (u32)g->fx.dev.mirror;  // (a cut frame is contiguous in the event ring: at most half of it)
  cl.max_chunk_blocks = frame_max_chunk_blocks("XM_FC_MAX_BLOCKS");
  const size_t n_seg = (size_t)cl.cap / 64 + 1;
  HIP_TRY(hipSetDevice(h->cfg.device));
  HIP_TRY(cl.d_acc.alloc(1));
  HIP_TRY(cl.d_code.alloc(cl.cap));
  HIP_TRY(cl.d_cnt.alloc(n_seg));
  HIP_TRY(cl.d_off.alloc(n_seg));
  HIP_TRY(cl.d_ring.alloc((size_t)ring * max_points * 3));
  if (int rc = cl.r.alloc(ring)) return rc;
  HIP_TRY(hipMemset(cl.d_acc, 0, sizeof(FcAcc)));
  HIP_TRY(hipDeviceSynchronize());  // (default-stream memsets: the ingest's non-blocking streams do not wait for them)
  cl.r.ready = true;
  return XM_OK;
}

int xm_ingest_set_cloud_output(xm_ingest* g, int on, int64_t max_points, int ring) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (ring < 0 || ring > 65536) return fail(XM_ERR_INVALID, "ring must lie in 0 .. 65536");
  if (on && (max_points <= 0 || max_points >= (1ll << 31))) return fail(XM_ERR_INVALID, "max_points must lie in 1 .. 2^31 - 1");
  if (on && !g->fx.h->fcloud.has_tables)
    return fail(XM_ERR_INVALID, "the cloud stage needs the float rectify maps and Q: call xm_cloud_set_tables on the handle first");
  int rc = ingest_take_error(g);
  if (rc) return rc;
  if (on) {
    const int want = g->cl.r.want_ring(ring, g->fx.ring);
    if (!g->cl.r.ready && (rc = ingest_cloud_alloc(g, (size_t)max_points, want))) return rc;
    if (g->cl.r.ring != want || g->cl.max_points != (size_t)max_points)
      return fail(XM_ERR_INVALID, "the cloud ring holds %d entries of %zu rows since the first call that switched the stage on", g->cl.r.ring,
                  g->cl.max_points);
  }
  // ordered like a push: the packets handed in before this call keep the setting they were pushed under
  IngestJob j;
  j.kind = JobKind::set_cloud;
  j.cloud_on = on ? 1 : 0;
  return ingest_submit(g, j, false);
}

int xm_ingest_copy_cloud(xm_ingest* g, uint64_t seq, float* dst, int mem, xm_frame_cloud_stats* stats) {
  if (!g || (!dst && !stats)) return fail(XM_ERR_INVALID, "NULL argument");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  const IngestCloud& cl = g->cl;
  return cl.r.read(
      seq, [&](u64 t) { return cloud_tag_names(t, seq); },
      [&](size_t e, u64, const FcStats& st) {
        const size_t rows = (size_t)std::min<u64>(st.n_inliers, cl.max_points);
        if (!dst || !rows) return (int)XM_OK;
        HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
        HIP_TRY(hipMemcpy(dst, cl.d_ring + e * cl.max_points * 3, rows * 12, mem == XM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        if (mem == XM_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(nullptr));
        return (int)XM_OK;
      },
      stats);
}

// the record stage's scratch and ring, once (IngestRecord)
static int ingest_record_alloc(xm_ingest* g, size_t max_words, int ring) {
  IngestRecord& rec = g->rec;
  rec.max_words = max_words;
  rec.cap = (u32)g->fx.dev.mirror;  // (a cut frame is contiguous in the event ring: at most half of it)
  rec.max_chunk_blocks = frame_max_chunk_blocks("XM_ENC_MAX_BLOCKS");
  const size_t n_seg = (size_t)rec.cap / 64 + 1;
  HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
  HIP_TRY(rec.d_code.alloc(rec.cap));
  HIP_TRY(rec.d_cnt.alloc(n_seg));
  HIP_TRY(rec.d_off.alloc(n_seg));
  HIP_TRY(rec.d_ring.alloc((size_t)ring * max_words));
  if (int rc = rec.r.alloc(ring)) return rc;
  HIP_TRY(hipDeviceSynchronize());  // (default-stream memsets: the ingest's non-blocking streams do not wait for them)
  rec.r.ready = true;
  return XM_OK;
}

int xm_ingest_set_record_output(xm_ingest* g, int on, int use_vectors, int64_t max_words, int ring) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (ring < 0 || ring > 65536) return fail(XM_ERR_INVALID, "ring must lie in 0 .. 65536");
  if (on && (max_words <= 0 || max_words >= (1ll << 31))) return fail(XM_ERR_INVALID, "max_words must lie in 1 .. 2^31 - 1");
  int rc = ingest_take_error(g);
  if (rc) return rc;
  if (on) {
    const int want = g->rec.r.want_ring(ring, g->fx.ring);
    if (!g->rec.r.ready && (rc = ingest_record_alloc(g, (size_t)max_words, want))) return rc;
    if (g->rec.r.ring != want || g->rec.max_words != (size_t)max_words)
      return fail(XM_ERR_INVALID, "the record ring holds %d entries of %zu words since the first call that switched the stage on", g->rec.r.ring,
                  g->rec.max_words);
  }
  // ordered like a push: the packets handed in before this call keep the setting they were pushed under
  IngestJob j;
  j.kind = JobKind::set_record;
  j.record_on = on ? 1 : 0;
  j.record_vectors = use_vectors ? 1 : 0;
  return ingest_submit(g, j, false);
}

int xm_ingest_copy_record(xm_ingest* g, uint64_t seq, uint16_t* dst, int mem, xm_evt3_record_stats* stats) {
  if (!g || (!dst && !stats)) return fail(XM_ERR_INVALID, "NULL argument");
  if (mem != XM_MEM_HOST && mem != XM_MEM_DEVICE) return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST or XM_MEM_DEVICE");
  const IngestRecord& rec = g->rec;
  return rec.r.read(
      seq, [&](u64 t) { return cloud_tag_names(t, seq); },
      [&](size_t e, u64, const EncStats& st) {
        if (!dst || !st.n_words || st.n_words > rec.max_words) return (int)XM_OK;  // (all or nothing: the entry holds no word of such a frame)
        HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
        HIP_TRY(hipMemcpy(dst, rec.d_ring + e * rec.max_words, (size_t)st.n_words * 2, mem == XM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        if (mem == XM_MEM_DEVICE) HIP_TRY(hipStreamSynchronize(nullptr));
        return (int)XM_OK;
      },
      stats);
}

int xm_ingest_flush(xm_ingest* g) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(g->fx.h->cfg.device));
  IngestJob j;
  j.kind = JobKind::flush;
  return ingest_submit(g, j, true);
}

int xm_ingest_reset(xm_ingest* g) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  int rc = xm_ingest_flush(g);
  if (rc) return rc;
  // RobustTriggerFinder.reset(): the buffered events are discarded (trigger_finder.py:116-119).  The stream indices start over
  // (nothing live refers to the old ones); the frame counter and the sticky overflow count go on.
  IngestState z;
  HIP_TRY(hipMemcpy(&z, g->fx.dev.st, sizeof z, hipMemcpyDeviceToHost));
  z.start_abs = z.write_abs = z.p_head = z.p_tail = 0;
  z.last_t = 0;
  z.span_ok = 0;
  HIP_TRY(hipMemcpy(g->fx.dev.st, &z, sizeof z, hipMemcpyHostToDevice));
  // the surface, cloud and record stages keep their settings; their rings are emptied
  g->sf.r.clear();
  g->cl.r.clear();
  g->rec.r.clear();
  // The activity filter's history goes too: a reset is "the stream starts over" (the reference resets when a recording loops,
  // depth_reprojection.py:76) and its stamps then start below everything the history holds -- against the old history every
  // event with a neighbour that ever fired would pass.  (Metavision's filter object keeps its state there; the frames behind
  // the first period of a loop are what differs.)
  const ActDev& act = g->fx.act_base;
  if (act.last_ts) {
    std::vector<long long> init((size_t)act.cam_w * act.cam_h, ING_NO_TS);
    HIP_TRY(hipMemcpy(act.last_ts, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipDeviceSynchronize());  // (default-stream work: the ingest's non-blocking streams do not wait for it)
  return XM_OK;
}

// the device's counters after everything pushed so far has run (synchronises like xm_ingest_flush)
int xm_ingest_device_stats(xm_ingest* g, uint64_t* frames_cut, uint64_t* events_appended, uint64_t* events_dropped, uint64_t* events_live) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  int rc = xm_ingest_flush(g);
  if (rc) return rc;
  IngestState z;
  HIP_TRY(hipMemcpy(&z, g->fx.dev.st, sizeof z, hipMemcpyDeviceToHost));
  if (frames_cut) *frames_cut = z.frames;
  if (events_appended) *events_appended = z.appended;
  if (events_dropped) *events_dropped = z.overflow;
  if (events_live) *events_live = z.write_abs - z.start_abs;
  return XM_OK;
}

int xm_ingest_host_stats(xm_ingest* g, uint64_t* pushes, double* host_seconds_in_push, uint64_t* staging_waits, double* seconds_waiting) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (pushes) *pushes = g->ca.push_calls;
  if (host_seconds_in_push) *host_seconds_in_push = g->ca.push_host_s;
  if (staging_waits) *staging_waits = g->ca.stage_waits;
  if (seconds_waiting) *seconds_waiting = g->ca.push_wait_s;
  return XM_OK;
}

int xm_ingest_activity_stats(xm_ingest* g, uint64_t* sequential_packets) {
  if (!g) return fail(XM_ERR_INVALID, "NULL argument");
  if (sequential_packets) *sequential_packets = 0;
  if (!g->fx.act_base.last_ts) return XM_OK;
  int rc = xm_ingest_flush(g);
  if (rc) return rc;
  u32 c[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // (both sets' control words)
  HIP_TRY(hipMemcpy(c, g->fx.act_base.ctl, sizeof c, hipMemcpyDeviceToHost));
  if (sequential_packets) *sequential_packets = (uint64_t)c[2] + c[6];
  return XM_OK;
}

int xm_ingest_fused_first_passes(xm_ingest* g, uint64_t* n) {
  if (!g || !n) return fail(XM_ERR_INVALID, "NULL argument");
  int rc = xm_ingest_flush(g);  // (the launch side's count: read when it is idle, behind the flush's wait_done)
  if (rc) return rc;
  *n = g->la.act_fused_count;
  return XM_OK;
}

}  // extern "C"
