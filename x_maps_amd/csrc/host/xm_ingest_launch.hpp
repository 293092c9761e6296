// xm_ingest_launch.hpp -- device-side ingest (N2), the launch and copy sides: a packet's way to the device, its ingest kernels,
// the verdicts and the kernels of the frames they cut; the two threads' main loops and the caller's door to them
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; state and threads: xm_ingest_state.hpp)
#pragma once

namespace {

// ---- frames ---------------------------------------------------------------------------------------------------------------

// the frame-filter stage's arguments for verdict entry vi under `filter` (FILTER_*) with the semantics `intended`
FrameFilterDev ingest_frame_filter_dev(const xm_ingest* g, int vi, int filter, int intended) {
  const IngestFrameFilter& ff = g->ff;
  const xm_handle* h = g->fx.h;
  const bool yt = filter == FILTER_FIRST_PER_YT;
  FrameFilterDev f{};
  f.cut = g->fx.d_descs + vi;
  f.out = ff.d_descs + vi;
  f.info = ff.d_infos + vi;
  f.ctl = ff.d_ctl;
  f.last = ff.d_last;
  f.first = ff.d_first;
  f.sums = ff.d_sums;
  f.survivors = ff.d_survivors;
  f.lut = h->tb.lut;
  f.cam_w = h->tb.cam_w;
  f.cam_h = h->tb.cam_h;
  f.map_w = yt ? ff.yt_w : h->tb.cam_w;
  f.n_cells = yt ? ff.cells_yt : ff.cells_xy;
  f.filter = filter;
  f.use_first = intended && filter != FILTER_LAST_PER_XY;
  f.wrap = yt && ff.yt_wrap;
  return f;
}

// [frame event filter ->] K0 -> K1 -> K2 -> statistics for the frame that packet `push_no` cut (n events), on the frame stream; its
// copies to the out side
int ingest_issue_frame(xm_ingest* g, uint64_t push_no, u64 n) {
  const IngestFixed& fx = g->fx;
  IngestLaunch& la = g->la;
  xm_handle* h = fx.h;
  hipStream_t s = fx.frame_stream;
  const int vi = (int)(push_no % ING_VRING);
  const FrameDesc* cut = fx.d_descs + vi;
  // the filter the packet was pushed under: its stage leaves the entry's second descriptor (the survivors, <= n of them), on
  // which everything below runs; n stays the bound of the grids.  No filter: the launches below and nothing else
  const int flt = la.push_filter[vi] & 7;
  const FrameDesc* desc = flt ? g->ff.d_descs + vi : cut;
  if (la.frames_since_clear >= fx.clear_every) {  // (stream-ordered behind every frame so far)
    hipLaunchKernelGGL(k_reset_slot, dim3(1024), dim3(BLOCK), 0, s, fx.dev.slot, fx.dev.key_frame, (u64)h->plan().dims.key_cells, (unsigned char*)nullptr);
    la.frames_since_clear = 0;
  }
  la.frames_since_clear += 1;
  // the surface stage the packet was pushed under: the cut frame's time surface into ring entry (frame number % ring), in front
  // of everything else that reads the frame.  Its reads of the ring are over before the event the ingest stream waits for below
  // (the filter stage's, else K1's) is recorded on this stream.  Stage off: nothing is launched
  if (const int sfs = la.push_surface[vi]) {
    IngestSurface& sf = g->sf;
    const size_t e = sf.r.entry(la.frames_issued);
    const int dt = sfs >> 2;
    FsArgs a{};
    a.desc = cut;
    a.map = sf.d_map;
    a.acc = sf.d_acc;
    a.stats = sf.r.d_stats + e;
    a.out = sf.d_ring + e * sf.cells * 8;
    a.tag = sf.r.h_tag + e;
    a.tag_value = surface_tag(la.frames_issued, dt);
    a.host_stats = sf.r.h_stats + e;
    a.cells = (u32)sf.cells, a.map_stride = (u32)sf.stride;
    a.cam_w = h->tb.cam_w, a.cam_h = h->tb.cam_h;
    a.use_polarity = 0, a.select = sfs & 3;
    a.max_chunk_blocks = sf.max_chunk_blocks;
    launch_frame_surfaces(a, 1, n, dt, s);
  }
  // the cloud stage the packet was pushed under: the cut frame's point cloud (its first max_points rows) into ring entry (frame
  // number % ring), behind the surface stage and in front of everything else that reads the frame, under the same ordering.
  // Stage off: nothing is launched
  if (la.push_cloud[vi]) {
    IngestCloud& cl = g->cl;
    const size_t e = cl.r.entry(la.frames_issued);
    FcArgs a{};
    a.desc = cut;
    a.cap = cl.cap;
    a.max_rows = (u32)cl.max_points;
    a.tb = h->tb;
    a.mapx = h->fcloud.mapx.get(), a.mapy = h->fcloud.mapy.get(), a.Q = h->fcloud.q;
    a.acc = cl.d_acc;
    a.code = cl.d_code;
    a.cnt = cl.d_cnt;
    a.off = cl.d_off;
    a.stats = cl.r.d_stats + e;
    a.cloud = cl.d_ring + e * cl.max_points * 3;
    a.tag = cl.r.h_tag + e;
    a.tag_value = cloud_tag(la.frames_issued);
    a.host_stats = cl.r.h_stats + e;
    a.use_polarity = 0;
    a.max_chunk_blocks = cl.max_chunk_blocks;
    launch_frame_clouds(a, 1, std::min<u64>(n, cl.cap), s);
  }
  // the record stage the packet was pushed under: the cut frame's EVT 3.0 words (all of them, or none where they exceed max_words)
  // into ring entry (frame number % ring), behind the cloud stage and in front of everything else that reads the frame, under the
  // same ordering.  Stage off: nothing is launched
  if (const int rcs = la.push_record[vi]) {
    IngestRecord& rec = g->rec;
    const size_t e = rec.r.entry(la.frames_issued);
    EncArgs a{};
    a.desc = cut;
    a.cap = rec.cap;
    a.max_words = (u32)rec.max_words;
    a.code = rec.d_code;
    a.cnt = rec.d_cnt;
    a.off = rec.d_off;
    a.stats = rec.r.d_stats + e;
    a.words = rec.d_ring + e * rec.max_words;
    a.tag = rec.r.h_tag + e;
    a.tag_value = cloud_tag(la.frames_issued);
    a.host_stats = rec.r.h_stats + e;
    a.use_vectors = rcs >> 1;
    a.max_chunk_blocks = rec.max_chunk_blocks;
    launch_frame_records(a, 1, std::min<u64>(n, rec.cap), s);
  }
  // one EventCD frame in descriptor form: grids from at least two events, the tiled K1's block from the frame itself
  if (flt) {
    launch_frame_filter(ingest_frame_filter_dev(g, vi, flt, la.push_filter[vi] >> 3), n, s);
    // the stage's last launch is the last reader of the cut frame in the ring (K0 / K1 read the survivors): the ingest stream waits
    // for it instead of for K1
    hipEvent_t ev = g->ff.read_ev[la.frames_issued % 8];
    HIP_TRY(hipEventRecord(ev, s));
    HIP_TRY(hipStreamWaitEvent(fx.stream, ev, 0));
  }
  const FrameGroup one{desc, 1, n < 2 ? 2 : n, n, false};
  // K0 (general path: the cut frame is sorted whenever the camera stream is, but nothing here relies on it)
  launch_k0<long long, true, false>(one, s);
  // K1: tiled where a group of such frames would be, else one thread per event
  if (int rc = launch_k1<long long, true, false>(h, one, batch_path(h->plan(), n), false, false, s)) return rc;
  // the ingest stream must not append over the frame's events (dead, but still in the ring) before K1 has read them: whatever
  // is issued on it from now on waits for this event; what has been issued already fits the room k_ing_segment keeps (`ahead`)
  if (!flt) {
    hipEvent_t ev = fx.k1_ev[la.frames_issued % 8];
    HIP_TRY(hipEventRecord(ev, s));
    HIP_TRY(hipStreamWaitEvent(fx.stream, ev, 0));
  }
  // K2 writes device output frame o = frame number % ING_NOUT (k_ing_segment put its address into the descriptor) -- once the DMA
  // of the frame that used it last has left
  const uint64_t f = la.frames_issued;
  const int o = (int)(f % ING_NOUT);
  if (f >= (uint64_t)ING_NOUT) {
    // (the event must have been RECORDED by the out side before this stream can be told to wait for it)
    const double tw = ingest_now();
    if (int rc = ingest_out_wait(g, f - ING_NOUT + 1)) return rc;
    la.t_out_wait_s += ingest_now() - tw;
    HIP_TRY(hipStreamWaitEvent(s, fx.out_ev[o], 0));
  }
  if (h->cfg.view == XM_VIEW_PROJECTOR && h->plan().modes.k2_direct) return fail(XM_ERR_INVALID, "ingest needs the tiled frame kernel (XM_K2_DIRECT is set)");
  launch_frame_kernel(h, one, KM_KEY64, s);
  // the frame's statistics into its status entry while the slot's counters and the frame's events are still the frame's ...
  hipLaunchKernelGGL(k_ing_publish, dim3(1), dim3(64), 0, s, fx.dev.st, desc, (const IngFrameInfo*)(fx.d_infos + vi), (IngestStatus*)fx.h_status, (u64)push_no,
                     flt ? cut : (const FrameDesc*)nullptr, flt ? &(g->ff.d_infos + vi)->n_dropped : (u32*)nullptr);
  HIP_TRY(hipGetLastError());
  // ... device -> pinned result ring by DMA and the entry's sequence number behind it on the OUT stream: a 6 MB frame is 140 us
  // on the link, during which the frame stream already runs the next frame's kernels (on one stream the frames came out one DMA
  // + one kernel chain apart).  (frame numbers count on both sides: the verdicts arrive in packet order)
  HIP_TRY(hipEventRecord(fx.k2_ev[o], s));
  OutJob job;
  job.frame_no = f;
  job.slot = (int)(f % (uint64_t)fx.ring);
  job.o = o;
  job.desc = cut;
  job.t_push = la.push_t[vi];
  job.serial = fx.out_on_frame_stream || la.out_serial_now;
  if (int rc = ingest_out_hand_over(g, job)) return rc;
  la.entry_frame[vi] = f + 1;
  la.frames_issued += 1;
  g->sh.frames_issued_pub.store(la.frames_issued, std::memory_order_release);
  return XM_OK;
}

// Verdicts in packet order; for a packet that cut a frame, its kernels.  block_upto: wait for the verdicts of packets <= that
// number (0: take what is there).
int ingest_handle_verdicts(xm_ingest* g, uint64_t block_upto) {
  IngestLaunch& la = g->la;
  while (la.next_verdict <= la.issued) {
    const uint64_t v = la.next_verdict;
    const IngVerdict* e = g->fx.h_verdicts + (v % ING_VRING);
    if (__atomic_load_n(&e->push_no, __ATOMIC_ACQUIRE) != v) {
      if (v > block_upto) return XM_OK;
      const double cb = ingest_now();
      struct Acc { double& a; double t0; ~Acc() { a += ingest_now() - t0; } } acc{la.t_block_s, cb};
      unsigned spins = 0;
      while (__atomic_load_n(&e->push_no, __ATOMIC_ACQUIRE) != v) {
        __builtin_ia32_pause();
        if ((++spins & 0x3ff) == 0) {  // make sure the runtime has handed the launches to the GPU; an idle stream without the
          hipError_t q = hipStreamQuery(g->fx.stream);  // verdict would be a lost launch: report it instead of spinning for ever
          if (q == hipSuccess && __atomic_load_n(&e->push_no, __ATOMIC_ACQUIRE) != v)
            return fail(XM_ERR_HIP, "ingest: packet %llu left no verdict", (unsigned long long)v);
          if (q != hipSuccess && q != hipErrorNotReady) HIP_TRY(q);
        }
      }
    }
    const u64 info = __atomic_load_n(&e->info, __ATOMIC_RELAXED);
    if (info >> 63) {
      const double cf = ingest_now();
      int rc = ingest_issue_frame(g, v, info & ~(1ull << 63));
      la.t_frames_s += ingest_now() - cf;
      if (rc) return rc;
    }
    la.next_verdict = v + 1;
    g->sh.handled.store(v, std::memory_order_release);
  }
  return XM_OK;
}

// ---- packets ----------------------------------------------------------------------------------------------------------------

// upper bound of the events one word of the decoder's format yields (for the host's bookkeeping: an EVT 3.0 vector word yields up
// to 12, an EVT 2.1 word up to 32, an EVT 2.0 word or a DAT record at most one)
int ingest_words_to_events(const xm_evt3* d) {
  if (!d) return 12;
  return d->format == 2 || d->format == EVT_FMT_DAT ? 1 : d->format == EVT_FMT_21 ? 32 : 12;
}

// the activity filter's state as a packet sees it: its set of cells and control words.  The packets that take part -- the
// non-empty ones -- take the two sets strictly in turns (IngestLaunch::act_toggle, advanced by ingest_process; an empty push between
// two packets must not make them share a set: the second one's first pass runs beside the first one's counting launch)
ActDev ingest_act_set(const xm_ingest* g, int set) {
  ActDev a = g->fx.act_base;
  if (a.last_ts && (set & 1)) {
    a.cells += (size_t)a.cam_w * (size_t)a.cam_h * ACT_NB;
    a.ctl += 4;
  }
  return a;
}

// the three ingest launches of one (sub-)packet.  With the activity filter on and the NEXT packet already on its way to the device
// (la.next_job: a replay, or a camera that is ahead of the GPU), that packet's first pass (k_act_first) rides on this packet's
// k_ing_count launch (k_ing_count_act: the other set of cells) instead of being a link of its own in the chain of the stream.
void ingest_launch3(xm_ingest* g, const IngestPush& pp, u32 bound) {
  const IngestFixed& fx = g->fx;
  IngestLaunch& la = g->la;
  const unsigned nb = (bound + ING_EPB - 1) / ING_EPB;
  if (nb) {
    const IngestJob* nx = la.next_job;
    bool fused = false;
    if (nx && fx.act_base.last_ts && fx.opt_act_fuse) {
      const bool words = nx->kind == JobKind::words;
      const size_t n2 = words ? std::min<size_t>((size_t)fx.max_packet, nx->n * (size_t)ingest_words_to_events(nx->dec)) : nx->n;
      const unsigned nb2 = (unsigned)((n2 + ING_THREADS - 1) / ING_THREADS);
      if (n2 && hipStreamWaitEvent(fx.stream, fx.copied_ev[nx->k], 0) == hipSuccess) {
        hipLaunchKernelGGL(k_ing_count_act, dim3(nb + nb2), dim3(ING_THREADS), 0, fx.stream, la.dev, pp, (u32)nb, ingest_act_set(g, la.act_toggle /* the set the next packet will take: ingest_process has advanced it for this one */),
                           (const uint4*)fx.d_pkt[nx->k], words ? (const u32*)(fx.d_pkt_n + nx->k) : (const u32*)nullptr, (u32)n2,
                           fx.cfg.use_polarity ? 1 : 0);
        la.act_fused_push = pp.push_no + 1;
        la.act_fused_count += 1;
        fused = true;
      }
    }
    if (!fused) hipLaunchKernelGGL(k_ing_count, dim3(nb), dim3(ING_THREADS), 0, fx.stream, la.dev, pp);
    hipLaunchKernelGGL(k_ing_append, dim3(nb), dim3(ING_THREADS), 0, fx.stream, la.dev, pp);
  }
  hipLaunchKernelGGL(k_ing_segment, dim3(1), dim3(ING_THREADS), 0, fx.stream, la.dev, pp);
}

// everything behind the packet's arrival in d_pkt[j.k]: filters, append, segmentation (the activity filter is evaluated on the
// device for every kind of packet).  n events; for a packet decoded on the device the event count lives at n_dev (device memory)
// and n is the room of its slot
int ingest_process(xm_ingest* g, const IngestJob& j, size_t n, const u32* n_dev = nullptr) {
  const IngestFixed& fx = g->fx;
  IngestLaunch& la = g->la;
  hipStream_t s = fx.stream;
  // the ingest stream stays at most `ahead` packets in front of the verdicts handled here
  int rc = XM_OK;
  while (la.issued + 1 - la.next_verdict > (uint64_t)fx.ahead)
    if ((rc = ingest_handle_verdicts(g, la.next_verdict))) return rc;
  const uint64_t push_no = la.issued + 1;
  const int vi = (int)(push_no % ING_VRING);
  // The entry's previous user (packet push_no - ING_VRING) may have cut a frame, whose K2 and publishing launches read the
  // descriptor and the frame info out of the entry -- the last of them on the out stream, behind the frame's copies.  The ingest
  // stream waits only for that frame's K1, so the entry is handed to k_ing_segment again only once the frame's sequence number
  // is out (a read of pinned memory: by now it is, except with > ING_VRING packets between a cut and a stalled out side).
  if (const uint64_t fe = la.entry_frame[vi]) {
    const IngestStatus* stp = fx.h_status + (fe - 1) % (uint64_t)fx.ring;
    unsigned spins = 0;
    while (__atomic_load_n(&stp->seq, __ATOMIC_ACQUIRE) < fe) {
      if (g->out.err.code()) return ingest_out_error(g);
      __builtin_ia32_pause();
      if ((++spins & 0xfff) == 0) (void)hipStreamQuery(fx.out_stream);
    }
    la.entry_frame[vi] = 0;
  }
  la.push_t[vi] = j.t_push;
  la.push_filter[vi] = (unsigned char)(la.filter | (la.intended ? 8 : 0));
  la.push_surface[vi] = (unsigned char)(la.surf_select ? la.surf_select | (la.surf_dtype << 2) : 0);
  la.push_cloud[vi] = (unsigned char)(la.cloud_on ? 1 : 0);
  la.push_record[vi] = (unsigned char)(la.record_on ? 1 | (la.record_vectors ? 2 : 0) : 0);
  la.dev.desc = fx.d_descs + vi;
  la.dev.info = fx.d_infos + vi;
  la.dev.verdict = fx.d_verdicts + vi;
  IngestPush p{};
  p.flags = (fx.cfg.use_polarity ? ING_F_POLARITY : 0u) | ING_F_SEGMENT;
  p.push_no = push_no;
  p.src = fx.d_pkt[j.k];
  p.n = (u32)n;
  p.n_dev = n_dev;
  // activity filter: the packet's first pass (the per-(bucket, pixel) cells, one event per thread; xmaps_ingest.hpp) -- unless it
  // went out with the packet before (ingest_launch3) -- then the flags themselves are computed by k_ing_count as it counts.
  // Nothing is decided here: a chunk decoded on the device is treated like records.
  const int act_set = la.act_toggle;  // (the packet's set of cells: k_ing_count reads them, k_ing_append empties them, k_ing_segment resets its flags)
  if (n) la.act_toggle ^= 1;          // (an empty packet launches k_ing_segment only: it takes no turn)
  la.dev.act = ingest_act_set(g, act_set);
  if (la.dev.act.last_ts && n && la.act_fused_push != push_no)  // (fused: it went out with the packet before, ingest_launch3)
    hipLaunchKernelGGL(k_act_first, dim3((unsigned)((n + ING_THREADS - 1) / ING_THREADS)), dim3(ING_THREADS), 0, s, la.dev.act,
                       (const uint4*)fx.d_pkt[j.k], n_dev, (u32)n, fx.cfg.use_polarity ? 1 : 0);
  ingest_launch3(g, p, (u32)n);
  HIP_TRY(hipGetLastError());
  la.issued = push_no;
  // the frame (if this or an earlier packet cut one) as soon as its verdict is in: at once when nothing else is waiting
  return ingest_handle_verdicts(g, 0);
}

// one packet of records, the copy side: H2D on the copy stream (beside the previous packets' kernels) + the event behind it
int ingest_copy_records(xm_ingest* g, const IngestJob& j) {
  if (j.n) {
    HIP_TRY(hipMemcpyAsync(g->fx.d_pkt[j.k], j.host, j.n * 16, hipMemcpyHostToDevice, g->fx.copy_stream));
    HIP_TRY(hipEventRecord(g->fx.copied_ev[j.k], g->fx.copy_stream));
  }
  return XM_OK;
}

// ... the launch side: everything else (j.arrived: the copy side has done its part already)
int ingest_issue_records(xm_ingest* g, const IngestJob& j) {
  g->la.out_serial_now = false;
  int rc = j.arrived ? XM_OK : ingest_copy_records(g, j);
  if (rc) return rc;
  if (j.n) HIP_TRY(hipStreamWaitEvent(g->fx.stream, g->fx.copied_ev[j.k], 0));
  return ingest_process(g, j, j.n);
}

// one chunk of words, the copy side: H2D + the three decode launches on the decoder's stream + the event behind them
int ingest_copy_evt3(xm_ingest* g, const IngestJob& j) {
  xm_evt3* d = j.dec;
  if (j.n) {
    int rc = evt3_enqueue(d, j.host, j.n, j.pinned, g->fx.d_pkt[j.k], (size_t)g->fx.max_packet, d->stream, g->fx.d_pkt_n + j.k);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(g->fx.copied_ev[j.k], d->stream));
    d->cur ^= 1;
  }
  return XM_OK;
}

// ... the launch side: everything behind it, nothing waited for: the ingest's kernels read the chunk's event count on the device
int ingest_issue_evt3(xm_ingest* g, const IngestJob& j) {
  g->la.out_serial_now = !g->fx.opt_evt3_out_stream;  // (see IngestLaunch::out_serial_now)
  int rc = j.arrived ? XM_OK : ingest_copy_evt3(g, j);
  if (rc) return rc;
  if (!j.n) return ingest_process(g, j, 0);
  HIP_TRY(hipStreamWaitEvent(g->fx.stream, g->fx.copied_ev[j.k], 0));
  const size_t bound = std::min<size_t>((size_t)g->fx.max_packet, j.n * (size_t)ingest_words_to_events(j.dec));
  return ingest_process(g, j, bound, g->fx.d_pkt_n + j.k);
}

// every verdict in, every frame's kernels launched and run
int ingest_finish(xm_ingest* g) {
  int rc = ingest_handle_verdicts(g, g->la.issued);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(g->fx.copy_stream));
  HIP_TRY(hipStreamSynchronize(g->fx.stream));
  HIP_TRY(hipStreamSynchronize(g->fx.frame_stream));
  if ((rc = ingest_out_wait(g, g->la.frames_issued))) return rc;  // (every frame issued so far has its out-stream work enqueued)
  HIP_TRY(hipStreamSynchronize(g->fx.out_stream));
  return XM_OK;
}

int ingest_run_job(xm_ingest* g, const IngestJob& j) {
  switch (j.kind) {
    case JobKind::records: return ingest_issue_records(g, j);
    case JobKind::words: return ingest_issue_evt3(g, j);
    case JobKind::on_device: return ingest_process(g, j, j.n);
    case JobKind::flush: return ingest_finish(g);
    case JobKind::set_filter:
      g->la.filter = j.filter;
      g->la.intended = j.intended;
      break;
    case JobKind::set_surface:
      g->la.surf_select = j.surf_select;
      g->la.surf_dtype = j.surf_dtype;
      break;
    case JobKind::set_cloud:
      g->la.cloud_on = j.cloud_on;
      break;
    case JobKind::set_record:
      g->la.record_on = j.record_on;
      g->la.record_vectors = j.record_vectors;
      break;
    case JobKind::stop:
    case JobKind::count_only: break;
  }
  return XM_OK;
}

// ---- the threads ------------------------------------------------------------------------------------------------------------

void ingest_thread_main(xm_ingest* g) {
  (void)hipSetDevice(g->fx.h->cfg.device);
  IngestLaunch& la = g->la;
  // Nothing to launch: verdicts first -- a frame's kernels go out the moment its packet's verdict arrives (a live camera's
  // packets are milliseconds apart: the frame must not wait for the next one) -- then spin a little, then sleep.  Never
  // asleep with a verdict outstanding (it is at most a few ten microseconds away).
  const auto idle = [g, &la](unsigned long long i) {
    if (la.next_verdict > la.issued) return true;
    g->sh.err.note(ingest_handle_verdicts(g, 0), g_err);
    if (g->sh.err.code(std::memory_order_relaxed)) la.next_verdict = la.issued + 1;  // (do not spin on a failed stream)
    if ((i & 0x3ff) == 0x3ff) (void)hipStreamQuery(g->fx.stream);  // (a query makes the runtime hand over what it may still hold back)
    return false;
  };
  for (;;) {
    const IngestJob j = g->sh.launch_q.take(20000, idle);
    if (j.kind != JobKind::stop) {
      const double cj = ingest_now();
      // the job queued behind this one, if it is a packet whose copy / decoding the copy side has issued already
      la.next_job = nullptr;
      if (carries_packet(j.kind)) {
        const IngestJob* c = g->sh.launch_q.next();
        if (c && copy_side_has_work(c->kind) && c->arrived && c->n) la.next_job = c;
      }
      g->sh.err.note(ingest_run_job(g, j), g_err);
      la.next_job = nullptr;
      la.t_jobs_s += ingest_now() - cj;
    }
    g->sh.launch_q.finish();
    if (j.kind == JobKind::stop) return;
  }
}

// Copy side (round 5): a second thread IN FRONT of the launch thread issues what brings a packet to the device -- the H2D copy
// of records, or the H2D + the three decode launches of a RAW chunk, and the event behind them -- and forwards every job, in
// order, to the launch thread, which then issues one stream-wait and the ingest kernels.  With the activity filter the launch
// thread's 7 runtime calls per packet were what bounded the stream (profiles/r05_ingest.md); now 2-4 of them run beside the rest.
// "XM_INGEST_NO_COPY_THREAD": the launch thread does both (A/B).
void ingest_copy_thread_main(xm_ingest* g) {
  (void)hipSetDevice(g->fx.h->cfg.device);
  for (;;) {
    IngestJob j = g->sh.copy_q.take(20000);
    if (copy_side_has_work(j.kind) && !g->sh.err.code(std::memory_order_relaxed)) {
      const int rc = j.kind == JobKind::records ? ingest_copy_records(g, j) : ingest_copy_evt3(g, j);
      if (rc != XM_OK) {
        g->sh.err.note(rc, g_err);
        j.kind = JobKind::count_only;  // (nothing arrived)
      }
      j.arrived = true;
    }
    g->sh.launch_q.post(j);
    if (j.kind == JobKind::stop) return;
  }
}

// ---- the caller's door ------------------------------------------------------------------------------------------------------

// The copy thread's queue when there is one (every job passes through it and is forwarded IN ORDER, so a job's number is the same
// in both queues and the launch queue's count of finished jobs counts them alike), else the launch thread's.
unsigned long long ingest_post(xm_ingest* g, const IngestJob& j) {
  return (g->fx.copy_threaded ? g->sh.copy_q : g->sh.launch_q).post(j);
}

// jobs handed in so far (the caller's count)
unsigned long long ingest_posted(const xm_ingest* g) {
  return (g->fx.copy_threaded ? g->sh.copy_q : g->sh.launch_q).posted();
}

int ingest_take_error(xm_ingest* g) {
  std::string text;
  const int e = g->sh.err.take(&text);
  return e ? fail(e, "%s (reported by the ingest's launch thread)", text.c_str()) : XM_OK;
}

// hand a job to the launch thread (or run it here); wait: until it has run
int ingest_submit(xm_ingest* g, const IngestJob& j, bool wait) {
  if (!g->fx.threaded) return ingest_run_job(g, j);
  const unsigned long long n = ingest_post(g, j);
  if (wait) {
    g->sh.launch_q.wait_done(n);
    return ingest_take_error(g);
  }
  return XM_OK;
}

// The staging entry's previous packet has been consumed once that packet's verdict has been handled (k_ing_segment runs behind
// the kernels that read the packet): no API call, no event.
int ingest_wait_entry(xm_ingest* g, int k) {
  const uint64_t need = g->ca.pkt_push[k];
  if (!need || g->sh.handled.load(std::memory_order_acquire) >= need) return XM_OK;
  if (!g->fx.threaded) return ingest_handle_verdicts(g, need);
  const double c0 = ingest_now();
  g->ca.stage_waits += 1;
  while (g->sh.handled.load(std::memory_order_acquire) < need && !g->sh.err.code(std::memory_order_relaxed)) __builtin_ia32_pause();
  g->ca.push_wait_s += ingest_now() - c0;
  return ingest_take_error(g);
}

// The bookkeeping of one accepted push, whatever it carries: the staging entry j.k is taken, the push gets its number and its
// entry time c0 (when the call entered), the job goes to the launch side; the call's time into the statistics.
int ingest_accept_push(xm_ingest* g, IngestJob& j, double c0, bool wait) {
  IngestCaller& ca = g->ca;
  ca.pkt_next = (j.k + 1) % ING_STAGE;
  ca.posted += 1;
  ca.pkt_push[j.k] = ca.posted;
  j.push_no = ca.posted;
  j.t_push = c0;
  const int rc = ingest_submit(g, j, wait);
  ca.push_host_s += ingest_now() - c0;
  ca.push_calls += 1;
  return rc;
}

}  // namespace
