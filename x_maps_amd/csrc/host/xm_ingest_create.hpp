// xm_ingest_create.hpp -- device-side ingest (N2): the stages of xm_ingest_create, in the order they run (as xm_create.hpp does for
// the handle): options -> streams and events -> device rings and activity state -> result ring with warm-up copies -> threads
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; state and threads: xm_ingest_state.hpp)
#pragma once

namespace {

// Each stage returns an error code; xm_ingest_create's Owned<> cleans up a half-built ingest.

// sizes, the reference's defaults, the debug options (read once, here)
int ingest_read_options(IngestFixed& fx, xm_handle* h, const xm_ingest_config* cfg) {
  fx.h = h;
  fx.cfg = *cfg;
  const u64 want_cap = cfg->capacity_events ? cfg->capacity_events : (1u << 21);
  fx.capacity = 1;
  while (fx.capacity < want_cap) fx.capacity <<= 1;  // the ring is indexed by (absolute stream index) & (capacity - 1)
  fx.max_packet = cfg->max_packet_events ? cfg->max_packet_events : (1u << 19);
  if (fx.capacity >= 0x7fffffffull || fx.max_packet * 2 > fx.capacity || fx.max_packet > (u64)ING_MAX_BLOCKS * ING_EPB)
    return fail(XM_ERR_INVALID, "capacity must be < 2^31 events and at least twice max_packet_events (itself at most %llu)",
                (unsigned long long)ING_MAX_BLOCKS * ING_EPB);
  // packets the ingest stream may run ahead of the frame kernels: each costs one packet's worth of ring (the room rule)
  fx.ahead = fx.capacity >= 8 * fx.max_packet ? (int)std::min<u64>(3, fx.capacity / fx.max_packet / 4) : 0;
  fx.period = 1e6 / (double)cfg->projector_fps;                       // trigger_finder.py: 1e6 / self.projector_fps (float)
  fx.act_thresh = cfg->activity_thresh_us > 0 ? cfg->activity_thresh_us : (long long)(1e6 / cfg->projector_fps);  // pipe:65-68
  if (fx.cfg.pause_thresh_us <= 0) fx.cfg.pause_thresh_us = 40;       // trigger_finder.py:98
  if (fx.cfg.min_events_per_frame <= 0) fx.cfg.min_events_per_frame = 1000;  // trigger_finder.py:8
  // the cut is evs[prev + 2 : next - 2] (trigger_finder.py:172): fewer than 4 events between two pauses would be an empty frame, on
  // which the reference's t.min() raises
  if (fx.cfg.min_events_per_frame < 4) return fail(XM_ERR_INVALID, "min_events_per_frame must be >= 4 (the frame is evs[prev + 2 : next - 2])");
  fx.ring = cfg->result_ring > 0 ? cfg->result_ring : 8;
  if (const char* e = dbg_opt("XM_INGEST_CLEAR_EVERY")) fx.clear_every = (uint64_t)std::max(1, atoi(e));
  if (const char* e = dbg_opt("XM_INGEST_OUT_PIECE")) fx.out_piece = std::max<size_t>(2u << 20, (size_t)atoll(e));
  if (const char* e = dbg_opt("XM_INGEST_OUT_SERIAL")) fx.out_on_frame_stream = e[0] == '1';
  fx.opt_out_no_query = dbg_opt("XM_INGEST_OUT_NO_QUERY") != nullptr;
  if (const char* e = dbg_opt("XM_INGEST_HOST_SEQ")) fx.host_seq = e[0] != '0';
  fx.opt_evt3_out_stream = dbg_opt("XM_INGEST_EVT3_OUT_STREAM") != nullptr;
  fx.opt_trace = dbg_opt("XM_INGEST_TRACE") != nullptr;
  if (const char* e = dbg_opt("XM_INGEST_ACT_FUSE")) fx.opt_act_fuse = e[0] != '0';
  return XM_OK;
}

int ingest_create_streams(IngestFixed& fx, const void* who) {
  int lo = 0, hi = 0;
  HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
  // "XM_INGEST_PRIOS": four letters h / n / l = the priority pools of the ingest, frame, copy and out stream (A/B; default below).
  // The streams come from the process's set for this device (ingest_stream_set) when nobody else has it.
  const char* pr = dbg_opt("XM_INGEST_PRIOS");
  if (!pr || strlen(pr) != 4) pr = "hhnh";
  const auto prio_of = [&](char c) { return c == 'l' ? lo : c == 'n' ? (lo + hi) / 2 : hi; };
  hipStream_t* set = dbg_opt("XM_INGEST_OWN_STREAMS") ? nullptr : ingest_stream_set(fx.h->cfg.device, who);
  for (int i = 0; i < 4; ++i) {
    if (!set) HIP_TRY(fx.streams[i].create_with_priority(hipStreamNonBlocking, prio_of(pr[i])));
    else {
      if (!set[i]) HIP_TRY(hipStreamCreateWithPriority(&set[i], hipStreamNonBlocking, prio_of(pr[i])));  // (the set's: it stays)
      fx.streams[i].borrow(set[i]);
    }
  }
  fx.stream = fx.streams[0];        // ingest kernels
  fx.frame_stream = fx.streams[1];  // the cut frames' kernels
  fx.copy_stream = fx.streams[2];   // H2D of a packet beside the kernels of the previous one
  fx.out_stream = fx.streams[3];    // the result frames' copies + sequence numbers
  for (Event& e : fx.copied_ev) HIP_TRY(e.create());
  for (Event& e : fx.k1_ev) HIP_TRY(e.create());
  for (Event& e : fx.k2_ev) HIP_TRY(e.create());
  for (Event& e : fx.out_ev) HIP_TRY(e.create());
  return XM_OK;
}

// the event ring, the pause ring, the per-packet rings, the slot, the activity filter's state, the staging entries
int ingest_create_device_rings(IngestFixed& fx) {
  xm_handle* h = fx.h;
  IngestDev& d = fx.dev;
  d.cap = fx.capacity;
  d.room = fx.max_packet * (u64)(1 + fx.ahead);
  d.mirror = fx.capacity / 2;  // frames of up to half the ring are contiguous wherever they start
  d.pcap = fx.capacity * 2;    // (a pause per live event + the stale head the trigger finder has not skipped yet)
  HIP_TRY(fx.d_buf.alloc(d.cap + d.mirror));
  HIP_TRY(fx.d_pring.alloc(d.pcap));
  HIP_TRY(fx.d_blk.alloc(ING_MAX_BLOCKS));
  d.buf = fx.d_buf.get();
  d.pring = fx.d_pring.get();
  d.blk = fx.d_blk.get();
  if (fx.cfg.activity_filter) {
    if (int rc = act_alloc(fx.act_mem, &d.act, h->tb.cam_w, h->tb.cam_h, fx.act_thresh, (size_t)fx.max_packet, 2)) return rc;
    d.act.self_counts = (fx.cfg.flags & XM_INGEST_ACT_SELF) ? 1 : 0;
    fx.act_base = d.act;
  }
  d.cam_w = h->tb.cam_w;
  d.cam_h = h->tb.cam_h;
  d.pause_thresh = fx.cfg.pause_thresh_us;
  d.period = fx.period;
  d.min_events = (u32)fx.cfg.min_events_per_frame;
  d.ring = (u32)fx.ring;
  HIP_TRY(fx.d_st.alloc(1));
  d.st = fx.d_st.get();
  HIP_TRY(hipMemset(d.st, 0, sizeof(IngestState)));
  HIP_TRY(fx.d_descs.alloc(ING_VRING));
  HIP_TRY(hipMemset(fx.d_descs, 0, sizeof(FrameDesc) * ING_VRING));
  HIP_TRY(fx.d_infos.alloc(ING_VRING));
  HIP_TRY(hipMemset(fx.d_infos, 0, sizeof(IngFrameInfo) * ING_VRING));
  HIP_TRY(fx.h_verdicts.alloc(ING_VRING, hipHostMallocMapped));
  memset(fx.h_verdicts, 0, sizeof(IngVerdict) * ING_VRING);
  HIP_TRY(hipHostGetDevicePointer((void**)&fx.d_verdicts, fx.h_verdicts, 0));
  HIP_TRY(fx.d_key_frame.alloc(h->plan().dims.key_cells));
  HIP_TRY(fx.d_slot.alloc(1));
  d.key_frame = fx.d_key_frame.get();
  d.slot = fx.d_slot.get();
  HIP_TRY(hipMemset(d.slot, 0, sizeof(SlotState)));
  // (a memset of device memory may return before it has run and the ingest's streams do not wait for the default stream:
  //  k_reset_slot initialises the extrema slots inside these bytes -- seen once as a first frame with a wrong time normalisation)
  HIP_TRY(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_reset_slot, dim3(1024), dim3(BLOCK), 0, fx.frame_stream, d.slot, d.key_frame, (u64)h->plan().dims.key_cells, (unsigned char*)nullptr);
  HIP_TRY(hipGetLastError());
  // (the staging entries' pinned twins, IngestCaller::h_pkt[], are allocated by the first PAGEABLE push: callers that push pinned
  //  packets or RAW words never pay for 16 x max_packet x 16 bytes of page-locked memory)
  for (DevMem<uint4>& p : fx.d_pkt) HIP_TRY(p.alloc(fx.max_packet));
  HIP_TRY(fx.d_pkt_n.alloc(ING_STAGE));
  return XM_OK;
}

// the pinned result ring, the device-side output frames, one warm-up copy into every ring entry
int ingest_create_result_ring(IngestFixed& fx, IngestShared& sh) {
  const xm_ingest_config& cfg = fx.cfg;
  const size_t px = (size_t)fx.h->plan().dims.out_w * fx.h->plan().dims.out_h;
  HIP_TRY(fx.h_status.alloc(fx.ring, hipHostMallocMapped));
  memset(fx.h_status, 0, sizeof(IngestStatus) * fx.ring);
  sh.h_depth.assign(fx.ring, nullptr);
  sh.h_bgr.assign(fx.ring, nullptr);
  sh.slot_frame.assign(fx.ring, 0);
  for (int i = 0; i < fx.ring; ++i) {
    if (cfg.want_depth) HIP_TRY(ring_buf_alloc((void**)&sh.h_depth[i], px * 4));
    if (cfg.want_bgr) HIP_TRY(ring_buf_alloc((void**)&sh.h_bgr[i], px * 3));
  }
  float* out_depth[ING_NOUT];
  uint8_t* out_bgr[ING_NOUT];
  for (int i = 0; i < ING_NOUT; ++i) {
    if (cfg.want_depth) HIP_TRY(fx.d_out_depth[i].alloc(px));
    if (cfg.want_bgr) HIP_TRY(fx.d_out_bgr[i].alloc(px * 3));
    out_depth[i] = fx.d_out_depth[i], out_bgr[i] = fx.d_out_bgr[i];
  }
  HIP_TRY(fx.d_depth_ring.alloc(ING_NOUT));
  HIP_TRY(fx.d_bgr_ring.alloc(ING_NOUT));
  HIP_TRY(hipMemcpy(fx.d_depth_ring, out_depth, sizeof out_depth, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(fx.d_bgr_ring, out_bgr, sizeof out_bgr, hipMemcpyHostToDevice));
  fx.dev.nout = ING_NOUT;
  // (the first DMA into a pinned buffer is several times slower than the later ones -- seen as 0.2 ms per frame for the first
  //  round through the ring: every entry takes one copy now)
  for (int i = 0; i < fx.ring; ++i) {
    if (cfg.want_depth) HIP_TRY(hipMemcpyAsync(sh.h_depth[i], fx.d_out_depth[i % ING_NOUT], px * 4, hipMemcpyDeviceToHost, fx.out_stream));
    if (cfg.want_bgr) HIP_TRY(hipMemcpyAsync(sh.h_bgr[i], fx.d_out_bgr[i % ING_NOUT], px * 3, hipMemcpyDeviceToHost, fx.out_stream));
  }
  HIP_TRY(hipStreamSynchronize(fx.out_stream));
  fx.dev.depth_ring = fx.d_depth_ring;
  fx.dev.bgr_ring = fx.d_bgr_ring;
  HIP_TRY(hipDeviceSynchronize());  // (the memsets above ran on the default stream, which the ingest's non-blocking streams do not wait for)
  return XM_OK;
}

// last: from here on IngestFixed is read-only
void ingest_start_threads(xm_ingest* g) {
  IngestFixed& fx = g->fx;
  g->la.dev = fx.dev;
  if (fx.cfg.flags & XM_INGEST_NO_LAUNCH_THREAD) return;
  fx.threaded = true;
  fx.copy_threaded = !dbg_opt("XM_INGEST_NO_COPY_THREAD");
  fx.out_threaded = !fx.out_on_frame_stream && !dbg_opt("XM_INGEST_OUT_INLINE");
  g->th = std::thread(ingest_thread_main, g);
  if (fx.copy_threaded) g->copy_th = std::thread(ingest_copy_thread_main, g);
  if (fx.out_threaded) g->out_th = std::thread(ingest_out_main, g);
}

}  // namespace
