// xm_workers.hpp -- slot rotation, launch workers, a frame from the API thread or posted to a worker (run_frame, post_frame), the
// verified-shortcut verdict and redo (resolve_prev), the single-frame entry (process_common)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

Slot& pick_slot(xm_handle* h) {
  h->last_slot = h->next_slot;
  h->next_slot = (h->next_slot + 1) % (int)h->slots.size();
  return h->slots[h->last_slot];
}

// ---- worker threads --------------------------------------------------------------------------------------------------
void worker_main(xm_handle* h, Worker* w) {
  (void)hipSetDevice(h->cfg.device);
  for (;;) {
    const Job j = w->q.take(20000);
    if (j.kind == Job::STOP) {
      w->q.finish();
      return;
    }
    w->err.note(enqueue_frame(h, h->slots[j.slot], j.ev, j.depth, j.bgr, nullptr, j.allow_sorted), g_err);  // (this thread's text)
    w->q.finish();
  }
}

// wait until the workers have issued everything posted so far (the GPU may still be running it); reports a failed job
int drain_workers(xm_handle* h, int only = -1) {
  int rc = XM_OK;
  for (size_t i = 0; i < h->workers.size(); ++i) {
    if (only >= 0 && (int)i != only) continue;
    Worker* w = h->workers[i].get();
    w->q.wait_done(w->q.posted());
    std::string text;
    if (rc == XM_OK)
      if (const int e = w->err.take(&text)) rc = fail(e, "%s (reported by the launch worker of stream %zu)", text.c_str(), i);
  }
  return rc;
}

// device set + launch workers idle: the entry of every call that uses the slots' streams itself
#define XM_ENTER(h)                          \
  do {                                       \
    HIP_TRY(hipSetDevice((h)->cfg.device));  \
    int rc_enter_ = drain_workers(h);        \
    if (rc_enter_) return rc_enter_;         \
    if (!(h)->pending.empty() && (rc_enter_ = flush_pending(h))) return rc_enter_;  \
  } while (0)

// One frame on the slot's own stream from the API thread: its launches, the API's tag, and -- a host-memory call -- the copies of
// the outputs to where the caller wants them.  redo_frame: the same frame again on the general path (its shortcut did not hold).
int run_frame(xm_handle* h, Slot& s, const EventsView& ev, float* depth, uint8_t* bgr, float* host_depth, uint8_t* host_bgr,
              const Event* prof = nullptr, bool allow_sorted = true) {
  if (int rc = enqueue_frame(h, s, ev, depth, bgr, prof, allow_sorted)) return rc;
  s.last.api_tag = s.last.host_tag;
  const size_t px = (size_t)h->plan().dims.out_w * h->plan().dims.out_h;
  if (host_depth) HIP_TRY(hipMemcpyAsync(host_depth, depth, px * 4, hipMemcpyDeviceToHost, s.stream));
  if (host_bgr) HIP_TRY(hipMemcpyAsync(host_bgr, bgr, px * 3, hipMemcpyDeviceToHost, s.stream));
  return XM_OK;
}
int redo_frame(xm_handle* h, Slot& s, const EventsView& ev, float* depth, uint8_t* bgr, float* host_depth, uint8_t* host_bgr) {
  return run_frame(h, s, ev, depth, bgr, host_depth, host_bgr, nullptr, false);
}

// the frame's launches are the job of the slot's worker: the API counts its tag at once (with the wrap enqueue_frame will make)
void post_frame(xm_handle* h, Slot& s, const EventsView& ev, float* depth, uint8_t* bgr, bool allow_sorted) {
  const Job j{Job::FRAME, (int)(&s - h->slots.data()), ev, depth, bgr, allow_sorted};
  s.last.api_tag = s.last.api_tag >= KEY_MAX_TAG ? 1 : s.last.api_tag + 1;
  h->workers[s.worker]->q.post(j);
}

// XM_FLAG_TRY_SORTED: did the (t[0], t[n-1]) shortcut hold for the slot's last asynchronous frame?  The kernels answer in
// pinned host memory (no API call when the frame has finished, which it has when a slot comes round again); a frame that
// failed is redone here on the general path, into the same output buffers, before anything else happens on the slot.
#ifndef XM_POLL_FIRST_US
#define XM_POLL_FIRST_US 30
#define XM_POLL_NEXT_US 100
#endif
int resolve_prev(xm_handle* h, Slot& s, bool* redone = nullptr) {
  if (!s.prev.valid) return XM_OK;
  s.prev.valid = false;
  const u32 tag = s.prev.tag;
  // launch workers: the frame may be posted but not launched yet -- an empty stream also answers hipSuccess to the query
  // below, which would read as "shortcut held".  Wait until the worker has issued everything posted so far.
  if (s.worker >= 0) {
    const int rcw = drain_workers(h, s.worker);
    if (rcw) return rcw;
  }
  // still in flight?  Wait for K2's start marker by polling the pinned word: a blocking stream synchronisation costs a
  // ~200 us wake-up, per frame, whenever the host runs ahead of the GPU (few slots); the marker is a few us away.
  if (__atomic_load_n(&s.h_flags[1], __ATOMIC_ACQUIRE) != tag) {
    auto t_next = std::chrono::steady_clock::now() + std::chrono::microseconds(XM_POLL_FIRST_US);
    unsigned spins = 0;
    while (__atomic_load_n(&s.h_flags[1], __ATOMIC_ACQUIRE) != tag) {
      __builtin_ia32_pause();
      if ((++spins & 0x3f) == 0 && std::chrono::steady_clock::now() > t_next) {
        // not there after 30 us: make sure the runtime has really handed the slot's commands to the GPU (a query flushes
        // anything it still holds back -- seen: a frame that sat for 20 ms until something synchronised), and stop polling
        // once the stream itself reports completion
        hipError_t q = hipStreamQuery(s.prev.stream ? s.prev.stream : s.stream);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) HIP_TRY(q);
        t_next = std::chrono::steady_clock::now() + std::chrono::microseconds(XM_POLL_NEXT_US);
      }
    }
  }
  if (!s.prev.check || __atomic_load_n(&s.h_flags[0], __ATOMIC_ACQUIRE) != tag) return XM_OK;
  h->sorted_fallbacks += 1;
  if (s.last.key32) key32_note(h, true);
  const Slot::Prev& pv = s.prev;
  if (s.worker >= 0 && !pv.host_depth && !pv.host_bgr) {  // the redo goes the way the frame went
    post_frame(h, s, pv.ev, pv.depth, pv.bgr, false);
  } else {
    int rc = s.worker >= 0 ? drain_workers(h, s.worker) : XM_OK;
    if (rc) return rc;
    if ((rc = redo_frame(h, s, pv.ev, pv.depth, pv.bgr, pv.host_depth, pv.host_bgr))) return rc;
  }
  if (redone) *redone = true;
  return XM_OK;
}

int process_common(xm_handle* h, EventsView ev, int mem, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats,
                   bool profile) {
  if (!h) return fail(XM_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(h->cfg.device));
  int rc = check_events(ev);
  if (rc) return rc;
  const size_t px = (size_t)h->plan().dims.out_w * h->plan().dims.out_h;
  if (h->ab_max >= 2 && mem == XM_MEM_DEVICE && !profile && !h->capturing && !stats) {  // adaptive batching (see xm_handle::pending)
    // One group = one kernel template (AoS or SoA, the time stamps' type, polarity column or not), chosen from its first frame:
    // a frame of another layout closes the group that is pending and opens its own.
    if (!h->pending.empty()) {
      const EventsView& e0 = h->pending.front().ev;
      if ((e0.aos != nullptr) != (ev.aos != nullptr) || e0.t_dtype != ev.t_dtype || e0.use_p != ev.use_p || (e0.p != nullptr) != (ev.p != nullptr))
        if ((rc = flush_pending(h))) return rc;
    }
    h->pending.push_back(xm_handle::Deferred{ev, depth_out, bgr_out});
    int in_flight = 0;
    for (hipEvent_t e : h->ab_inflight)
      if (e && hipEventQuery(e) == hipErrorNotReady) in_flight += 1;
    (void)hipGetLastError();
    // Launch at once when the GPU is idle (the 60 Hz live pipe: latency), else hold the frame back until a full group is pending: a
    // caller that produces frames faster than the GPU takes them gets groups of ab_max from the second launch on.  ("in_flight < 3"
    // until the end of round 3: every group's submission costs the CALLING thread ~30 us, so a run that started with small groups
    // could stay there -- the thread had no time left to get ahead of the GPU: 37 instead of 140 Gev/s on some boxes.)
    if ((int)h->pending.size() >= h->ab_max || in_flight == 0) return flush_pending(h);
    return XM_OK;
  }
  if (!h->pending.empty() && (rc = flush_pending(h))) return rc;  // (a synchronous / host-memory call behind deferred frames)
  Slot& s = profile ? h->slots[0] : pick_slot(h);
  if (profile) h->last_slot = 0;
  if ((rc = resolve_prev(h, s))) return rc;
  if (s.worker >= 0 && mem == XM_MEM_DEVICE && !profile && !h->capturing) {
    // asynchronous device-pointer frame: the launches are the worker's job
    post_frame(h, s, ev, depth_out, bgr_out, true);
    if (s.h_flags) s.prev.set(ev, depth_out, bgr_out, nullptr, nullptr, s.last.api_tag, s.stream, h->plan().modes.try_sorted && sorted_path(h->plan(), path_now(h), ev));
    return XM_OK;
  }
  if (s.worker >= 0 && (rc = drain_workers(h, s.worker))) return rc;  // this call uses the slot's stream itself
  float* d_depth = depth_out;
  uint8_t* d_bgr = bgr_out;
  const bool host_in = mem == XM_MEM_HOST || mem == XM_MEM_HOST_PINNED;
  if (host_in) {
    const size_t n = ev.n;
    if (ev.aos) {
      if ((rc = stage_in(s.ev_aos, ev.aos, n * 16, s.stream))) return rc;
      ev.aos = s.ev_aos.p;
    } else {
      if ((rc = stage_in(s.ev_x, ev.x, n * 2, s.stream))) return rc;
      if ((rc = stage_in(s.ev_y, ev.y, n * 2, s.stream))) return rc;
      if ((rc = stage_in(s.ev_t, ev.t, n * t_size(ev.t_dtype), s.stream))) return rc;
      ev.x = (const uint16_t*)s.ev_x.p;
      ev.y = (const uint16_t*)s.ev_y.p;
      ev.t = s.ev_t.p;
      if (ev.p) {
        if ((rc = stage_in(s.ev_p, ev.p, n * 2, s.stream))) return rc;
        ev.p = (const int16_t*)s.ev_p.p;
      }
    }
    if (depth_out) {
      if ((rc = s.out_depth.reserve(px * 4))) return rc;
      d_depth = (float*)s.out_depth.p;
    }
    if (bgr_out) {
      if ((rc = s.out_bgr.reserve(px * 3))) return rc;
      d_bgr = (uint8_t*)s.out_bgr.p;
    }
  } else if (mem != XM_MEM_DEVICE) {
    return fail(XM_ERR_INVALID, "mem must be XM_MEM_HOST, XM_MEM_HOST_PINNED or XM_MEM_DEVICE");
  }
  float* const host_depth = host_in ? depth_out : nullptr;  // (d_depth / d_bgr are NULL where these are)
  uint8_t* const host_bgr = host_in ? bgr_out : nullptr;
  if ((rc = run_frame(h, s, ev, d_depth, d_bgr, host_depth, host_bgr, profile ? h->prof_ev : nullptr))) return rc;
  if (s.h_flags && !h->capturing && mem != XM_MEM_HOST && !profile) {
    // asynchronous call: the slot is not reused before this frame has reached K2 (keeps the host from running queues
    // deep ahead of the GPU, which made the frame rate uneven), and a try-sorted verdict is read then
    // (ev: device pointers -- the slot's staging buffers for pinned host input)
    s.prev.set(ev, d_depth, d_bgr, host_depth, host_bgr, s.last.host_tag, s.stream, h->plan().modes.try_sorted && s.last.sorted);
  }
  if (mem == XM_MEM_HOST || profile) {
    if ((rc = s.order.host_wait())) return rc;
    xm_frame_stats st;
    if ((rc = fetch_stats(h, s, ev.aos ? XM_T_INT64 : ev.t_dtype, &st))) return rc;
    if (profile) {
      const int first = s.last.sorted && !s.last.cols ? 1 : 0;  // K0 is not launched on the time-sorted path (column tiles: K0b in its place)
#ifdef XM_ABLATE  // experiment builds may skip kernels (XM_SKIP_MASK): their events were never recorded
      for (int i = first; i < 3; ++i)
        if (hipEventElapsedTime(&st.gpu_ms[i], h->prof_ev[2 * i], h->prof_ev[2 * i + 1]) != hipSuccess) (void)hipGetLastError();
      if (hipEventElapsedTime(&st.gpu_ms[3], h->prof_ev[2 * first], h->prof_ev[5]) != hipSuccess) (void)hipGetLastError();
#else
      for (int i = first; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&st.gpu_ms[i], h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
      HIP_TRY(hipEventElapsedTime(&st.gpu_ms[3], h->prof_ev[2 * first], h->prof_ev[5]));  // start of first .. end of K2
#endif
    }
    if (st.n_unsorted && s.last.sorted) {
      // the time-sorted declaration did not hold for this frame: redo it on the general path (K0 -> K1 -> K2)
      h->sorted_fallbacks += 1;
      if (s.last.key32) key32_note(h, true);
      if ((rc = redo_frame(h, s, ev, d_depth, d_bgr, host_depth, host_bgr))) return rc;
      if ((rc = s.order.host_wait())) return rc;
      const uint64_t flagged = st.n_unsorted;
      if ((rc = fetch_stats(h, s, ev.aos ? XM_T_INT64 : ev.t_dtype, &st))) return rc;
      st.n_unsorted = flagged;
      HIP_TRY(hipMemsetAsync(&s.st->unsorted_sticky, 0, sizeof(u32), s.stream));  // handled here, not an xm_sync error
      HIP_TRY(hipStreamSynchronize(s.stream));
    }
    if (stats) *stats = st;
    if (st.n_index_errors)
      return fail(XM_ERR_INDEX, "%llu event(s) indexed outside a table/frame (IndexError in the reference)",
                  (unsigned long long)st.n_index_errors);
  }
  return XM_OK;
}

int ensure_stage_frame(xm_handle* h) {
  const size_t need = std::max((size_t)h->tb.rect_w * h->tb.rect_h, (size_t)h->tb.cam_w * h->tb.cam_h);
  if (h->stage_frame && h->stage_cells >= need) return XM_OK;
  HIP_TRY(h->stage_frame.alloc(need));
  h->stage_cells = need;
  return XM_OK;
}

int rearm_aux(xm_handle* h, hipStream_t stream, u64* frame, u64 cells) {
  hipLaunchKernelGGL(k_reset_slot, dim3(cells ? 1024 : 1), dim3(BLOCK), 0, stream, h->aux_st, frame, cells,
                     (unsigned char*)nullptr);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

template <typename T>
void host_minmax_out(const SlotState& hs, void* out) {
  u64 a = MM_INIT_MIN, b = MM_INIT_MAX;
  for (int i = 0; i < MM_SLOTS; ++i) {
    a = hs.mm[0][i][0] < a ? hs.mm[0][i][0] : a;
    b = hs.mm[0][i][1] > b ? hs.mm[0][i][1] : b;
  }
  T* o = (T*)out;
  if (a == MM_INIT_MIN && b == MM_INIT_MAX) {  // empty shard: neutral elements of min / max
    o[0] = std::numeric_limits<T>::has_infinity ? std::numeric_limits<T>::infinity() : std::numeric_limits<T>::max();
    o[1] = std::numeric_limits<T>::has_infinity ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::lowest();
    return;
  }
  o[0] = TimeCodec<T>::dec(a);
  o[1] = TimeCodec<T>::dec(b);
}

}  // namespace
