// xm_ingest_out.hpp -- device-side ingest (N2), the out side: a cut frame's copies to the pinned result ring and its sequence
// number (the out thread, or the launch side for frames that leave in order), and the pool of result buffers that leave with a frame
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; state and threads: xm_ingest_state.hpp)
#pragma once

// Result buffers that LEAVE the ingest with a frame (xm_ingest_poll_owned) and come back when the consumer lets go of them
// (xm_frame_pool_release): the reference hands frame_callback a fresh array per frame (depth_reprojection_pipe.py:164-167,
// SURVEY 8(b) "Ownership"); copying a 6.2 MB frame out of the result ring for that costs more host time than the GPU needs for
// the frame, so the pinned buffer the DMA filled IS the fresh array and the ring slot gets another one.  The pool outlives its
// ingest while buffers are out (the last release deletes it).
struct xm_frame_pool {
  std::mutex mu;
  int device = 0;
  size_t bytes[2] = {0, 0};            // [0] depth (f32), [1] BGR
  std::vector<void*> free_bufs[2];
  size_t outstanding = 0;              // buffers in consumers' hands
  size_t allocated = 0, cap = 0;       // buffers made so far / at most (then the caller copies, as before)
  bool closed = false;                 // the ingest is gone: a released buffer is freed
};

namespace {

// The result ring's and the frame pool's pinned buffers (raw on purpose: a buffer leaves with a frame through xm_ingest_poll_owned
// and comes back through xm_frame_pool_release -- ownership crosses the C ABI; these two are the only places that make / free one)
hipError_t ring_buf_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
void ring_buf_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- one frame's out work -----------------------------------------------------------------------------------------------

// wait for the frame's K2, copy its outputs to the pinned result ring, the sequence number behind them.  Runs on the out thread
// (j on the out stream), or on the launch side (j.serial: on the frame stream; or there is no out thread)
int ingest_out_frame(xm_ingest* g, const OutJob& j) {
  const IngestFixed& fx = g->fx;
  xm_handle* h = fx.h;
  const bool out_thread = fx.out_threaded && !j.serial;  // which thread this is
  hipStream_t os = j.serial ? fx.frame_stream : fx.out_stream;
  // A copy enqueued behind one that is still running can block its caller for as long as that one runs -- inside the runtime,
  // with other threads' calls waiting behind it: the previous frame's copies are seen off first (a query loop, no blocking call).
  const bool host_seq = fx.host_seq && out_thread;
  if (out_thread && j.frame_no > 0 && !fx.opt_out_no_query && !host_seq) {
    const int po = (int)((j.frame_no - 1) % ING_NOUT);
    while (hipEventQuery(fx.out_ev[po]) == hipErrorNotReady)
      for (int k = 0; k < 64; ++k) __builtin_ia32_pause();
    (void)hipGetLastError();
  }
  const double t0 = ingest_now();
  HIP_TRY(hipStreamWaitEvent(os, fx.k2_ev[j.o], 0));
  const size_t px = (size_t)h->plan().dims.out_w * h->plan().dims.out_h;
  // In pieces of 4 MB: with one frame per packet (EVT 3.0 period chunks) whole 6 MB copies gave 620-870 Mev/s in an ingest's first
  // minutes and 1170-1210 later, pieces 1130 every time (tools/esl_evt3_probe.py); 1 MB pieces overflow a queue of the runtime
  // and stall for milliseconds (tools/ubench/dma_mix.cpp), so the option does not go below 2 MB.
  const size_t piece = fx.out_piece;
  const auto copy_out = [&](void* dst, const void* src, size_t bytes) -> int {
    for (size_t off = 0; off < bytes; off += piece)
      HIP_TRY(hipMemcpyAsync((char*)dst + off, (const char*)src + off, std::min(piece, bytes - off), hipMemcpyDeviceToHost, os));
    return XM_OK;
  };
  int rc;
  void *dst_bgr, *dst_depth;
  {
    std::lock_guard<std::mutex> lk(g->sh.res_mu);
    dst_bgr = g->sh.h_bgr[j.slot];
    dst_depth = g->sh.h_depth[j.slot];
    g->sh.slot_frame[j.slot] = j.frame_no + 1;
  }
  if (dst_bgr && (rc = copy_out(dst_bgr, fx.d_out_bgr[j.o], px * 3))) return rc;
  if (dst_depth && (rc = copy_out(dst_depth, fx.d_out_depth[j.o], px * 4))) return rc;
  if (!host_seq) {
    hipLaunchKernelGGL(k_ing_publish_seq, dim3(1), dim3(64), 0, os, fx.dev.st, j.desc, fx.h_status + j.slot, (u64)j.frame_no);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(fx.out_ev[j.o], os));
  // (nothing else is issued on this stream until the next frame: without a query the runtime kept the last copy and the sequence
  //  number in its batch until some other call of the process flushed it -- seen in the copy trace: the second piece of a frame
  //  starting 90 us after the first, together with the next packet's H2D copy)
  (void)hipStreamQuery(os);
  (out_thread ? g->out.t_out_s : g->la.t_out_s) += ingest_now() - t0;  // (one counter per thread, summed in the trace)
  if (host_seq) {
    // the copies have landed once their event has fired (a query loop: no blocking call of the runtime while the launch thread is
    // issuing): then the sequence number, the last thing the poller looks at (xm_ingest_poll reads it with acquire)
    for (hipError_t q; (q = hipEventQuery(fx.out_ev[j.o])) != hipSuccess;) {
      if (q != hipErrorNotReady) HIP_TRY(q);
      for (int k = 0; k < 32; ++k) __builtin_ia32_pause();
    }
    (void)hipGetLastError();
    // (live latency as the library sees it: the push call of the packet that completed the frame entered -> now)
    fx.h_status[j.slot].latency_us = j.t_push > 0.0 ? (float)((ingest_now() - j.t_push) * 1e6) : 0.0f;
    __atomic_store_n(&fx.h_status[j.slot].seq, (uint64_t)j.frame_no + 1, __ATOMIC_RELEASE);
  }
  return XM_OK;
}

void ingest_out_main(xm_ingest* g) {
  (void)hipSetDevice(g->fx.h->cfg.device);
  for (;;) {
    // A frame's copy should start the moment its K2 is on the stream (with one frame per packet the copies are what bounds the
    // pipe: a sleeping thread's wake-up would go straight into the frame period): spin for about a millisecond before sleeping.
    const OutJob j = g->out.q.take(40000);
    // (a frame the launch side took itself -- j.done -- is only counted; after an error nothing more is enqueued)
    if (!j.stop && !j.done && !g->out.err.code(std::memory_order_relaxed)) g->out.err.note(ingest_out_frame(g, j), g_err);
    g->out.q.finish();
    if (j.stop) return;
  }
}

// the out side's error, if it has one (it stays)
int ingest_out_error(xm_ingest* g) {
  std::string text;
  const int e = g->out.err.peek(&text);
  return e ? fail(e, "ingest, out side: %s", text.c_str()) : XM_OK;
}

// ---- the launch side's calls ------------------------------------------------------------------------------------------------

// frames below `upto` (= the out queue's jobs 1 .. upto) have their out work enqueued, or the out side has failed
int ingest_out_wait(xm_ingest* g, uint64_t upto) {
  if (g->fx.out_threaded) g->out.q.wait_done(upto, &g->out.err);  // (no out thread: a frame's out work is enqueued when it is issued)
  return ingest_out_error(g);
}

// a cut frame leaves: to the out thread; or at once, here, when it goes out in order on the frame stream or there is no out thread
int ingest_out_hand_over(xm_ingest* g, OutJob j) {
  if (!g->fx.out_threaded) return ingest_out_frame(g, j);
  if (j.serial) {
    // (the frames posted before the mode changed come first; the out thread then finishes this job without work, so that
    //  job number = frame number + 1 holds whichever side ran the frame)
    int rc = ingest_out_wait(g, j.frame_no);
    if (!rc) rc = ingest_out_frame(g, j);
    if (rc) return rc;
    j.done = true;
  }
  g->out.q.post(j);
  return XM_OK;
}

// ---- the frame pool (caller side) -------------------------------------------------------------------------------------------

// the ingest's pool, made by the first xm_ingest_poll_owned (NULL: out of host memory)
xm_frame_pool* pool_of(xm_ingest* g) {
  if (g->ca.pool) return g->ca.pool;
  xm_frame_pool* pl = new (std::nothrow) xm_frame_pool();
  if (!pl) return nullptr;
  pl->device = g->fx.h->cfg.device;
  const size_t px = (size_t)g->fx.h->plan().dims.out_w * g->fx.h->plan().dims.out_h;
  pl->bytes[0] = px * 4;
  pl->bytes[1] = px * 3;
  pl->cap = 1024;
  if (const char* e = dbg_opt("XM_INGEST_POOL_CAP")) pl->cap = (size_t)std::max(0, atoi(e));
  return g->ca.pool = pl;
}

// spare[b] for every kind of buffer (0 depth, 1 BGR) that want[b] names, from the pool's free ones or new: all of them or none (then the caller copies
// the frame out of the ring as xm_ingest_poll's callers do)
bool pool_take_spares(xm_ingest* g, const bool want[2], void* spare[2]) {
  xm_frame_pool* pl = pool_of(g);
  if (!pl) return false;
  std::lock_guard<std::mutex> lk(pl->mu);
  bool have = true;
  for (int b = 0; b < 2 && have; ++b) {
    if (!want[b]) continue;
    if (!pl->free_bufs[b].empty()) {
      spare[b] = pl->free_bufs[b].back();
      pl->free_bufs[b].pop_back();
    } else if (pl->allocated < pl->cap && hipSetDevice(pl->device) == hipSuccess && ring_buf_alloc(&spare[b], pl->bytes[b]) == hipSuccess) {
      pl->allocated += 1;
    } else {
      (void)hipGetLastError();
      spare[b] = nullptr;
      have = false;
    }
  }
  if (!have)  // (not both: what was taken goes back)
    for (int b = 0; b < 2; ++b)
      if (spare[b]) pl->free_bufs[b].push_back(spare[b]);
  return have;
}

// ... afterwards: the spares went into the ring slot and the slot's `n_out` buffers left with the frame (they are in the
// consumer's hands now), or (n_out = 0) the slot had been lapped and the spares come back
void pool_give_back(xm_frame_pool* pl, void* spare[2], int n_out) {
  std::lock_guard<std::mutex> lk(pl->mu);
  pl->outstanding += (size_t)n_out;
  for (int b = 0; b < 2 && !n_out; ++b)
    if (spare[b]) pl->free_bufs[b].push_back(spare[b]);
}

// the ingest goes: spare buffers now, buffers in consumers' hands when they come back (the last one takes the pool along)
void pool_close(xm_frame_pool* pl) {
  bool last;
  {
    std::lock_guard<std::mutex> lk(pl->mu);
    pl->closed = true;
    for (auto& v : pl->free_bufs) {
      for (void* p : v) ring_buf_free(p);
      v.clear();
    }
    last = pl->outstanding == 0;
  }
  if (last) delete pl;
}

}  // namespace

extern "C" {

void xm_frame_pool_release(xm_frame_pool* pl, void* buffer, int kind) {
  if (!pl || !buffer || kind < 0 || kind > 1) return;
  bool last = false, free_it = false;
  {
    std::lock_guard<std::mutex> lk(pl->mu);
    if (pl->outstanding) pl->outstanding -= 1;
    if (pl->closed) {
      free_it = true;
      last = pl->outstanding == 0;
    } else {
      pl->free_bufs[kind].push_back(buffer);
    }
  }
  if (free_it) ring_buf_free(buffer);
  if (last) delete pl;
}

int xm_frame_pool_stats(xm_frame_pool* pl, uint64_t* allocated, uint64_t* outstanding, uint64_t* spare) {
  if (!pl) return fail(XM_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(pl->mu);
  if (allocated) *allocated = pl->allocated;
  if (outstanding) *outstanding = pl->outstanding;
  if (spare) *spare = pl->free_bufs[0].size() + pl->free_bufs[1].size();
  return XM_OK;
}

}  // extern "C"
