// xm_api_graph.hpp -- C-ABI: batches captured into a hipGraph (BASELINE config 5).  A capture runs nothing: the slots' last-frame
// records are copied out and back around it; a replay is ordered behind the slots' last work by SlotOrder::before_all
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

extern "C" {

// ---- hipGraph batch ------------------------------------------------------------------------------------
// Default: the frames are captured as GROUPS of multi-frame launches (3 kernel nodes per group instead of 3 per frame).
// With n_slots >= n_frames the whole batch is one group; otherwise groups of n_slots / 2 frames alternate between two
// capture streams (each half of the slots always on the same branch), so that one group's tail overlaps the next one's head.
// XM_GRAPH_PER_FRAME=1 (experiments) keeps the round-1 form: three nodes per frame, frames forked over the slots' streams.
static int graph_capture_batched(xm_handle* h, xm_graph* g, const BatchViews& v) {
  const int ns = (int)h->slots.size(), n_frames = (int)v.evs.size();
  const bool two = ns >= 2 && n_frames > ns;
  const int G = two ? ns / 2 : std::min(ns, n_frames);
  g->h_descs.resize(2 * (size_t)n_frames);  // [n_frames] the frames, [n_frames] the same frames on their slots' 64-bit key frames
  for (auto& d : g->h_descs) d = FrameDesc{};  // (valid = 0: unused entries are skipped by every kernel)
  HIP_TRY(g->d_descs.alloc(2 * (size_t)n_frames));
  hipStream_t origin = h->gstreams[0], second = two ? h->gstreams[1] : nullptr;
  int rc = XM_OK;
  hipError_t e = hipSuccess;
  h->capturing = true;
  e = hipStreamBeginCapture(origin, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    h->capturing = false;
    return fail(XM_ERR_HIP, "hipStreamBeginCapture: %s", hipGetErrorString(e));
  }
  do {
    if (two) {
      if ((e = hipEventRecord(h->fork_ev, origin)) != hipSuccess) break;
      if ((e = hipStreamWaitEvent(second, h->fork_ev, 0)) != hipSuccess) break;
    }
    int gi = 0;
    for (int f0 = 0; f0 < n_frames && rc == XM_OK; f0 += G, ++gi) {
      const int nf = std::min(G, n_frames - f0);
      const int half = two ? gi & 1 : 0;
      std::vector<int> idx(nf);
      for (int j = 0; j < nf; ++j) {
        idx[j] = half * G + j;
        h->slots[idx[j]].last.host_tag = 0;  // tags advance on the device inside a graph; no reset mid-capture
        g->frames_on_slot[idx[j]] += 1;
      }
      rc = enqueue_batch(h, idx.data(), v.evs.data() + f0, v.dep.data() + f0, v.bg.data() + f0, nf, half ? second : origin,
                         g->h_descs.data() + f0, g->d_descs + f0, false, true, nullptr, nullptr,
                         g->h_descs.data() + n_frames + f0, g->d_descs + n_frames + f0);
    }
    if (two && rc == XM_OK) {
      if ((e = hipEventRecord(h->join_ev[1], second)) != hipSuccess) break;
      if ((e = hipStreamWaitEvent(origin, h->join_ev[1], 0)) != hipSuccess) break;
    }
  } while (0);
  hipError_t e2 = hipStreamEndCapture(origin, &g->graph);
  h->capturing = false;
  if (rc == XM_OK && (e != hipSuccess || e2 != hipSuccess))
    rc = fail(XM_ERR_HIP, "graph capture failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
  if (rc == XM_OK)  // the descriptors are static: one upload for the graph's lifetime
    HIP_TRY(hipMemcpy(g->d_descs, g->h_descs.data(), sizeof(FrameDesc) * 2 * n_frames, hipMemcpyHostToDevice));
  return rc;
}

int xm_graph_create(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                    const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out, xm_graph** out) {
  if (!h || !out || !offsets_host || n_frames <= 0) return fail(XM_ERR_INVALID, "bad argument");
  *out = nullptr;
  XM_ENTER(h);
  const int ns = (int)h->slots.size();
  if ((u64)n_frames / ns + 1 >= KEY_MAX_TAG) return fail(XM_ERR_INVALID, "too many frames per graph");
  BatchViews v;  // (offsets that decrease, frames too large: refused before anything is captured)
  if (int rc = batch_views(h->plan(), x, y, t, p, t_dtype, nullptr, offsets_host, n_frames, depth_out, bgr_out, v)) return rc;
  for (Slot& s : h->slots) HIP_TRY(hipStreamSynchronize(s.stream));
  for (Slot& s : h->slots) s.order.forget();  // idle: nothing to order the capture against
  Owned<xm_graph, xm_graph_destroy> g(new (std::nothrow) xm_graph());
  if (!g) return fail(XM_ERR_NOMEM, "out of host memory");
  g->h = h;
  g->n_frames = n_frames;
  g->frames_on_slot.assign(ns, 0);
  std::vector<Slot::Last> saved(ns);
  for (int i = 0; i < ns; ++i) saved[i] = h->slots[i].last;
  // Graphs are captured on (and launched from) default-priority streams of their own: launched from the slots'
  // high-priority streams the replay ran its branches one after the other (28 instead of 61 Gevents/s).
  if (h->gstreams.empty()) {
    std::vector<Stream> gs(std::max(ns, 2));
    for (Stream& s : gs) HIP_TRY(s.create(hipStreamNonBlocking));
    h->gstreams = std::move(gs);
  }
  int rc = graph_capture_batched(h, g.get(), v);
  for (int i = 0; i < ns; ++i) {  // capture only recorded launches: the slots are where they were
    h->slots[i].last = saved[i];
    h->slots[i].order.forget();
  }
  if (rc == XM_OK) {
    hipError_t e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) rc = fail(XM_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
  }
  if (rc != XM_OK) return rc;
  *out = g.release();
  return XM_OK;
}

int xm_graph_launch(xm_graph* g) {
  if (!g || !g->exec) return fail(XM_ERR_INVALID, "NULL graph");
  xm_handle* h = g->h;
  XM_ENTER(h);
  const int ns = (int)h->slots.size();
  hipStream_t origin = h->gstreams[0];
  if (h->plan().modes.try_sorted)
    for (Slot& s : h->slots) {  // settle pending try-sorted verdicts before the replay advances the slots' tags
      int rc = resolve_prev(h, s);
      if (rc) return rc;
    }
  // order the replay after whatever the slots did last -- per distinct stream, and only where something is pending (a
  // handle that only replays graphs pays one hipGraphLaunch + one hipEventRecord per replay, not 3 API calls per slot)
  const auto order_of = [](Slot& s) -> SlotOrder<HipOrderOps>& { return s.order; };
  if (int rc = SlotOrder<HipOrderOps>::before_all(h->slots.begin(), h->slots.end(), order_of, origin)) return rc;
  for (int i = 0; i < ns; ++i) {  // tag wrap per slot
    Slot& s = h->slots[i];
    if ((u64)s.last.host_tag + g->frames_on_slot[i] >= KEY_MAX_TAG) {
      hipLaunchKernelGGL(k_reset_slot, dim3(1024), dim3(BLOCK), 0, origin, s.st, s.key_frame, (u64)h->plan().dims.key_cells, s.dirty);
      HIP_TRY(hipGetLastError());
      s.last.host_tag = 0;
      s.last.api_tag = 0;
    }
  }
  HIP_TRY(hipGraphLaunch(g->exec, origin));
  // whatever a slot does next on its own stream waits for the replay (lazily, see enqueue_frame / enqueue_batch)
  hipEvent_t done = h->graph_ev[h->graph_ev_next++ % 8];
  HIP_TRY(hipEventRecord(done, origin));
  for (int i = 0; i < ns; ++i) {
    Slot& s = h->slots[i];
    s.last.host_tag += g->frames_on_slot[i];
    s.last.api_tag = s.last.host_tag;  // the worker path derives the next frame's tag from api_tag
    if (g->frames_on_slot[i]) s.order.note_group(done, origin);
  }
  return XM_OK;
}

void xm_graph_destroy(xm_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;  // (d_descs goes with it)
}

}  // extern "C"
