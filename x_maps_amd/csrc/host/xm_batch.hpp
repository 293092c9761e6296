// xm_batch.hpp -- multi-frame launches: a batch's offsets as one view per frame (batch_views), one K0 / K1 / K2 launch each for a
// group of frames (enqueue_batch), frame statistics, host staging
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

// ---- multi-frame launches -------------------------------------------------------------------------------------------
// One K0 / K1 / K2 launch each for a whole group of frames (grid = frames x tiles).  Frame f of the group runs on slot
// slots[f] (its own key frame + state), all on ONE stream.  A single frame's launches leave the chip half empty while
// they ramp up and drain (245 K1 blocks for 256 CUs, each a ~10 us dependent chain); a group's launch keeps every CU fed.
template <typename T, bool AOS, bool HAS_P>
int launch_group(xm_handle* h, const FrameGroup& g, const FramePath& p, hipStream_t stream, const Event* prof,
                 const FrameDesc* d_descs_redo) {
  const ProfSlots ps{prof};
  if constexpr (std::is_same<T, long long>::value && !HAS_P) {
    if (p.cols_w) {  // column / owner tiles: K1 grid = (tiles, frames), K2 on the plain u16 frames
      ps.at(0);
      launch_cols_bounds<AOS>(h, g, p.cols_w, 0, stream);
      ps.at(1);
      int rc = launch_tiles_k1<AOS>(h, g, p.cols_w, p.dev_redo ? COLS_F_DEVICE_REDO : 0, (size_t)h->plan().cols.lds_pad, stream);
      if (rc) return rc;
      ps.at(2);
      if (!p.dev_redo) {
        launch_frame_kernel(h, g, KM_COLS, stream);
        HIP_TRY(hipGetLastError());
        return XM_OK;
      }
      // Captured batch (hipGraph): no host at hand to redo a frame whose tiles objected, so the graph carries both paths and the
      // kernels decide per frame on the device (frame_attempt_failed): K2 on the u16 frame only where the attempt held, then --
      // for the frames where it did not, and for those only: every other block returns at once -- the counters cleared and
      // K0 -> K1 -> K2 on the 64-bit key frame (d_descs_redo = the same frames with key_frame = the slots' 64-bit frames).
      launch_k2_batch<2, 2>(h, stream, g.descs, g.n);
      g_prof = ProfCtx{};
      XM_LAUNCH(k_redo_prepare_batch, dim3(g.n), dim3(64), 0, stream, d_descs_redo);
      const FrameGroup redo{d_descs_redo, g.n, g.events_max, g.events_mean, g.all_vec16};
      launch_k0<T, AOS, false, 1>(redo, stream, 64);
      if ((rc = launch_k1<T, AOS, false, 1>(h, redo, true, false, false, stream))) return rc;
      launch_k2_batch<0, 1>(h, stream, d_descs_redo, g.n);
      HIP_TRY(hipGetLastError());
      return XM_OK;
    }
  }
  ps.at(0);
  if (!p.sorted) launch_k0<T, AOS, HAS_P>(g, stream);
  ps.at(1);
  if (int rc = launch_k1<T, AOS, HAS_P>(h, g, !p.direct, p.key32, p.sorted, stream)) return rc;
  ps.at(2);
  launch_frame_kernel(h, g, p.kmode(), stream);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// A batch as the API takes it -- columns (or EventCD records, 16 bytes each, every event used) cut into frames by offsets_host[0 ..
// n_frames], outputs packed frame after frame -- as one EventsView and one pair of output pointers per frame, each checked
struct BatchViews {
  std::vector<EventsView> evs;
  std::vector<float*> dep;
  std::vector<uint8_t*> bg;
};
int batch_views(const RigPlan& pl, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype, const void* aos,
                const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out, BatchViews& v) {
  const size_t px = (size_t)pl.dims.out_w * pl.dims.out_h, tsz = t_size(t_dtype);
  v.evs.assign(n_frames, EventsView{});
  v.dep.assign(n_frames, nullptr);
  v.bg.assign(n_frames, nullptr);
  for (int f = 0; f < n_frames; ++f) {
    const u64 a = offsets_host[f], b = offsets_host[f + 1];
    if (b < a) return fail(XM_ERR_INVALID, "offsets must be non-decreasing");
    EventsView& ev = v.evs[f];
    if (aos) {
      ev.aos = (const char*)aos + a * 16;
      ev.t_dtype = XM_T_INT64;
    } else {
      ev.x = x + a; ev.y = y + a; ev.t = (const char*)t + a * tsz; ev.p = p ? p + a : nullptr;
      ev.t_dtype = t_dtype; ev.use_p = p != nullptr;
    }
    ev.n = (size_t)(b - a);
    if (int rc = check_events(ev)) return rc;
    if (depth_out) v.dep[f] = depth_out + f * px;
    if (bgr_out) v.bg[f] = bgr_out + f * px * 3;
  }
  return XM_OK;
}

// Enqueue one group: frame f = evs[f] on slot slot_idx[f], outputs depth[f] / bgr[f] (device pointers), everything on `stream`.
// d_descs / h_descs: where the group's descriptors live (the caller owns their lifetime).  `upload`: copy them now
// (eager) -- false when the caller uploads once (graph capture).
int enqueue_batch(xm_handle* h, const int* slot_idx, const EventsView* evs, float* const* depth, uint8_t* const* bgr,
                  int n_frames, hipStream_t stream, FrameDesc* h_descs, FrameDesc* d_descs, bool upload, bool allow_sorted,
                  const Event* prof = nullptr, int* kinds = nullptr, FrameDesc* h_descs_redo = nullptr,
                  FrameDesc* d_descs_redo = nullptr) {
  const FramePath p = frame_path(h->plan(), path_now(h), evs, n_frames, allow_sorted, true, d_descs_redo != nullptr);
  for (int f = 0; f < n_frames; ++f)  // order the group after whatever its slots did last on other streams
    if (int rc = h->slots[slot_idx[f]].order.before(stream, h->capturing)) return rc;
  if (p.per_frame) {  // untiled K2: frame by frame, still on the group's stream
    for (int f = 0; f < n_frames; ++f) {
      Slot& s = h->slots[slot_idx[f]];
      int rc = enqueue_frame(h, s, evs[f], depth[f], bgr[f], nullptr, allow_sorted, stream);
      if (rc) return rc;
      s.last.api_tag = s.last.host_tag;
    }
    return XM_OK;
  }
  key32_pause_tick(h, n_frames);
  for (int f = 0; f < n_frames; ++f) {
    Slot& s = h->slots[slot_idx[f]];
    if (s.last.host_tag >= KEY_MAX_TAG && !h->capturing) {
      int rc = reset_slot(h->plan(), s, stream);
      if (rc) return rc;
    }
    if (p.key32) {
      int rc = key32_prepare(h->plan(), s, s.last.host_tag + 1, stream);
      if (rc) return rc;
    }
    FrameDesc& d = h_descs[f];
    const EventsView& ev = evs[f];
    d.x = ev.x; d.y = ev.y; d.t = ev.t; d.p = ev.use_p ? ev.p : nullptr; d.aos = (const uint4*)ev.aos;
    d.n = ev.n; d.key_frame = p.cols_w ? reinterpret_cast<u64*>(s.frame16.get()) : p.key32 ? reinterpret_cast<u64*>(s.key32.get()) : s.key_frame.get();
    d.st = s.st; d.depth = depth[f];
    d.bgr = bgr[f]; d.valid = 1; d.pad = 0;
    if (p.dev_redo) {  // the same frame on the slot's 64-bit key frame
      h_descs_redo[f] = d;
      h_descs_redo[f].key_frame = s.key_frame;
    }
  }
  if (upload) HIP_TRY(hipMemcpyAsync(d_descs, h_descs, sizeof(FrameDesc) * n_frames, hipMemcpyHostToDevice, stream));
  const FrameGroup g{d_descs, n_frames, p.n_max, p.n_mean, p.vec16};
  const int rc = with_event_types(evs[0], [&](auto ty) -> int {
    using E = decltype(ty);  // (the profile events attach to the groups of int64 time stamps without a polarity column only)
    return launch_group<typename E::T, E::AOS, E::HAS_P>(h, g, p, stream, tile_types<E> ? prof : nullptr, d_descs_redo);
  });
  if (rc) return rc;
  if (kinds) {  // which launches the group consisted of: {K0 general / K0b bounds / none, K1 variant}
    kinds[0] = p.cols_w ? 2 : p.sorted ? 0 : 1;  // (K0 runs whenever the frames are not on a sorted path)
    kinds[1] = p.kmode();
  }
  for (int f = 0; f < n_frames; ++f) note_enqueued(h, h->slots[slot_idx[f]], evs[f], p, true);
  return XM_OK;
}

template <typename T>
void decode_minmax(const SlotState& hs, u32 parity, double& lo, double& hi, bool& any) {
  u64 a = MM_INIT_MIN, b = MM_INIT_MAX;
  for (int i = 0; i < MM_SLOTS; ++i) {
    a = hs.mm[parity][i][0] < a ? hs.mm[parity][i][0] : a;
    b = hs.mm[parity][i][1] > b ? hs.mm[parity][i][1] : b;
  }
  any = !(a == MM_INIT_MIN && b == MM_INIT_MAX);
  lo = any ? (double)TimeCodec<T>::dec(a) : 0.0;
  hi = any ? (double)TimeCodec<T>::dec(b) : 0.0;
}

// read the slot's state back and fill stats for its most recent frame (stream must be idle)
int fetch_stats(xm_handle* h, Slot& s, int t_dtype, xm_frame_stats* out) {
  SlotState hs;
  HIP_TRY(hipMemcpy(&hs, s.st, sizeof hs, hipMemcpyDeviceToHost));
  const u32 parity = s.last.host_tag & 1;
  memset(out, 0, sizeof *out);
  out->n_events = s.last.n;
  for (int i = 0; i < CNT_SLOTS; ++i) {
    out->n_used += hs.cnt[parity][i][CNT_USED];
    out->n_inliers += hs.cnt[parity][i][CNT_INLIER];
    out->n_index_errors += hs.cnt[parity][i][CNT_OOB];
    out->n_unsorted += hs.cnt[parity][i][CNT_UNSORTED];
  }
  if (s.last.sorted) out->n_used = s.last.n;  // no polarity column on the time-sorted path; K0 (which counts) did not run
  bool any;
  if (t_dtype == XM_T_FLOAT32) decode_minmax<float>(hs, parity, out->t_min, out->t_max, any);
  else if (t_dtype == XM_T_FLOAT64) decode_minmax<double>(hs, parity, out->t_min, out->t_max, any);
  else decode_minmax<long long>(hs, parity, out->t_min, out->t_max, any);
  (void)h;
  return XM_OK;
}

// (`head` bytes of room in front of the copy, `tail` behind it: the data stand at b.p + head)
int stage_in(DevBuf& b, const void* host, size_t bytes, hipStream_t st, size_t head = 0, size_t tail = 0) {
  const size_t room = head + bytes + tail;
  int rc = b.reserve(room ? room : 16);
  if (rc) return rc;
  if (bytes) HIP_TRY(hipMemcpyAsync((char*)b.p + head, host, bytes, hipMemcpyHostToDevice, st));
  return XM_OK;
}


}  // namespace
