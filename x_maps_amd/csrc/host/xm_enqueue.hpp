// xm_enqueue.hpp -- the tiles' launchers (K0b, column / owner-tile K1), what the path rules may know about the moment (path_now), what
// a slot records once a frame is enqueued, and the launches of ONE frame (enqueue_frame)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

// K0b: the tile boundaries + column thresholds of the frame(s), left behind the u16 frame (its shape: cols_bounds_shape,
// xm_plan.hpp).  flags: k_cols_bounds_batch's (a lone frame's kernel has none)
template <bool AOS, typename F>
void launch_cols_bounds(xm_handle* h, const F& fr, int W, int flags, hipStream_t stream) {
  const BoundsShape sh = cols_bounds_shape(h->plan(), W);
  DevTables tb = h->tb;
  if constexpr (!is_lone<F>) {
    if (sh.split) own_apply(h->plan().own[sh.own], h->own[sh.own], tb);  // (a group's owner-tile K0b takes its plan's tables, a lone frame's the plain ones)
  }
  auto go = [&](auto lanes_tag) {
    constexpr int G = decltype(lanes_tag)::value;
    if constexpr (is_lone<F>)
      XM_LAUNCH((k_cols_bounds<AOS, G>), dim3(sh.gx), dim3(256), 0, stream, fr.ev.x, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos,
                (u32)fr.ev.n, tb, W, static_cast<uint16_t*>(fr.frame), sh.split);
    else
      XM_LAUNCH((k_cols_bounds_batch<AOS, G>), dim3(sh.gx, fr.n), dim3(256), 0, stream, fr.descs, tb, W, flags, sh.split);
  };
  if (sh.lanes == 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
}

// K1 on the column tiles (xmaps_k1cols.hpp) or, where the rig's X-map is not injective, on the owner tiles (xmaps_k1own.hpp):
// grid = tiles (x frames), block from the mean frame (tiles_k1_shape, xm_plan.hpp).  flags: on top of the rig's own; lds_pad: extra
// dynamic LDS of a column-tile block (XM_COLS_LDS_PAD, experiments: fewer K1 blocks per CU, room for another kernel's -- the
// groups' launch only)
template <bool AOS, typename F>
int launch_tiles_k1(xm_handle* h, const F& fr, int W, int flags, size_t lds_pad, hipStream_t stream) {
  const RigPlan& pl = h->plan();
  const bool v16 = !AOS && vec16(fr);
  const TilesK1Shape sh = tiles_k1_shape(pl, fr.n_mean(), W, v16, flags, lds_pad);
  const dim3 grid(sh.gx, frames(fr)), block(sh.threads);
  if (sh.own >= 0) {
    DevTables tbo = h->tb;
    own_apply(pl.own[sh.own], h->own[sh.own], tbo);
    auto inst = [](auto vec_tag, auto ept_tag) {
      constexpr bool V = decltype(vec_tag)::value;
      constexpr int E = decltype(ept_tag)::value;
      if constexpr (is_lone<F>) return k_scatter_own<AOS, V, E>;
      else return k_scatter_own_batch<AOS, V, E>;
    };
    auto kern = sh.ept == 4 ? inst(std::false_type{}, std::integral_constant<int, 4>{})
                            : inst(std::false_type{}, std::integral_constant<int, COLS_EPT>{});
    if constexpr (!AOS) {
      if (v16) kern = inst(std::true_type{}, std::integral_constant<int, COLS_EPT>{});
    }
    int rc = h->ensure_lds(reinterpret_cast<const void*>(kern), sh.lds);
    if (rc) return rc;
    if constexpr (is_lone<F>)
      XM_LAUNCH(kern, grid, block, sh.lds, stream, fr.ev.x, fr.ev.y, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos, (u32)fr.ev.n, tbo,
                fr.st, static_cast<uint16_t*>(fr.frame), W, sh.halo, sh.flags);
    else
      XM_LAUNCH(kern, grid, block, sh.lds, stream, fr.descs, tbo, W, sh.halo, sh.flags);
    return XM_OK;
  }
  auto inst = [](auto vec_tag) {
    constexpr bool V = decltype(vec_tag)::value;
    if constexpr (is_lone<F>) return k_scatter_cols<AOS, V>;
    else return k_scatter_cols_batch<AOS, V>;
  };
  auto kern = inst(std::false_type{});
  if constexpr (!AOS) {
    if (v16) kern = inst(std::true_type{});
  }
  int rc = h->ensure_lds(reinterpret_cast<const void*>(kern), sh.lds);
  if (rc) return rc;
  if constexpr (is_lone<F>)
    XM_LAUNCH(kern, grid, block, sh.lds, stream, fr.ev.x, fr.ev.y, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos, (u32)fr.ev.n, h->tb,
              fr.st, static_cast<uint16_t*>(fr.frame), W, pl.k1.w_x, pl.cols.xr_min, sh.flags);
  else
    XM_LAUNCH(kern, grid, block, sh.lds, stream, fr.descs, h->tb, W, pl.k1.w_x, pl.cols.xr_min, sh.flags);
  return XM_OK;
}

int check_events(const EventsView& ev) {
  if (ev.n >= XM_KEY_MAX_EVENTS) return fail(XM_ERR_TOO_MANY, "frame of %zu events exceeds 2^%d", ev.n, XM_KEY_IDX_BITS);
  if (ev.n == 0) return XM_OK;
  if (ev.aos) {
    if (!aligned(ev.aos, 16)) return fail(XM_ERR_INVALID, "EventCD buffer must be 16-byte aligned");
    return XM_OK;
  }
  if (!ev.x || !ev.y || !ev.t) return fail(XM_ERR_INVALID, "x, y, t must be non-NULL when n > 0");
  if (ev.t_dtype != XM_T_INT64 && ev.t_dtype != XM_T_FLOAT32 && ev.t_dtype != XM_T_FLOAT64)
    return fail(XM_ERR_INVALID, "unknown t_dtype %d", ev.t_dtype);
  if (!aligned(ev.t, t_size(ev.t_dtype)) || !aligned(ev.x, 2) || !aligned(ev.y, 2) || (ev.p && !aligned(ev.p, 2)))
    return fail(XM_ERR_INVALID, "event columns must be naturally aligned");
  return XM_OK;
}

// ---- which path a frame or a group takes: frame_path (xm_plan.hpp), from the plan and this ------------------------------------
PathNow path_now(const xm_handle* h) { return PathNow{h->capturing, h->key32_pause.load(std::memory_order_relaxed) > 0}; }

// keep the slot's compact frame unambiguous for a frame with tag `tag` (4-bit tags repeat every 15 frames)
int key32_prepare(const RigPlan& pl, Slot& s, u32 tag, hipStream_t stream) {
  if (!pl.dims.projector) return XM_OK;  // camera view: no tag -- the frame kernel zeroes every pixel it reads
  if (tag - s.key32_valid_from >= 15u || tag < s.key32_valid_from) {
    HIP_TRY(hipMemsetAsync(s.key32, 0, pl.dims.key_cells * sizeof(u32), stream));
    s.key32_valid_from = tag;
  }
  return XM_OK;
}

void key32_note(xm_handle* h, bool failed) {
  if (failed) {
    if (h->key32_score.fetch_add(8, std::memory_order_relaxed) + 8 >= 24) {  // the stream keeps producing events outside the
      h->key32_pause.store(512, std::memory_order_relaxed);                  // LDS time window (sparse / bursty frames)
      h->key32_score.store(0, std::memory_order_relaxed);
    }
  } else {
    int v = h->key32_score.load(std::memory_order_relaxed);
    while (v > 0 && !h->key32_score.compare_exchange_weak(v, v - 1, std::memory_order_relaxed)) {
    }
  }
}

// the compact paths' pause (key32_note) counts down by the frames enqueued: one per lone frame, a group's all at once
void key32_pause_tick(xm_handle* h, int frames) {
  int v = h->key32_pause.load(std::memory_order_relaxed);
  while (v > 0 && !h->key32_pause.compare_exchange_weak(v, std::max(0, v - frames), std::memory_order_relaxed)) {
  }
}

// frame `ev` was enqueued on slot s along path p: what the slot's redo and statistics read later, and the path counters.  A group
// hands its tags to the API at once (api_tag); a lone frame's caller does that itself.
void note_enqueued(xm_handle* h, Slot& s, const EventsView& ev, const FramePath& p, bool group) {
  Slot::Last& l = s.last;
  l.host_tag += 1;
  if (group) l.api_tag = l.host_tag;
  l.n = ev.n;
  l.sorted = p.sorted || p.cols_w != 0;  // (no K0 either on a captured group's column tiles; a lone frame's are sorted)
  l.key32 = p.key32 || p.cols_w;
  l.cols = p.cols_w != 0;
  l.t_dtype = ev.aos ? XM_T_INT64 : ev.t_dtype;
  h->path_counts[p.counter()].fetch_add(1, std::memory_order_relaxed);
  if (p.key32 || p.cols_w) key32_note(h, false);
}

// enqueue K0 -> K1 -> K2 for one frame on a slot.  All pointers are device pointers.
int enqueue_frame(xm_handle* h, Slot& s, const EventsView& ev, float* depth, uint8_t* bgr, const Event* prof,
                  bool allow_sorted = true, hipStream_t stream_override = nullptr) {
  const FramePath p = frame_path(h->plan(), path_now(h), &ev, 1, allow_sorted);
  key32_pause_tick(h, 1);
  hipStream_t stream = stream_override ? stream_override : s.stream;
  // the slot's previous frame may have run inside a group or a replay on another stream (the own stream's eager work: a group's
  // stream was ordered behind it by enqueue_batch, the own stream needs no order with itself)
  if (int rc = s.order.before_group_only(stream)) return rc;
  if (s.last.host_tag >= KEY_MAX_TAG) {  // tag field about to wrap: clear the frame once per 2^19 frames
    int rc = reset_slot(h->plan(), s, stream);
    if (rc) return rc;
  }
#ifdef XM_ABLATE
  static const int skip = dbg_opt("XM_SKIP_MASK") ? atoi(dbg_opt("XM_SKIP_MASK")) : 0;  // experiments: 1=K0 2=K1 4=K2
#else
  constexpr int skip = 0;
#endif
  const ProfSlots ps{prof};
  void* out = p.cols_w ? (void*)s.frame16 : p.key32 ? (void*)s.key32 : (void*)s.key_frame;
  const LoneFrame fr{ev, s.st, 0, out, s.dirty, depth, bgr};
  ps.at(0);
  int rc = with_event_types(ev, [&](auto ty) -> int {
    using E = decltype(ty);
    if (!(skip & 1) && !p.sorted) launch_k0<typename E::T, E::AOS, E::HAS_P>(fr, stream);
    if constexpr (tile_types<E>) {
      if (!(skip & 1) && p.cols_w) launch_cols_bounds<E::AOS>(h, fr, p.cols_w, 0, stream);  // K0b takes K0's place (and its profile events)
    }
    if (p.key32) {
      const int rc_k = key32_prepare(h->plan(), s, s.last.host_tag + 1, stream);
      if (rc_k) return rc_k;
    }
    ps.at(1);
    if (skip & 2) return XM_OK;
    if constexpr (tile_types<E>) {
      if (p.cols_w) return launch_tiles_k1<E::AOS>(h, fr, p.cols_w, 0, 0, stream);
    }
    return launch_k1<typename E::T, E::AOS, E::HAS_P>(h, fr, tiled_path(h->plan(), ev.n), p.key32, p.sorted, stream);
  });
  if (rc) return rc;
  ps.at(2);
  if (!(skip & 4)) launch_frame_kernel(h, fr, p.kmode(), stream);
  HIP_TRY(hipGetLastError());
  note_enqueued(h, s, ev, p, false);
  if (!stream_override) s.order.note_eager();
  return XM_OK;
}

}  // namespace
