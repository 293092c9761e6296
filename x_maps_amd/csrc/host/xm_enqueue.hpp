// xm_enqueue.hpp -- the tiles' launchers (K0b, column / owner-tile K1), which path a frame or a group takes (frame_path), what
// a slot records once a frame is enqueued, and the launches of ONE frame (enqueue_frame)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

// time columns per tile for frames of n events: about cols_target events per tile, within the LDS budget; 0 = not this path
int cols_width(const xm_handle* h, u64 n) {
  if (h->cols_ok && h->own_mode) {  // owner tiles: the widths the ownership tables are built for; not for nearly empty frames
    // the default plan (wide tiles) while a tile's own + halo columns fit ONE event pass of a block (8 events x 512 threads: past
    // that a tile looks its events up again for every row pass); denser frames take the second plan's narrow tiles
    const double per_col = (double)n / (double)h->tb.xmap_w;
    int pick = 0;  // (the mean tile: measured on the ESL-like frames at 94 % of a block's events, the fuller tiles' second pass included)
    while (pick + 1 < xm_handle::OWN_PLANS && h->own[pick + 1].ok &&
           per_col * (h->own[pick].w + h->own[pick].halo) > (double)(COLS_EPT * COLS_MAX_THREADS))
      pick += 1;
    const xm_handle::OwnSet& os = h->own[pick];
    const u64 tiles = grid_for(h->tb.xmap_w, os.w);
    return n >= tiles * 128 && n < (1ull << 28) ? os.w : 0;
  }
  if (!h->cols_ok || h->cols_w_max < 1 || h->tb.xmap_w < 1 || n == 0 || n >= (1ull << 28)) return 0;
  const double per_col = (double)n / (double)h->tb.xmap_w;
  int W = (int)((double)h->cols_target / per_col);
  W = std::max(1, std::min(W, h->cols_w_max));
  if (per_col * W < 1024.0) return 0;  // sparse frames: the band copies and the slot scan would dominate (direct kernel instead)
  return W;
}

// owner tiles: events per thread -- eight; four (twice the waves at half the registers for the same tile: xmaps_k1own.hpp) measured
// the same within the noise (profiles/r05_own_tiles.md) and is kept as an experiment switch ("XM_OWN_EPT" = 4; not for 16-byte SoA loads)
// the plan whose tiles are W columns wide (cols_width picked it)
const xm_handle::OwnSet& own_set(const xm_handle* h, int W) {
  for (int i = 1; i < xm_handle::OWN_PLANS; ++i)
    if (h->own[i].ok && h->own[i].w == W) return h->own[i];
  return h->own[0];
}

int own_ept(const xm_handle* h, u64 n, int W, bool vec16) {
  if (vec16 || h->own_ept_forced != 4) return 8;
  const double per = (double)n / (double)h->tb.xmap_w * (W + own_set(h, W).halo);
  return per * 1.12 <= 4.0 * COLS_MAX_THREADS ? 4 : 8;
}

unsigned cols_threads(const xm_handle* h, u64 n, int W, int ept = COLS_EPT) {
  if (h->own_mode) {  // own + halo columns in one pass where 512 threads hold them
    const double per = (double)n / (double)h->tb.xmap_w * (W + own_set(h, W).halo);
    const unsigned t = ((unsigned)(per * 1.12 / ept) + 63u) / 64u * 64u;
    return std::max(128u, std::min(t, (unsigned)COLS_MAX_THREADS));
  }
  const double per_tile = (double)n / (double)h->tb.xmap_w * W;
  // one pass for a tile 12 % above the mean (Poisson spread of an evenly filled scan); fuller tiles take a second pass.
  // Tiles of more than 2048 events get the full 512 threads even when 448 would hold them: three blocks per CU are then
  // 24 waves = every wave slot the kernel's 80 VGPRs allow (measured at C-1M, 3125 events per tile: 4.35 instead of 4.63 us
  // per frame at full occupancy; 384 threads = two passes: 5.9 us)
  unsigned t = ((unsigned)(per_tile * 1.12 / COLS_EPT) + 63u) / 64u * 64u;
  if (t > 256u) t = COLS_MAX_THREADS;
  return std::max(128u, std::min(t, (unsigned)COLS_MAX_THREADS));
}

// K0b: the tile boundaries + column thresholds of the frame(s), left behind the u16 frame.  Column tiles: one boundary per tile, 16
// lanes each on tiles of <= 16 columns, else 32 (cols_bounds_per_block); owner tiles: two per tile (its first column, the end of its
// halo behind it), 32 lanes.  flags: k_cols_bounds_batch's (a lone frame's kernel has none)
template <bool AOS, typename F>
void launch_cols_bounds(xm_handle* h, const F& fr, int W, int flags, hipStream_t stream) {
  const int split = h->own_mode ? own_set(h, W).halo : 0;
  const unsigned nb = (split ? 2u : 1u) * grid_for(h->tb.xmap_w, W);
  DevTables tb = h->tb;
  if constexpr (!is_lone<F>) {
    if (split) own_apply(own_set(h, W), tb);  // (a group's owner-tile K0b takes its plan's tables, a lone frame's the plain ones)
  }
  auto go = [&](auto lanes_tag) {
    constexpr int G = decltype(lanes_tag)::value;
    const unsigned gx = grid_for(nb + 1, cols_bounds_per_block(G));
    if constexpr (is_lone<F>)
      XM_LAUNCH((k_cols_bounds<AOS, G>), dim3(gx), dim3(256), 0, stream, fr.ev.x, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos,
                (u32)fr.ev.n, tb, W, static_cast<uint16_t*>(fr.frame), split);
    else
      XM_LAUNCH((k_cols_bounds_batch<AOS, G>), dim3(gx, fr.n), dim3(256), 0, stream, fr.descs, tb, W, flags, split);
  };
  if (!split && W <= 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
}

// K1 on the column tiles (xmaps_k1cols.hpp) or, where the rig's X-map is not injective, on the owner tiles (xmaps_k1own.hpp):
// grid = tiles (x frames), block from the mean frame (cols_threads).  flags: on top of h->cols_flags; lds_pad: extra dynamic LDS of
// a column-tile block (XM_COLS_LDS_PAD, experiments: fewer K1 blocks per CU, room for another kernel's -- the groups' launch only)
template <bool AOS, typename F>
int launch_tiles_k1(xm_handle* h, const F& fr, int W, int flags, size_t lds_pad, hipStream_t stream) {
  const bool v16 = !AOS && vec16(fr);
  const u64 n = fr.n_mean();
  const dim3 grid(grid_for(h->tb.xmap_w, W), frames(fr));
  flags |= h->cols_flags;
  if (h->own_mode) {
    const xm_handle::OwnSet& os = own_set(h, W);
    DevTables tbo = h->tb;
    own_apply(os, tbo);
    auto inst = [](auto vec_tag, auto ept_tag) {
      constexpr bool V = decltype(vec_tag)::value;
      constexpr int E = decltype(ept_tag)::value;
      if constexpr (is_lone<F>) return k_scatter_own<AOS, V, E>;
      else return k_scatter_own_batch<AOS, V, E>;
    };
    const int ept = own_ept(h, n, W, v16);
    auto kern = ept == 4 ? inst(std::false_type{}, std::integral_constant<int, 4>{})
                         : inst(std::false_type{}, std::integral_constant<int, COLS_EPT>{});
    if constexpr (!AOS) {
      if (v16) kern = inst(std::true_type{}, std::integral_constant<int, COLS_EPT>{});
    }
    const size_t lds = own_lds_bytes(os);
    int rc = h->ensure_lds(reinterpret_cast<const void*>(kern), lds);
    if (rc) return rc;
    const dim3 block(cols_threads(h, n, W, ept));
    if constexpr (is_lone<F>)
      XM_LAUNCH(kern, grid, block, lds, stream, fr.ev.x, fr.ev.y, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos, (u32)fr.ev.n, tbo,
                fr.st, static_cast<uint16_t*>(fr.frame), W, os.halo, flags);
    else
      XM_LAUNCH(kern, grid, block, lds, stream, fr.descs, tbo, W, os.halo, flags);
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
  const size_t lds = cols_lds_bytes(h, W) + lds_pad;
  int rc = h->ensure_lds(reinterpret_cast<const void*>(kern), lds);
  if (rc) return rc;
  const dim3 block(cols_threads(h, n, W));
  if constexpr (is_lone<F>)
    XM_LAUNCH(kern, grid, block, lds, stream, fr.ev.x, fr.ev.y, (const long long*)fr.ev.t, (const uint4*)fr.ev.aos, (u32)fr.ev.n, h->tb,
              fr.st, static_cast<uint16_t*>(fr.frame), W, h->w_x, h->cols_xr_min, flags);
  else
    XM_LAUNCH(kern, grid, block, lds, stream, fr.descs, h->tb, W, h->w_x, h->cols_xr_min, flags);
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

// ---- which path a frame or a group takes -----------------------------------------------------------------------------------------
bool sorted_path(const xm_handle* h, const EventsView& ev) {
  // the verified (t[0], t[n-1]) shortcut: both K1 kernels take it (tiled, and one thread per event for sparse frames)
  return (h->time_sorted || (h->try_sorted && !h->capturing)) && !ev.use_p && ev.n > 0;
}

// may this (sorted-path) frame use the compact key frame?  Needs the automatic redo (try-sorted mode, not inside a capture)
bool key32_path(const xm_handle* h, const EventsView& ev, bool sorted) {
  if (!sorted || !h->key32_ok || !h->try_sorted || h->capturing || h->key32_pause.load(std::memory_order_relaxed) > 0 ||
      h->k2_direct || h->k2_flags || !tiled_path(h, ev.n))
    return false;
  if (h->cfg.view != XM_VIEW_PROJECTOR) return ev.n <= (u64)CAM32_MAX_EVENTS;  // the key's order field is the event index
  return ev.n / (u64)(1024 / TILE_EPT * TILE_EPT) < (1ull << KEY32_TILE_BITS);  // tiles of >= 1024 events
}

// the column tiles' conditions on a frame: int64 time stamps, no polarity column, dense enough for a tile width of its own
bool cols_events(const xm_handle* h, const EventsView& ev) {
  return !ev.use_p && (ev.aos || ev.t_dtype == XM_T_INT64) && cols_width(h, ev.n) != 0;
}

// can this group of frames go through the multi-frame kernels?  (dense enough for the tiled K1, tiled K2 available)
bool batch_path(const xm_handle* h, u64 n_mean) {
  return tiled_path(h, n_mean) && !(h->cfg.view == XM_VIEW_PROJECTOR && h->k2_direct) && !h->k2_flags;
}

struct FramePath {
  bool per_frame = false;  // a group without a multi-frame path (untiled K2): frame by frame through enqueue_frame
  bool sorted = false;     // the verified (t[0], t[n-1]) shortcut: no K0
  bool direct = false;     // a group too sparse for the tiles: the one-thread-per-event K1 between the multi-frame K0 and K2
  int cols_w = 0;          // column / owner tiles of this width (0: none)
  bool dev_redo = false;   // a captured group on the column tiles: the redo decided on the device (launch_group)
  bool key32 = false;      // the compact key frame
  u64 n_max = 0, n_mean = 0;
  bool vec16 = true;       // every SoA frame's columns 16-byte aligned
  int kmode() const { return cols_w ? KM_COLS : key32 ? KM_KEY32 : KM_KEY64; }
  int counter() const { return cols_w ? 3 : key32 ? 2 : sorted ? 1 : 0; }  // index into h->path_counts
};

// The path of a lone frame (group = false) or of a group of n frames.  A group adds its own conditions on top of a lone frame's:
// the multi-frame kernels, or the one-thread-per-event K1 (>= 2 frames), or none; one tile width for all its frames (from the mean
// frame) and one layout (AoS / SoA); and while it is being captured (can_redo: descriptors for the redo at hand, >= 2 frames --
// a lone frame's seven launches, four of them returning at once, take longer than K0 -> K1 -> K2) the column tiles with the
// redo decided on the device.  A lone frame takes the column tiles only under cols_single.
FramePath frame_path(const xm_handle* h, const EventsView* evs, int n, bool allow_sorted, bool group = false, bool can_redo = false) {
  FramePath p;
  u64 n_sum = 0;
  bool one_layout = true;
  p.sorted = allow_sorted && n > 0;
  for (int f = 0; f < n; ++f) {
    const EventsView& ev = evs[f];
    p.n_max = std::max<u64>(p.n_max, ev.n);
    n_sum += ev.n;
    if (!ev.aos) p.vec16 = p.vec16 && ev_vec16(ev);
    p.sorted = p.sorted && sorted_path(h, ev);
    one_layout = one_layout && (ev.aos != nullptr) == (evs[0].aos != nullptr);
  }
  p.n_mean = n ? n_sum / (u64)n : 0;
  if (group) {
    // frames too sparse for the tiled K1 (the reference's own recordings: ~150 k events over 1080 time columns): the multi-frame
    // K0 and K2 with the one-thread-per-event K1 in between -- three launches per group instead of three per frame
    const bool tiled = batch_path(h, p.n_mean);
    p.direct = !tiled && !(h->cfg.view == XM_VIEW_PROJECTOR && (h->k2_direct || !h->d_k2_tiles[1])) && !h->k2_flags && n >= 2 &&
               p.n_max < (1ull << 31);
    p.per_frame = !tiled && !p.direct;
    if (p.per_frame) return p;
  }
  auto tile_width = [&] {
    int W = one_layout ? cols_width(h, p.n_mean) : 0;
    for (int f = 0; f < n && W; ++f)
      if (!cols_events(h, evs[f])) W = 0;
    return W;
  };
  // the column tiles need the automatic redo at hand on the host, as the compact key frame does
  if (p.sorted && (group || h->cols_single) && h->cols_ok && h->try_sorted && !h->capturing &&
      h->key32_pause.load(std::memory_order_relaxed) <= 0 && !h->k2_direct && !h->k2_flags)
    p.cols_w = tile_width();
  else if (group && can_redo && n >= 2 && h->capturing && !p.direct && h->cols_ok && !h->k2_direct && !h->k2_flags)
    p.dev_redo = (p.cols_w = tile_width()) != 0;
  p.key32 = p.sorted && !p.cols_w && !p.direct;
  for (int f = 0; f < n && p.key32; ++f) p.key32 = key32_path(h, evs[f], p.sorted);
  return p;
}

// keep the slot's compact frame unambiguous for a frame with tag `tag` (4-bit tags repeat every 15 frames)
int key32_prepare(xm_handle* h, Slot& s, u32 tag, hipStream_t stream) {
  if (h->cfg.view != XM_VIEW_PROJECTOR) return XM_OK;  // camera view: no tag -- the frame kernel zeroes every pixel it reads
  if (tag - s.key32_valid_from >= 15u || tag < s.key32_valid_from) {
    HIP_TRY(hipMemsetAsync(s.key32, 0, h->key_cells * sizeof(u32), stream));
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
  const FramePath p = frame_path(h, &ev, 1, allow_sorted);
  key32_pause_tick(h, 1);
  hipStream_t stream = stream_override ? stream_override : s.stream;
  // the slot's previous frame may have run inside a group or a replay on another stream (the own stream's eager work: a group's
  // stream was ordered behind it by enqueue_batch, the own stream needs no order with itself)
  if (int rc = s.order.before_group_only(stream)) return rc;
  if (s.last.host_tag >= KEY_MAX_TAG) {  // tag field about to wrap: clear the frame once per 2^19 frames
    int rc = reset_slot(h, s, stream);
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
      const int rc_k = key32_prepare(h, s, s.last.host_tag + 1, stream);
      if (rc_k) return rc_k;
    }
    ps.at(1);
    if (skip & 2) return XM_OK;
    if constexpr (tile_types<E>) {
      if (p.cols_w) return launch_tiles_k1<E::AOS>(h, fr, p.cols_w, 0, 0, stream);
    }
    return launch_k1<typename E::T, E::AOS, E::HAS_P>(h, fr, tiled_path(h, ev.n), p.key32, p.sorted, stream);
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
