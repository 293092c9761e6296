// xm_launch.hpp -- kernel dispatch: the two forms a launch takes its frames in, the (aos, use_p, t_dtype) dispatch, and the
// launchers of K0 (extrema), K1 (tiled / one thread per event) and K2 (every view and key format, pipelined K2)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

// ---- the two forms a launch takes its frames in ------------------------------------------------------------------------
// A lone frame passes its events as the kernels' own arguments (nothing to upload on the latency path); a group passes n
// descriptors in device memory, frame = blockIdx.y (K2: blockIdx.z).  Every launcher serves both forms: the kernel instance,
// grid, block and dynamic LDS come from one rule; only the frame dimension and the per-frame pointers differ.
struct LoneFrame {
  const EventsView& ev;
  SlotState* st;
  u32 tag_override;
  void* frame = nullptr;  // K1's output, K2's input: the 64-bit / compact key frame, or the column tiles' u16 frame
  unsigned char* dirty = nullptr;
  float* depth = nullptr;
  uint8_t* bgr = nullptr;
  u64 idx_offset = 0, mm_lo = 0, mm_hi = 0;  // shards: global index of the first event, the frame's extrema
  const void* mm_ext = nullptr;              // sharded mode: {tmin, -tmax} in device memory (NULL: mm_lo / mm_hi)
  u64 n_max() const { return ev.n; }
  u64 n_mean() const { return ev.n; }
};
struct FrameGroup {
  const FrameDesc* descs;
  int n;                        // frames
  u64 events_max, events_mean;  // the largest frame (grids) and the mean frame (block sizes)
  bool all_vec16;               // every SoA frame's columns 16-byte aligned (ev_vec16)
  u64 n_max() const { return events_max; }
  u64 n_mean() const { return events_mean; }
};
template <typename F>
constexpr bool is_lone = std::is_same<F, LoneFrame>::value;
unsigned frames(const LoneFrame&) { return 1; }
unsigned frames(const FrameGroup& g) { return (unsigned)g.n; }

bool vec16(const LoneFrame& f) { return ev_vec16(f.ev); }
bool vec16(const FrameGroup& g) { return g.all_vec16; }

// prof = 6 events {start0, stop0, start1, stop1, start2, stop2} attached to the dispatch packets of K0 / K0b, K1, K2 (g_prof);
// cleared when the frame's or group's launches are issued, on every return
struct ProfSlots {
  const Event* prof;
  void at(int i) const {
    if (prof) g_prof = ProfCtx{prof[2 * i], prof[2 * i + 1]};
  }
  ~ProfSlots() { g_prof = ProfCtx{}; }
};

// ---- (aos, use_p, t_dtype) -> template arguments -------------------------------------------------------------------------------
// fn(EvTypes<T, AOS, HAS_P>{}) for the eight event layouts the kernels are instantiated for (AoS EventCD: int64 time stamps)
template <typename T_, bool AOS_, bool HAS_P_>
struct EvTypes {
  using T = T_;
  static constexpr bool AOS = AOS_, HAS_P = HAS_P_;
};
template <typename Fn>
auto with_event_types(const EventsView& ev, Fn&& fn) {
  if (ev.aos) return ev.use_p ? fn(EvTypes<long long, true, true>{}) : fn(EvTypes<long long, true, false>{});
  switch (ev.t_dtype) {
    case XM_T_INT64: return ev.use_p ? fn(EvTypes<long long, false, true>{}) : fn(EvTypes<long long, false, false>{});
    case XM_T_FLOAT32: return ev.use_p ? fn(EvTypes<float, false, true>{}) : fn(EvTypes<float, false, false>{});
    default: return ev.use_p ? fn(EvTypes<double, false, true>{}) : fn(EvTypes<double, false, false>{});
  }
}
// the layouts of the column / owner tiles (and of a captured group's redo): int64 time stamps, no polarity column
template <typename E>
constexpr bool tile_types = std::is_same<typename E::T, long long>::value && !E::HAS_P;

// ---- K0 (extrema) ---------------------------------------------------------------------------------------------------------------
// VEC2 (16-byte loads of int64 SoA time stamps): a lone frame needs its t (and p) aligned, a group every column of every frame
bool k0_vec2(const LoneFrame& f) { return xm::k0_vec2(f.ev); }
bool k0_vec2(const FrameGroup& g) { return g.all_vec16; }

// COND = 1: the redo node of a captured group (cap = 64: usually every block returns at once)
template <typename T, bool AOS, bool HAS_P, int COND = 0, typename F>
void launch_k0(const F& fr, hipStream_t stream, unsigned cap = 1024) {
  auto go = [&](auto vec_tag) {
    constexpr int VEC = decltype(vec_tag)::value;
    const unsigned gx = k0_blocks(fr.n_max(), VEC == 2, cap);
    if constexpr (is_lone<F>)
      XM_LAUNCH((k_minmax<T, AOS, HAS_P, VEC>), dim3(gx), dim3(BLOCK), 0, stream, (const T*)fr.ev.t, fr.ev.p,
                (const uint4*)(VEC == 2 ? nullptr : fr.ev.aos), fr.ev.n, fr.st, fr.tag_override);
    else
      XM_LAUNCH((k_minmax_batch<T, AOS, HAS_P, VEC, COND>), dim3(gx, fr.n), dim3(BLOCK), 0, stream, fr.descs);
  };
  if constexpr (!AOS && std::is_same<T, long long>::value) {
    if (k0_vec2(fr)) return go(std::integral_constant<int, 2>{});
  }
  go(std::integral_constant<int, 1>{});
}

void launch_minmax(const EventsView& ev, SlotState* st, u32 tag_override, hipStream_t stream) {
  with_event_types(ev, [&](auto ty) {
    using E = decltype(ty);
    launch_k0<typename E::T, E::AOS, E::HAS_P>(LoneFrame{ev, st, tag_override}, stream);
  });
}

// ---- K1 (scatter): tiled, or one thread per event --------------------------------------------------------------------------------
// (when a frame takes the tiled kernel, and its block: tiled_path / k1_tiled_shape, xm_plan.hpp)
// tiled: the tiled kernel (key32: onto the compact key frame), else one thread per event.  COND = 1: the redo node of a captured
// group (projector view, 64-bit keys, at most 32 blocks per frame)
template <typename T, bool AOS, bool HAS_P, int COND = 0, typename F>
int launch_k1(xm_handle* h, const F& fr, bool tiled, bool key32, bool sorted, hipStream_t stream) {
  const RigPlan& pl = h->plan();
  auto go = [&](auto view_tag) -> int {
    constexpr int VIEW = decltype(view_tag)::value;
    if (!tiled) {
      if constexpr (is_lone<F>) {
        const EventsView& ev = fr.ev;
        const bool vec = !AOS && aligned(ev.x, 8) && aligned(ev.y, 8) && aligned(ev.t, 16) && (!HAS_P || aligned(ev.p, 8));
        if constexpr (AOS)
          XM_LAUNCH((k_scatter<T, true, HAS_P, 1, VIEW>), dim3(k1_direct_blocks(ev.n, false)), dim3(BLOCK), 0, stream,
                    (const uint16_t*)nullptr, (const uint16_t*)nullptr, (const T*)nullptr, (const int16_t*)nullptr,
                    (const uint4*)ev.aos, ev.n, fr.idx_offset, h->tb, fr.st, fr.tag_override, fr.mm_lo, fr.mm_hi, fr.mm_ext,
                    (u64*)fr.frame, fr.dirty, sorted ? 1 : 0);
        else if (vec)
          XM_LAUNCH((k_scatter<T, false, HAS_P, 4, VIEW>), dim3(k1_direct_blocks(ev.n, true)), dim3(BLOCK), 0, stream, ev.x, ev.y,
                    (const T*)ev.t, ev.p, (const uint4*)nullptr, ev.n, fr.idx_offset, h->tb, fr.st, fr.tag_override, fr.mm_lo,
                    fr.mm_hi, fr.mm_ext, (u64*)fr.frame, fr.dirty, sorted ? 1 : 0);
        else
          XM_LAUNCH((k_scatter<T, false, HAS_P, 1, VIEW>), dim3(k1_direct_blocks(ev.n, false)), dim3(BLOCK), 0, stream, ev.x, ev.y,
                    (const T*)ev.t, ev.p, (const uint4*)nullptr, ev.n, fr.idx_offset, h->tb, fr.st, fr.tag_override, fr.mm_lo,
                    fr.mm_hi, fr.mm_ext, (u64*)fr.frame, fr.dirty, sorted ? 1 : 0);
      } else {  // grid = (blocks of the largest frame, frames)
        XM_LAUNCH((k_scatter_direct_batch<T, AOS, HAS_P, VIEW>), dim3(k1_direct_blocks(fr.n_max(), false), fr.n), dim3(BLOCK), 0, stream,
                  fr.descs, h->tb, sorted ? 1 : 0);
      }
      return XM_OK;
    }
    auto inst = [](auto vec_tag, auto key32_tag) {
      constexpr bool V = decltype(vec_tag)::value, K = decltype(key32_tag)::value;
      if constexpr (is_lone<F>) return k_scatter_tiled<T, AOS, HAS_P, VIEW, V, K>;
      else return k_scatter_tiled_batch<T, AOS, HAS_P, VIEW, V, K, COND>;
    };
    // vector-load variant: 16-byte aligned SoA columns with int64 t (the EventCD time type); everything else takes the
    // lane-strided loads (any alignment)
    constexpr bool kHasVec = !AOS && std::is_same<T, long long>::value;
    const bool v16 = kHasVec && vec16(fr);
    auto kern = inst(std::false_type{}, std::false_type{});
    if constexpr (kHasVec) {
      if (v16) kern = inst(std::true_type{}, std::false_type{});
    }
    if constexpr (COND == 0) {
      if (key32) {
        kern = inst(std::false_type{}, std::true_type{});
        if constexpr (kHasVec) {
          if (v16) kern = inst(std::true_type{}, std::true_type{});
        }
      }
    }
    // raise the kernel's dynamic-LDS cap once per (handle = device, kernel instantiation); gfx950: 160 KB / CU
    const K1TiledShape sh = k1_tiled_shape(pl, fr.n_max(), fr.n_mean(), COND == 1);
    int rc = h->ensure_lds(reinterpret_cast<const void*>(kern), sh.lds);
    if (rc) return rc;
    if constexpr (is_lone<F>) {
      const EventsView& ev = fr.ev;
      XM_LAUNCH(kern, dim3(sh.gx), dim3(sh.threads), sh.lds, stream, ev.x, ev.y, (const T*)ev.t, ev.p, (const uint4*)ev.aos, ev.n,
                fr.idx_offset, h->tb, fr.st, fr.tag_override, fr.mm_lo, fr.mm_hi, fr.mm_ext, (u64*)fr.frame, fr.dirty, pl.k1.w_ts,
                pl.k1.w_x, sorted ? 1 : 0);
    } else {
      XM_LAUNCH(kern, dim3(sh.gx, fr.n), dim3(sh.threads), sh.lds, stream, fr.descs, h->tb, pl.k1.w_ts, pl.k1.w_x, sorted ? 1 : 0);
    }
    return XM_OK;
  };
  if (COND == 1 || pl.dims.projector) return go(std::integral_constant<int, 0>{});
  if constexpr (COND == 0) return go(std::integral_constant<int, 1>{});
  return XM_OK;
}

int launch_scatter(xm_handle* h, const EventsView& ev, SlotState* st, u32 tag_override, u64 idx_offset, u64 mm_lo,
                   u64 mm_hi, u64* frame, unsigned char* dirty, hipStream_t stream, bool sorted = false,
                   const void* mm_ext = nullptr, bool key32 = false) {
  const LoneFrame fr{ev, st, tag_override, frame, dirty, nullptr, nullptr, idx_offset, mm_lo, mm_hi, mm_ext};
  return with_event_types(ev, [&](auto ty) -> int {
    using E = decltype(ty);
    return launch_k1<typename E::T, E::AOS, E::HAS_P>(h, fr, tiled_path(h->plan(), ev.n), key32, sorted, stream);
  });
}

// ---- K2 launches (tiled frame kernel, projector view) -----------------------------------------------------------------------
// (pixels per thread, grid and LDS of a launch: k2_tiled_shape, xm_plan.hpp)
template <int FMT>
void launch_k2(xm_handle* h, hipStream_t stream, const u64* key_frame, SlotState* st, u32 tag_override, const unsigned char* dirty,
               float* depth, uint8_t* bgr, bool unsheared = false, int col_lo = 0, int col_hi = 0) {
  const K2TiledShape sh = k2_tiled_shape(h->plan(), 1);
  const dim3 grid(sh.gx, sh.gy);
  DevTables tb = h->tb;
  if (unsheared) tb.shear_m = tb.shear_bias = tb.shear_extra = 0;  // a plain [rect_w][rect_h] u16 frame (shards), not a slot's frame16
  if (sh.ppt == 1)
    XM_LAUNCH((k_frame_proj_tiled<FMT, 1>), grid, dim3(sh.threads), sh.lds, stream, key_frame, tb, st, tag_override,
              dirty, (const ulonglong2*)h->d_zero16, depth, bgr, sh.tile_cap, col_lo, col_hi);
  else
    XM_LAUNCH((k_frame_proj_tiled<FMT, 2>), grid, dim3(sh.threads), sh.lds, stream, key_frame, tb, st, tag_override,
              dirty, (const ulonglong2*)h->d_zero16, depth, bgr, sh.tile_cap, col_lo, col_hi);
}

// the software-pipelined K2 (persistent blocks walking (frame, tile) items): whether a group takes it, and its shape, is
// k2_pipe_shape's (xm_plan.hpp); false = the group goes to the tiled K2
template <int COND = 0>
bool launch_k2_pipe(xm_handle* h, hipStream_t stream, const FrameDesc* d_descs, int n_frames) {
  const RigPlan& pl = h->plan();
  const K2PipeShape sh = k2_pipe_shape(pl, n_frames);
  if (!sh.use) return false;
  const int g = sh.g;
  const bool cs = sh.consecutive;
  const void* fn = g == 2 ? (cs ? reinterpret_cast<const void*>(k_frame_proj_pipe<4, true, COND>) : reinterpret_cast<const void*>(k_frame_proj_pipe<4, false, COND>))
                          : (cs ? reinterpret_cast<const void*>(k_frame_proj_pipe<2, true, COND>) : reinterpret_cast<const void*>(k_frame_proj_pipe<2, false, COND>));
  if (h->ensure_lds(fn, sh.lds) != XM_OK) return false;
  K2PipeArgs pa;
  pa.proj_w = h->tb.proj_w; pa.proj_h = h->tb.proj_h; pa.rect_w = h->tb.rect_w; pa.rect_h = h->tb.rect_h;
  pa.shear_m = h->tb.shear_m; pa.shear_bias = h->tb.shear_bias;
#define XM_K2P_LAUNCH(P, C)                                                                                                          \
  XM_LAUNCH((k_frame_proj_pipe<P, C, COND>), dim3(sh.blocks), dim3(K2_TX * K2_TY), sh.lds, stream, d_descs, (const int4*)h->d_k2_tiles[g], \
            (const u32*)h->d_k2_pix[g], (const uint16_t*)h->d_k2_pix16[g], pl.k2pipe.pix_stride, h->tb.dlut, pa, pl.k2.tile_cap[g],  \
            (u32)n_frames, sh.gx, sh.gy, pl.k2pipe.nlds, sh.gx_magic, (const uint4*)h->d_k2_live[g])
  std::unique_lock<std::mutex> chain_lock(h->k2_chain_mu, std::defer_lock);
  if (pl.k2pipe.chain && COND == 0) {  // one K2 at a time: wait for the one launched last (whatever its stream)
    chain_lock.lock();
    if (h->k2_chain_n) (void)hipStreamWaitEvent(stream, h->k2_chain_ev[(h->k2_chain_n - 1) % 16], 0);
  }
  if (g == 2) {
    if (cs) XM_K2P_LAUNCH(4, true);
    else XM_K2P_LAUNCH(4, false);
  } else {
    if (cs) XM_K2P_LAUNCH(2, true);
    else XM_K2P_LAUNCH(2, false);
  }
#undef XM_K2P_LAUNCH
  if (chain_lock.owns_lock()) {
    Event& ev = h->k2_chain_ev[h->k2_chain_n % 16];
    if (!ev) (void)ev.create();
    if (ev && hipEventRecord(ev, stream) == hipSuccess) h->k2_chain_n += 1;
  }
  h->k2_pipe_frames += (uint64_t)n_frames;
  return true;
}

template <int FMT, int COND = 0>
void launch_k2_batch(xm_handle* h, hipStream_t stream, const FrameDesc* d_descs, int n_frames) {
  if constexpr (FMT == 2 && (COND == 0 || COND == 2)) {  // (COND = 2: the attempt's K2 node of a captured batch)
    if (launch_k2_pipe<COND>(h, stream, d_descs, n_frames)) return;
  }
  const K2TiledShape sh = k2_tiled_shape(h->plan(), n_frames, COND == 1);  // (redo node: a few blocks per frame walk its tiles)
  const dim3 grid(sh.gx, sh.gy, sh.gz);
  if (sh.ppt == 1)
    XM_LAUNCH((k_frame_proj_tiled_batch<FMT, COND, 1>), grid, dim3(sh.threads), sh.lds, stream, d_descs, h->tb,
              (const ulonglong2*)h->d_zero16, sh.tile_cap);
  else
    XM_LAUNCH((k_frame_proj_tiled_batch<FMT, COND, 2>), grid, dim3(sh.threads), sh.lds, stream, d_descs, h->tb,
              (const ulonglong2*)h->d_zero16, sh.tile_cap);
}

// K2 of a frame or a group by view and key format (kmode).  Projector view: the tiled frame kernel (a lone frame: k2_ppt(plan, 1);
// under XM_K2_DIRECT the per-pixel kernel, under XM_K2_FLAGS with the dirty map); camera view: k_frame_cam32 on the compact key
// frame, k_frame_direct otherwise
template <typename F>
void launch_frame_kernel(xm_handle* h, const F& fr, int kmode, hipStream_t stream) {
  const RigPlan& pl = h->plan();
  const bool proj = pl.dims.projector, key32 = kmode == KM_KEY32;
  const u64 px = cam_pixels(pl);
  const dim3 g32(cam32_gx(pl), cam32_gy(pl), frames(fr));
  if constexpr (is_lone<F>) {
    const u64* keys = static_cast<const u64*>(fr.frame);
    const KeyCells cells{keys, 0};
    if (proj && pl.modes.k2_direct)
      XM_LAUNCH((k_frame_proj<KeyCells, 0>), dim3(pixel_blocks((u64)pl.dims.proj_w * pl.dims.proj_h)), dim3(BLOCK), 0, stream, cells,
                h->tb, fr.st, fr.tag_override, fr.depth, fr.bgr);
    else if (proj && kmode == KM_COLS) launch_k2<2>(h, stream, keys, fr.st, fr.tag_override, nullptr, fr.depth, fr.bgr);
    else if (proj && key32) launch_k2<1>(h, stream, keys, fr.st, fr.tag_override, nullptr, fr.depth, fr.bgr);
    else if (proj) launch_k2<0>(h, stream, keys, fr.st, fr.tag_override, pl.modes.k2_flags ? fr.dirty : nullptr, fr.depth, fr.bgr);
    else if (key32)  // camera view, compact frame: (event index + 1) << 12 | disparity, zeroed as it is read
      XM_LAUNCH(k_frame_cam32, g32, dim3(BLOCK), 0, stream, static_cast<u32*>(fr.frame), h->tb.cam_w, h->tb.cam_h, fr.st, h->tb.dlut,
                fr.depth, fr.bgr);
    else
      XM_LAUNCH((k_frame_direct<KeyCells>), dim3(pixel_blocks(px)), dim3(BLOCK), 0, stream, cells, px, h->tb.p03, h->tb.z_near,
                h->tb.z_far, fr.st, fr.tag_override, 1, h->tb.dlut, fr.depth, fr.bgr);
  } else {
    if (proj && kmode == KM_COLS) launch_k2_batch<2>(h, stream, fr.descs, fr.n);
    else if (proj && key32) launch_k2_batch<1>(h, stream, fr.descs, fr.n);
    else if (proj) launch_k2_batch<0>(h, stream, fr.descs, fr.n);
    else if (key32) XM_LAUNCH(k_frame_cam32_batch, g32, dim3(BLOCK), 0, stream, fr.descs, h->tb.cam_w, h->tb.cam_h, h->tb.dlut);
    else XM_LAUNCH(k_frame_direct_batch, dim3(pixel_blocks(px), fr.n), dim3(BLOCK), 0, stream, fr.descs, px, h->tb.dlut);
  }
}

// ---- the ingest's frame-filter stage (xmaps_ingest_filter.hpp) ----------------------------------------------------------------
// One cut frame through the selected filter: events -> cells -> survivors in raster order + the second descriptor.  n_bound: the
// verdict's event count (the cut frame's length: the event passes' grids; the survivors' upper bound for K0 / K1 behind this).
// The cell passes take one block per FF_BLOCK cells of the fixed map; the width pass goes out only where a column can wrap.
unsigned ff_cell_blocks(const FrameFilterDev& f) { return grid_for(f.n_cells, FF_BLOCK); }
void launch_frame_filter(const FrameFilterDev& f, u64 n_bound, hipStream_t stream) {
  const unsigned ge = grid_for(n_bound < 1 ? 1 : n_bound, FF_THREADS), gc = ff_cell_blocks(f);
  if (f.wrap) XM_LAUNCH(k_ff_width, dim3(ge), dim3(FF_THREADS), 0, stream, f);
  XM_LAUNCH(k_ff_scatter, dim3(ge), dim3(FF_THREADS), 0, stream, f);
  XM_LAUNCH(k_ff_count, dim3(gc), dim3(FF_BLOCK), 0, stream, f);
  XM_LAUNCH(k_ff_emit, dim3(gc), dim3(FF_BLOCK), 0, stream, f, (u32)gc);
}

// ---- frames -> camera time surfaces (xmaps_framesurface.hpp): the group entry and the ingest's surface stage ---------------------
// One launch sequence: n_frames (<= FS_GROUP) frames, the longest of n_max events (the ingest: the verdict's count).  The event
// pass takes one block per FS_CHUNK events of the longest frame, at most a.max_chunk_blocks; the cell pass one per
// FS_CELLS_PER_BLOCK cells of the fixed map.
u32 frame_max_chunk_blocks(const char* option) {  // ("XM_FS_MAX_BLOCKS" / "XM_FC_MAX_BLOCKS" / "XM_ENC_MAX_BLOCKS": tests send short frames through the
  const char* o = dbg_opt(option);                 // chunk loops' further trips)
  const long v = o ? atol(o) : 0;
  return v > 0 && v < 65535 ? (u32)v : 4096u;
}
void launch_frame_surfaces(const FsArgs& a, unsigned n_frames, u64 n_max, int dtype, hipStream_t stream) {
  const unsigned ge = std::min<unsigned>(grid_for(n_max < 1 ? 1 : n_max, FS_CHUNK), a.max_chunk_blocks);
  const unsigned gc = grid_for(a.cells, FS_CELLS_PER_BLOCK);
  XM_LAUNCH(k_fs_events, dim3(ge, n_frames), dim3(FS_THREADS), 0, stream, a);
  if (dtype == XM_T_FLOAT32) XM_LAUNCH(k_fs_pixels<float>, dim3(gc, n_frames), dim3(FS_THREADS), 0, stream, a);
  else XM_LAUNCH(k_fs_pixels<double>, dim3(gc, n_frames), dim3(FS_THREADS), 0, stream, a);
  XM_LAUNCH(k_fs_finish, dim3(grid_for(n_frames, 64)), dim3(64), 0, stream, a, (u32)n_frames);
}

// ---- frames -> per-event point clouds (xmaps_framecloud.hpp): the group entry and the ingest's cloud stage ------------------------
// One launch sequence: n_frames (<= FC_GROUP) frames, the longest of n_max events (the ingest: the verdict's count).  The three
// per-event passes take one block per FC_CHUNK events of the longest frame, at most a.max_chunk_blocks; the scan one per frame.
void launch_frame_clouds(const FcArgs& a, unsigned n_frames, u64 n_max, hipStream_t stream) {
  const unsigned ge = std::min<unsigned>(grid_for(n_max < 1 ? 1 : n_max, FC_CHUNK), a.max_chunk_blocks);
  XM_LAUNCH(k_fc_extrema, dim3(ge, n_frames), dim3(FC_THREADS), 0, stream, a);
  XM_LAUNCH(k_fc_events, dim3(ge, n_frames), dim3(FC_THREADS), 0, stream, a);
  XM_LAUNCH(k_fc_scan, dim3(n_frames), dim3(FC_SCAN_BLOCK), 0, stream, a);
  if (a.cloud) XM_LAUNCH(k_fc_points, dim3(ge, n_frames), dim3(FC_THREADS), 0, stream, a);
  if (a.tag) XM_LAUNCH(k_fc_publish, dim3(1), dim3(64), 0, stream, a);
}

// ---- frames -> EVT 3.0 words (xmaps_evt3enc.hpp): the group entry and the ingest's record stage ---------------------------------
// One launch sequence: n_frames (<= ENC_GROUP) frames, the longest of n_max events (the ingest: the verdict's count).  The three
// per-event passes take one block per ENC_CHUNK events of the longest frame, at most a.max_chunk_blocks ("XM_ENC_MAX_BLOCKS"); the
// scan one per frame.
void launch_frame_records(const EncArgs& a, unsigned n_frames, u64 n_max, hipStream_t stream) {
  const unsigned ge = std::min<unsigned>(grid_for(n_max < 1 ? 1 : n_max, ENC_CHUNK), a.max_chunk_blocks);
  XM_LAUNCH(k_enc_runs, dim3(ge, n_frames), dim3(ENC_THREADS), 0, stream, a);
  XM_LAUNCH(k_enc_count, dim3(ge, n_frames), dim3(ENC_THREADS), 0, stream, a);
  XM_LAUNCH(k_enc_scan, dim3(n_frames), dim3(ENC_SCAN_BLOCK), 0, stream, a);
  XM_LAUNCH(k_enc_emit, dim3(ge, n_frames), dim3(ENC_THREADS), 0, stream, a);
  if (a.tag) XM_LAUNCH(k_enc_publish, dim3(1), dim3(64), 0, stream, a);
}


}  // namespace
