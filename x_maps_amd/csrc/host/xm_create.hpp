// xm_create.hpp -- the stages of xm_create, in the order it calls them.  The stages up to apply_k1_windows fill the rig plan
// (RigPlan, xm_plan.hpp) through xm_handle::plan_in_create() -- the only code that writes it; from build_k2_live on a stage is
// handed the finished plan as a const RigPlan&, like everything outside this file.  Every stage returns an xm_* code; a failure leaves the
// half-built handle to xm_destroy (xm_create holds it in an Owned<>).  The order of the HIP calls on the device, every
// hipDeviceSynchronize among them, is part of the contract: the stages' default-stream work must not be reordered.
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

// the switches that have no field of their own in the plan: read once (read_create_options), used by one stage each
struct CreateOpts {
  const char* k2_pipe_ppt = nullptr;  // "XM_K2_PIPE_PPT" (experiments / tests): 2 / 4
  const char* key32 = nullptr;        // "XM_KEY32": 0 = no compact key frame
  const char* cols = nullptr;         // "XM_COLS": 0 = off, 1 = groups only, 2 = also single-frame calls
  const char* workers = nullptr;      // "XM_WORKERS": overrides XM_FLAG_LAUNCH_WORKERS either way
  const char* ablate = nullptr;       // "XM_ABLATE" (builds with -DXM_ABLATE only)
  int k2_nlds_max = 2048;             // "XM_K2_NLDS_MAX" (experiments)
  int k1_wx = 16;                     // "XM_K1_WX" (experiments): the LUT band's width in camera columns
  std::vector<int4> k2_tiles[3];      // the K2 tile records, copied back once (build_k2_tables) for build_k2_live
};

int validate_config(const xm_config* cfg) {
  if (cfg->struct_size != sizeof(xm_config))
    return fail(XM_ERR_INVALID, "xm_config.struct_size %u != %zu", cfg->struct_size, sizeof(xm_config));
  if (cfg->cam_width <= 0 || cfg->cam_height <= 0 || cfg->rect_width <= 0 || cfg->rect_height <= 0 ||
      cfg->xmap_width <= 1)
    return fail(XM_ERR_INVALID, "bad dimensions");
  if (cfg->cam_width > 32767 || cfg->cam_height > 32767 || cfg->rect_width > 32767 || cfg->rect_height > 32767 ||
      cfg->xmap_width > 32767 || cfg->proj_width > 32767 || cfg->proj_height > 32767)
    return fail(XM_ERR_INVALID, "dimensions must fit int16 indices (x_maps_disparity.py:52-53)");
  if (cfg->x_offset < 0 || cfg->x_offset > 32767) return fail(XM_ERR_INVALID, "x_offset must fit int16");
  if (cfg->view != XM_VIEW_PROJECTOR && cfg->view != XM_VIEW_CAMERA) return fail(XM_ERR_INVALID, "bad view");
  if (!cfg->cam_mapx_i16 || !cfg->cam_mapy_i16 || !cfg->proj_x_map) return fail(XM_ERR_INVALID, "NULL table");
  if (cfg->view == XM_VIEW_PROJECTOR && (!cfg->disp_proj_mapxy_i16 || cfg->proj_width <= 0 || cfg->proj_height <= 0))
    return fail(XM_ERR_INVALID, "projector view needs disp_proj_mapxy_i16 and the projector size");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(XM_ERR_HIP, "no HIP device visible: the X-maps hot path needs an AMD GPU (no CPU fallback)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(XM_ERR_INVALID, "device %d out of range (%d)", cfg->device, ndev);
  return XM_OK;
}

// Every switch xm_create reads (xm_debug_option sets them; see dbg_opt), in one place, and for every rig ("XM_K2_PPT" and
// "XM_K2_PIPE_PPT" used to be read only when the rig has a projector map: only K2's projector path looks at what they set).
// (own_setup reads the owner tiles' own: "XM_OWN_W", "XM_OWN_GROUPED", "XM_OWN_EPT".)
void read_create_options(RigPlan& p, CreateOpts& o) {
  if (const char* e = dbg_opt("XM_K2_PPT")) p.k2.force_ppt = atoi(e);
  o.k2_pipe_ppt = dbg_opt("XM_K2_PIPE_PPT");
  o.key32 = dbg_opt("XM_KEY32");
  if (const char* e = dbg_opt("XM_K2_NLDS_MAX")) o.k2_nlds_max = std::max(1, std::min(4096, atoi(e)));
  if (const char* e = dbg_opt("XM_K2_PIPE")) {
    p.k2pipe.on = e[0] != '0';
    p.k2pipe.force = e[0] == '2';
  }
  if (const char* e = dbg_opt("XM_K2_CHAIN")) p.k2pipe.chain = e[0] != '0';
  if (const char* e = dbg_opt("XM_K2_PER_CU")) p.k2pipe.per_cu_max = std::max(1, atoi(e));
  if (const char* e = dbg_opt("XM_K2_PIPE_BLOCKS")) p.k2pipe.blocks_cap = std::max(0, atoi(e));
  if (const char* e = dbg_opt("XM_COLS_LDS_PAD")) p.cols.lds_pad = std::max(0, std::min(64 * 1024, atoi(e)));
  if (const char* e = dbg_opt("XM_K2_LIVE")) {
    p.k2pipe.live = e[0] != '0';
    p.k2pipe.live_report = e[0] == '2';
  }
  if (const char* e = dbg_opt("XM_K2_CONSEC")) p.k2pipe.consec = e[0] != '0' ? 1 : 0;  // experiments / tests: the strided pixel assignment
  o.cols = dbg_opt("XM_COLS");
  const char* e1 = dbg_opt("XM_K1_DIRECT");
  const char* e2 = dbg_opt("XM_K2_DIRECT");
  p.modes.k1_direct = e1 && e1[0] == '1';
  p.modes.k2_direct = e2 && e2[0] == '1';
  if (const char* e3 = dbg_opt("XM_K2_FLAGS")) p.modes.k2_flags = e3[0] == '1';
  if (const char* e = dbg_opt("XM_K1_WX")) o.k1_wx = std::max(2, std::min(64, atoi(e)));
#ifdef XM_ABLATE
  o.ablate = dbg_opt("XM_ABLATE");
#endif
  o.workers = dbg_opt("XM_WORKERS");
}

// re-pack the int16 tables: one 4-byte gather per event instead of two 2-byte ones, and the scan axis made the
// slow axis (column-major) so that a time slice of events touches a few contiguous runs (see DevTables)
int upload_tables(xm_handle* h) {
  const xm_config* cfg = &h->cfg;
  const int xmap_h = cfg->xmap_height;
  const size_t cam_px = (size_t)cfg->cam_width * cfg->cam_height;
  {
    std::vector<u32> lut(cam_px);
    for (int y = 0; y < cfg->cam_height; ++y)
      for (int x = 0; x < cfg->cam_width; ++x) {
        const size_t i = (size_t)y * cfg->cam_width + x;
        lut[(size_t)x * cfg->cam_height + y] =
            ((u32)(uint16_t)cfg->cam_mapy_i16[i] << 16) | (u32)(uint16_t)cfg->cam_mapx_i16[i];
      }
    HIP_TRY(h->d_lut.alloc(cam_px, 64));  // +slack: bands are read in aligned 16-B vectors
    HIP_TRY(hipMemcpy(h->d_lut, lut.data(), cam_px * 4, hipMemcpyHostToDevice));
  }
  const size_t xm_cells = (size_t)xmap_h * cfg->xmap_width;
  {
    std::vector<int16_t> xt(xm_cells);
    for (int r = 0; r < xmap_h; ++r)
      for (int c = 0; c < cfg->xmap_width; ++c) xt[(size_t)c * xmap_h + r] = cfg->proj_x_map[(size_t)r * cfg->xmap_width + c];
    HIP_TRY(h->d_xmap.alloc(xm_cells, 64));
    HIP_TRY(hipMemcpy(h->d_xmap, xt.data(), xm_cells * 2, hipMemcpyHostToDevice));
  }
  if (cfg->disp_proj_mapxy_i16 && cfg->proj_width > 0 && cfg->proj_height > 0) {
    const size_t ppx = (size_t)cfg->proj_width * cfg->proj_height;
    std::vector<u32> pm(ppx);
    for (size_t i = 0; i < ppx; ++i)
      pm[i] = ((u32)(uint16_t)cfg->disp_proj_mapxy_i16[2 * i + 1] << 16) | (u32)(uint16_t)cfg->disp_proj_mapxy_i16[2 * i];
    HIP_TRY(h->d_pmap.alloc(ppx));
    h->plan_in_create().dims.has_pmap = true;
    HIP_TRY(hipMemcpy(h->d_pmap, pm.data(), ppx * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(h->d_zero16.alloc(256 / sizeof(ulonglong2)));
  HIP_TRY(hipMemset(h->d_zero16, 0, 256));
  HIP_TRY(h->d_dlut.alloc(65536));
  hipLaunchKernelGGL(k_build_dlut, dim3(65536 / BLOCK), dim3(BLOCK), 0, 0, h->d_dlut.get(), cfg->p03, cfg->z_near, cfg->z_far);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  DevTables& tb = h->tb;
  tb.dlut = h->d_dlut.get(); tb.lut = h->d_lut.get(); tb.xmap = h->d_xmap.get(); tb.pmap = h->d_pmap.get();
  tb.cam_w = cfg->cam_width; tb.cam_h = cfg->cam_height; tb.proj_w = cfg->proj_width; tb.proj_h = cfg->proj_height;
  tb.rect_w = cfg->rect_width; tb.rect_h = cfg->rect_height; tb.xmap_w = cfg->xmap_width; tb.xmap_h = xmap_h;
  tb.x_offset = cfg->x_offset; tb.t_px_scale = cfg->xmap_width - 1;
  tb.p03 = cfg->p03; tb.z_near = cfg->z_near; tb.z_far = cfg->z_far;
  RigPlan::Dims& d = h->plan_in_create().dims;  // the same dimensions for the rules
  d.cam_w = tb.cam_w; d.cam_h = tb.cam_h; d.proj_w = tb.proj_w; d.proj_h = tb.proj_h; d.rect_w = tb.rect_w; d.rect_h = tb.rect_h;
  d.xmap_w = tb.xmap_w; d.xmap_h = tb.xmap_h; d.x_offset = tb.x_offset; d.projector = cfg->view == XM_VIEW_PROJECTOR;
  return XM_OK;
}

// K2's static per-tile patch rectangles and per-pixel offsets, for each of its geometries, and which one the pipelined kernel takes
int build_k2_tables(xm_handle* h, CreateOpts& o) {
  const xm_config* cfg = &h->cfg;
  RigPlan& p = h->plan_in_create();
  if (!p.dims.has_pmap) return XM_OK;
  double mean_cells2 = 0.0;
  bool pipe_ok_g[3] = {false, false, false};
  for (int g = 0; g < 3; ++g) {
    const int ppt = 1 << g;
    const unsigned tiles_x = grid_for(cfg->proj_width, K2_TX * ppt), tiles_y = grid_for(cfg->proj_height, K2_TY);
    HIP_TRY(h->d_k2_tiles[g].alloc((size_t)tiles_x * tiles_y));
    HIP_TRY(h->d_k2_pix[g].alloc((size_t)cfg->proj_width * cfg->proj_height));
    if (g == 1) p.k2.has_tables = true;
    int4* const d_tiles = h->d_k2_tiles[g].get();
    u32* const d_pix = h->d_k2_pix[g].get();
    if (g == 0) hipLaunchKernelGGL(k_build_k2_tables<1>, dim3(tiles_x, tiles_y), dim3(K2_TX * K2_TY), 0, 0, h->tb, d_tiles, d_pix);
    else if (g == 1) hipLaunchKernelGGL(k_build_k2_tables<2>, dim3(tiles_x, tiles_y), dim3(K2_TX * K2_TY), 0, 0, h->tb, d_tiles, d_pix);
    else hipLaunchKernelGGL(k_build_k2_tables<4>, dim3(tiles_x, tiles_y), dim3(K2_TX * K2_TY), 0, 0, h->tb, d_tiles, d_pix);
    HIP_TRY(hipGetLastError());
    if (g > 0) {  // the pipelined kernel's u16 copy
      p.k2pipe.pix_stride = (cfg->proj_width + 7) & ~7;
      const size_t n16 = (size_t)p.k2pipe.pix_stride * cfg->proj_height;
      HIP_TRY(h->d_k2_pix16[g].alloc(n16, 16));
      p.k2pipe.has_pix16[g] = true;
      hipLaunchKernelGGL(k_k2_pix_to_u16, dim3(grid_for(n16, BLOCK)), dim3(BLOCK), 0, 0, d_pix, h->d_k2_pix16[g].get(), cfg->proj_width,
                         cfg->proj_height, p.k2pipe.pix_stride);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    // largest LDS patch any tile of this rig needs -> K2's dynamic LDS
    std::vector<int4> tiles((size_t)tiles_x * tiles_y);
    HIP_TRY(hipMemcpy(tiles.data(), d_tiles, tiles.size() * sizeof(int4), hipMemcpyDeviceToHost));
    int cap = 8;
    bool pipe_ok = (cfg->rect_height & 7) == 0;
    double cells = 0.0;
    if (g > 0) o.k2_tiles[g] = tiles;  // (build_k2_live)
    for (const int4& r : tiles) {
      if (r.z > 0) cap = std::max(cap, r.z * r.w);
      if (r.z > 0) cells += (double)r.z * r.w;
      pipe_ok = pipe_ok && k2_pipe_tile_ok(r);
    }
    if (g < 2)
      for (const int4& r : tiles) p.k2.patch_cols_max = r.z < 0 || p.k2.patch_cols_max < 0 ? -1 : std::max(p.k2.patch_cols_max, r.z);
    if (g == 1) {
      p.k2pipe.rig_ok = pipe_ok;
      mean_cells2 = cells / (double)std::max<size_t>(tiles.size(), 1);
    }
    pipe_ok_g[g] = pipe_ok;
    // Four pixels per thread when the 32 x 16-pixel tiles' patches are small against the tile (a projector image finer than
    // the rectified frame: < 2 patch cells per pixel): an item's fixed costs -- five barriers, the descriptor reads, the tile
    // arithmetic -- then weigh more than its patch, and half as many items carry the same pixels.  (Eight per thread --
    // 128 x 16 tiles -- was built and measured on the ESL-like rig: 94 VGPRs, five blocks per CU, K2 7.3-7.9 against 5.9-6.7 us
    // per frame; removed.)
    if (g == 2) {
      const bool small = mean_cells2 < 2.0 * (2 * K2_TX * K2_TY);
      const int want = o.k2_pipe_ppt ? atoi(o.k2_pipe_ppt) : small ? 4 : 2;
      p.k2pipe.g = p.k2pipe.rig_ok && want >= 4 && pipe_ok_g[2] ? 2 : 1;
    }
    p.k2.tile_cap[g] = std::min((cap + 7) & ~7, (int)K2_TILE_MAX);
  }
  h->tb.k2_tiles1 = h->d_k2_tiles[0].get();
  h->tb.k2_pix1 = h->d_k2_pix[0].get();
  h->tb.k2_tiles = h->d_k2_tiles[1].get();
  h->tb.k2_pix = h->d_k2_pix[1].get();
  return XM_OK;
}

// What the rig's tables allow: the compact (32-bit) key frame, the pipelined K2's LDS table, column tiles or owner tiles.  The
// arithmetic on the tables' extrema is classify_tables' (xm_plan.hpp); here: the switches, the device, and the one question only
// the device answers (k_cols_check: is cell(row, column) injective, does every live pair land inside the frame).
int classify_rig(xm_handle* h, const CreateOpts& o) {
  const xm_config* cfg = &h->cfg;
  RigPlan& p = h->plan_in_create();
  const int xmap_h = cfg->xmap_height;
  const size_t cam_px = (size_t)cfg->cam_width * cfg->cam_height, xm_cells = (size_t)xmap_h * cfg->xmap_width;
  const bool projector = p.dims.projector;
  const TableExtrema ex = table_extrema(cfg->cam_mapx_i16, cam_px, cfg->proj_x_map, xm_cells);
  const RigClass rc = classify_tables(ex, cfg->x_offset, projector, cfg->rect_height, o.k2_nlds_max);
  p.compact.key32_ok = rc.key32_ok && !(o.key32 && o.key32[0] == '0');
  p.k2pipe.nlds = rc.k2_pipe_nlds;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) p.dims.n_cus = prop.multiProcessorCount;
  // does the rig qualify for the column-tile K1?  (xmaps_k1cols.hpp)
  const char* ec = o.cols;
  const int xr_min = ex.xr_min;
  p.cols.xr_min = xr_min;
  p.cols.xr_max = ex.xr_max;
  bool injective = false;
  if (projector && rc.no_wrap && cfg->rect_width <= 65536) {
    DevMem<u32> d_dup;
    HIP_TRY(d_dup.alloc(2));
    HIP_TRY(hipMemset(d_dup, 0, 2 * sizeof(u32)));
    const int rows = std::min(xmap_h - 1, cfg->rect_height);
    if (rows > 0) hipLaunchKernelGGL(k_cols_check, dim3(rows), dim3(BLOCK), 0, 0, h->tb, xr_min, d_dup.get());
    u32 dup[2] = {1, 1};
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(dup, d_dup, sizeof dup, hipMemcpyDeviceToHost));
    injective = dup[0] == 0;  // every frame cell has at most one (row, time column) that can write it
    // every live pair has its cell inside the frame and every row an event can land in was looked at: no per-event cell test
    if (dup[1] == 0 && cfg->rect_height >= xmap_h - 1) p.cols.flags |= COLS_F_ALL_IN_FRAME;
  }
  p.cols.ok = injective && p.dims.has_pmap && !(ec && ec[0] == '0');
  p.cols.single = ec && ec[0] == '2';
  if (!injective && projector && rc.no_wrap && p.dims.has_pmap && !(ec && ec[0] == '0')) {
    // the reference's own calibration: several time columns per frame cell -> owner tiles (xmaps_k1own.hpp)
    p.cols.flags = 0;
    if (int rc_o = own_setup(h, p, cfg, xr_min)) return rc_o;
    p.cols.ok = p.cols.own_mode;
    // single-frame calls take the owner tiles too unless XM_COLS=1 says groups only (measured on ESL-like frames, four frames in
    // flight: 12.05 us per frame against 13.6 with the one-thread-per-event kernel and its 150 k divergent atomics)
    if (p.cols.own_mode && !(ec && ec[0] == '1')) p.cols.single = true;
  }
  // the compact key frame orders the writers of a cell by TILE only: two time columns of one tile that share a cell would be
  // ordered by their disparity bits -- it needs the same property (the 64-bit keys carry the full event index and do not)
  if (projector) p.compact.key32_ok = p.compact.key32_ok && injective;
  if (projector) {
    p.dims.key_cells = (size_t)cfg->rect_width * cfg->rect_height;
    p.dims.out_w = cfg->proj_width;
    p.dims.out_h = cfg->proj_height;
  } else {
    p.dims.key_cells = cam_px;
    p.dims.out_w = cfg->cam_width;
    p.dims.out_h = cfg->cam_height;
  }
  return XM_OK;
}

// K1 LDS windows and the widest column tile (size_k1_windows, xm_plan.hpp) into the plan
void apply_k1_windows(RigPlan& p, const CreateOpts& o) {
  const K1Windows w = size_k1_windows(p, o.k1_wx);
  p.k1.w_ts = w.w_ts;
  p.k1.w_x = w.w_x;
  p.k1.lds = w.lds;
  p.modes.k1_direct = w.k1_direct;
  p.cols.w_max = w.cols_w_max;
  p.cols.ok = w.cols_ok;
}

// The pipelined K2's live-slot masks (xm_k2_live.hpp), for both of its geometries.  Derived only where this handle's column-tile
// K1 is the sole writer of the frames that kernel reads: a group's K2 (launch_k2_batch<2> / <2, 2>) reads the slots' frame16,
// which k_scatter_cols / k_scatter_cols_batch write through cols_cell() with h->tb and the plan's cols.xr_min, lone frames and groups
// alike, and which nothing else stores into after the memset of create_slots.  Owner-tile rigs (another flush, a sheared frame),
// rigs without column tiles and "XM_K2_LIVE"=0 get all ones.  After classify_rig and size_k1_windows: both decide cols_ok.
int build_k2_live(xm_handle* h, const RigPlan& p, const CreateOpts& o) {
  const xm_config* cfg = &h->cfg;
  const bool derive = p.k2pipe.live && p.cols.ok && !p.cols.own_mode && p.k2pipe.rig_ok;
  for (int g = 1; g < 3; ++g) {
    const std::vector<int4>& tiles = o.k2_tiles[g];
    if (tiles.empty()) {  // (a rig without a projector map has no K2 tables at all; with them, the pipelined kernel must find its masks)
      if (p.k2.has_tables) return fail(XM_ERR_INVALID, "no tile records for the pipelined K2's live-slot masks (geometry %d)", g);
      continue;
    }
    std::vector<uint32_t> mask(tiles.size() * (size_t)K2L_WORDS, ~0u);
    if (derive) {
      static_assert(sizeof(K2LiveTile) == sizeof(int4), "xm_k2_live.hpp restates a record of k2_tiles");
      K2LiveRig rig;
      rig.xmap = cfg->proj_x_map; rig.xmap_w = cfg->xmap_width; rig.xmap_h = cfg->xmap_height;
      rig.x_offset = cfg->x_offset; rig.xr_min = p.cols.xr_min; rig.rect_w = cfg->rect_width; rig.rect_h = cfg->rect_height;
      rig.shear_m = h->tb.shear_m; rig.shear_bias = h->tb.shear_bias; rig.shear_extra = h->tb.shear_extra;
      std::vector<K2LiveTile> recs(tiles.size());
      for (size_t i = 0; i < tiles.size(); ++i) recs[i] = K2LiveTile{tiles[i].x, tiles[i].y, tiles[i].z, tiles[i].w};
      k2_live_mask(rig, recs.data(), recs.size(), mask);
      if (p.k2pipe.live_report) {
        const K2LiveStats st = k2_live_stats(rig, recs.data(), recs.size());
        fprintf(stderr, "[xm] K2 live quads, tiles of %d x 16 pixels: frame cells %.4f quads %.4f lines %.4f; loader slots %.4f, their lines %.4f\n",
                16 << g, st.cells, st.quads, st.lines, st.slot_quads, st.slot_lines);
      }
    }
    HIP_TRY(h->d_k2_live[g].alloc(mask.size() / 4));
    HIP_TRY(hipMemcpy(h->d_k2_live[g], mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  return XM_OK;
}

// the slot states, then per slot: its stream, key frames, flags; every slot reset on its own stream
int create_slots(xm_handle* h, const RigPlan& p, [[maybe_unused]] const CreateOpts& o) {
  const xm_config* cfg = &h->cfg;
  const int n_slots = cfg->n_slots;
#ifdef XM_ABLATE
  if (o.ablate) {
    int v = atoi(o.ablate);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(xm::g_ablate), &v, sizeof v));
  }
#endif
  HIP_TRY(h->d_states.alloc(n_slots + 1));
  HIP_TRY(hipMemset(h->d_states, 0, sizeof(SlotState) * (n_slots + 1)));  // host_flags = NULL
  // (a memset of device memory may return before it has run, and the slots' non-blocking streams do not wait for the default one:
  //  k_reset_slot below initialises the extrema slots in the same bytes -- the memset must have landed first)
  HIP_TRY(hipDeviceSynchronize());
  h->aux_st = h->d_states + n_slots;
  h->slots.resize(n_slots);
  for (int i = 0; i < n_slots; ++i) {
    Slot& s = h->slots[i];
    {
      // The slots' streams get their own hardware queues: HIP multiplexes all streams of one priority onto
      // GPU_MAX_HW_QUEUES (4) hardware queues, the application's default stream included, and how the eight slot streams
      // happened to interleave with it cost up to 17 % of the pipelined frame rate (first engine of a process: 64 Gev/s,
      // second: 75; tools/engine_order_probe.py).  Streams of another priority live in another queue pool.
      int lo = 0, hi = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = least, hi = greatest priority (numerically lowest)
      // one stream per hardware queue; slots beyond that share them (more streams than queues is where the runtime's
      // stream -> queue assignment starts to matter, and it only added buffering, no overlap)
      static const int hw_q = getenv("GPU_MAX_HW_QUEUES") && atoi(getenv("GPU_MAX_HW_QUEUES")) > 0 ? atoi(getenv("GPU_MAX_HW_QUEUES")) : 4;
      const int n_streams = hw_q;
      if (n_streams > 0 && i >= n_streams) s.stream.borrow(h->slots[i % n_streams].stream);
      else if (cfg->flags & XM_FLAG_DEFAULT_STREAMS) HIP_TRY(s.stream.create(hipStreamNonBlocking));
      else HIP_TRY(s.stream.create_with_priority(hipStreamNonBlocking, hi));
    }
    HIP_TRY(s.key_frame.alloc(p.dims.key_cells));
    if (p.compact.key32_ok) {
      HIP_TRY(s.key32.alloc(p.dims.key_cells));
      HIP_TRY(hipMemset(s.key32, 0, p.dims.key_cells * sizeof(u32)));
    }
    if (p.cols.ok) {  // cells no (row, column) pair maps to are never written: they stay 0 from here on
      const size_t bytes = cols_frame_bytes(frame16_cells(h->tb), cfg->xmap_width);  // frame + K0b's bounds and thresholds
      HIP_TRY(s.frame16.alloc((bytes + 1) / sizeof(uint16_t)));
      HIP_TRY(hipMemset(s.frame16, 0, bytes));
    }
    if (cfg->view == XM_VIEW_PROJECTOR && p.modes.k2_flags) HIP_TRY(s.dirty.alloc(((p.dims.key_cells + 15) >> 4) + 64));
    s.st = h->d_states + i;
    if (p.modes.try_sorted) {
      HIP_TRY(s.h_flags.alloc(16, hipHostMallocMapped));
      s.h_flags[0] = s.h_flags[1] = 0;
      u32* d_flags = s.h_flags.device_ptr();
      if (!d_flags) return fail(XM_ERR_HIP, "hipHostGetDevicePointer failed for a slot's flag words");
      HIP_TRY(hipMemcpy(&s.st->host_flags, &d_flags, sizeof d_flags, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_reset_slot, dim3(1024), dim3(BLOCK), 0, s.stream.get(), s.st, s.key_frame.get(), (u64)p.dims.key_cells, s.dirty.get());
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_reset_slot, dim3(1), dim3(BLOCK), 0, h->slots[0].stream.get(), h->aux_st, (u64*)nullptr, (u64)0,
                     (unsigned char*)nullptr);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// profile / fork / join events, then (once the slots' resets have run) what the multi-frame launches need: the distinct slot
// streams, their end-of-batch events, the descriptor ring
int create_batch_rings(xm_handle* h) {
  const int n_slots = h->cfg.n_slots;
  for (Event& e : h->prof_ev) HIP_TRY(e.create(hipEventDefault));
  HIP_TRY(h->fork_ev.create());
  h->join_ev.resize(n_slots);
  for (Event& e : h->join_ev) HIP_TRY(e.create());
  for (int i = 0; i < n_slots; ++i) h->slots[i].order.bind(h->slots[i].stream.get(), h->join_ev[i].get());
  for (int i = 0; i < n_slots; ++i) HIP_TRY(hipStreamSynchronize(h->slots[i].stream));
  for (int i = 0; i < n_slots; ++i) {
    bool seen = false;
    for (hipStream_t st : h->streams) seen = seen || st == h->slots[i].stream;
    if (!seen) h->streams.push_back(h->slots[i].stream);
  }
  h->batch_ev.resize(h->streams.size());
  h->batch_ev_next.assign(h->streams.size(), 0);
  for (auto& ring : h->batch_ev) {
    ring.resize(8);
    for (Event& e : ring) HIP_TRY(e.create());
  }
  HIP_TRY(h->h_descs.alloc((size_t)xm_handle::DESC_RING * n_slots, hipHostMallocDefault));
  HIP_TRY(h->d_descs.alloc((size_t)xm_handle::DESC_RING * n_slots));
  for (Event& e : h->desc_ev) HIP_TRY(e.create());
  for (Event& e : h->graph_ev) HIP_TRY(e.create());
  // (the memsets and table builders above ran on the default stream; the slots' streams are non-blocking: nothing of a first frame
  //  may overtake them)
  HIP_TRY(hipDeviceSynchronize());
  return XM_OK;
}

// launch workers: one per distinct slot stream (XM_FLAG_LAUNCH_WORKERS; off: launches stay in the calling thread)
void start_workers(xm_handle* h, const CreateOpts& o) {
  const bool want = o.workers ? o.workers[0] != '0' : (h->cfg.flags & XM_FLAG_LAUNCH_WORKERS) != 0;
  if (!want) return;
  std::vector<hipStream_t> seen;
  for (Slot& s : h->slots) {
    int w = -1;
    for (size_t k = 0; k < seen.size(); ++k)
      if (seen[k] == s.stream) w = (int)k;
    if (w < 0) {
      w = (int)seen.size();
      seen.push_back(s.stream);
      h->workers.emplace_back(new Worker());
    }
    s.worker = w;
  }
  for (auto& w : h->workers) w->th = std::thread(worker_main, h, w.get());
}

}  // namespace
