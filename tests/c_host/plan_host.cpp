// plan_host.cpp -- the path and launch-shape rules of x_maps_amd/csrc/host/xm_plan.hpp, built alone (tests/test_plan_cpu.py: g++,
// AddressSanitizer + UBSan).  Every expectation below is a literal worked out by hand from the rules as they stood before they
// moved into that header (k0_blocks .. launch_k2_pipe, cols_width .. frame_path, size_k1_windows, classify_rig); the two real
// rigs' plans are the field values xm_create built on an MI355X (profiles/plan_identity.md).  Prints "ok"; at the first mismatch
// the case's name, and exits 1.
#include <cstdio>
#include <cstdlib>

#include "../../include/xmaps.h"
#include "../../x_maps_amd/csrc/host/xm_plan.hpp"

using namespace xm;

#define EQ(name, got, want)                                                                                        \
  do {                                                                                                             \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                                 \
    if (g_ != w_) {                                                                                                \
      printf("MISMATCH %s: %s = %lld, expected %lld (line %d)\n", name, #got, g_, w_, __LINE__);                   \
      exit(1);                                                                                                     \
    }                                                                                                              \
  } while (0)

// event columns that are never read: addresses only
static const void* addr(uintptr_t a) { return reinterpret_cast<const void*>(a); }
static EventsView soa(size_t n, int t_dtype = XM_T_INT64, bool with_p = false) {
  EventsView e;
  e.x = (const uint16_t*)addr(0x10000), e.y = (const uint16_t*)addr(0x20000), e.t = addr(0x30000);
  e.p = with_p ? (const int16_t*)addr(0x40000) : nullptr;
  e.n = n, e.t_dtype = t_dtype, e.use_p = with_p;
  return e;
}
static EventsView aos(size_t n) {
  EventsView e;
  e.aos = addr(0x50000), e.n = n;
  return e;
}

// ---- the benchmark's two rigs, as xm_create builds them on an MI355X ----------------------------------------------------------
static RigPlan c1m() {  // C-1M, projector view (bench.py's flagship)
  RigPlan p;
  p.dims.cam_w = 640, p.dims.cam_h = 480, p.dims.proj_w = 640, p.dims.proj_h = 480, p.dims.rect_w = 1760, p.dims.rect_h = 1320;
  p.dims.xmap_w = 640, p.dims.xmap_h = 1320, p.dims.x_offset = 4242, p.dims.projector = true;
  p.dims.key_cells = 2323200, p.dims.out_w = 640, p.dims.out_h = 480, p.dims.n_cus = 256, p.dims.has_pmap = true;
  p.modes.try_sorted = true;
  p.k1.w_ts = 5, p.k1.w_x = 16, p.k1.lds = 47040;
  p.compact.key32_ok = true;
  p.cols.ok = true, p.cols.single = false, p.cols.xr_min = 100, p.cols.xr_max = 1402, p.cols.w_max = 5, p.cols.target = 3700;
  p.cols.flags = 2;
  p.k2.has_tables = true, p.k2.tile_cap[0] = 2800, p.k2.tile_cap[1] = 6080, p.k2.tile_cap[2] = 10192, p.k2.patch_cols_max = 95;
  p.k2pipe.rig_ok = true, p.k2pipe.g = 1, p.k2pipe.nlds = 1585, p.k2pipe.pix_stride = 640;
  p.k2pipe.has_pix16[1] = p.k2pipe.has_pix16[2] = true;
  return p;
}
static RigPlan esl() {  // the ESL-like owner-tile rig of benchmodes/esl.py
  RigPlan p;
  p.dims.cam_w = 640, p.dims.cam_h = 480, p.dims.proj_w = 1080, p.dims.proj_h = 1920, p.dims.rect_w = 1760, p.dims.rect_h = 1320;
  p.dims.xmap_w = 1080, p.dims.xmap_h = 1320, p.dims.x_offset = 4242, p.dims.projector = true;
  p.dims.key_cells = 2323200, p.dims.out_w = 1080, p.dims.out_h = 1920, p.dims.n_cus = 256, p.dims.has_pmap = true;
  p.modes.try_sorted = true;
  p.k1.w_ts = 5, p.k1.w_x = 16, p.k1.lds = 47040;
  p.compact.key32_ok = false;
  p.cols.ok = true, p.cols.single = true, p.cols.xr_min = -2049, p.cols.xr_max = 1690, p.cols.w_max = 5, p.cols.target = 3700;
  p.cols.flags = 2, p.cols.own_mode = true;
  const int own[3][12] = {// ok all_in w halo extras r_lo hr hrp rp grouped nxs_max extra_max
                          {1, 1, 20, 7, 1243, 0, 1319, 1320, 664, 1, 20, 752},
                          {1, 1, 16, 7, 1225, 0, 1319, 1320, 664, 1, 17, 876},
                          {1, 1, 8, 2, 1013, 0, 1319, 1320, 664, 0, 8, 756}};
  for (int i = 0; i < 3; ++i) {
    RigPlan::Own& o = p.own[i];
    o.ok = own[i][0], o.all_in = own[i][1], o.w = own[i][2], o.halo = own[i][3], o.extras = own[i][4], o.r_lo = own[i][5];
    o.hr = own[i][6], o.hrp = own[i][7], o.rp = own[i][8], o.grouped = own[i][9], o.nxs_max = own[i][10], o.extra_max = own[i][11];
  }
  p.k2.has_tables = true, p.k2.tile_cap[0] = 768, p.k2.tile_cap[1] = 1400, p.k2.tile_cap[2] = 2832, p.k2.patch_cols_max = 37;
  p.k2pipe.rig_ok = true, p.k2pipe.g = 2, p.k2pipe.nlds = 2048, p.k2pipe.pix_stride = 1080;
  p.k2pipe.has_pix16[1] = p.k2pipe.has_pix16[2] = true;
  return p;
}

struct WantPath {
  int per_frame, sorted, direct, cols_w, dev_redo, key32, kmode, counter;
};
static void path_is(const char* name, const FramePath& p, const WantPath& w) {
  EQ(name, p.per_frame, w.per_frame);
  EQ(name, p.sorted, w.sorted);
  EQ(name, p.direct, w.direct);
  EQ(name, p.cols_w, w.cols_w);
  EQ(name, p.dev_redo, w.dev_redo);
  EQ(name, p.key32, w.key32);
  EQ(name, p.kmode(), w.kmode);
  EQ(name, p.counter(), w.counter);
}
static FramePath group_path(const RigPlan& p, PathNow now, const EventsView& ev, int n, bool can_redo = false) {
  EventsView evs[60];
  for (int f = 0; f < n; ++f) evs[f] = ev;
  return frame_path(p, now, evs, n, true, true, can_redo);
}
static void k1_tiled_is(const char* name, const K1TiledShape& s, unsigned threads, unsigned gx, size_t lds) {
  EQ(name, s.threads, threads);
  EQ(name, s.gx, gx);
  EQ(name, s.lds, lds);
}
static void k2_tiled_is(const char* name, const K2TiledShape& s, int ppt, unsigned gx, unsigned gy, unsigned gz, size_t lds, int cap) {
  EQ(name, s.ppt, ppt);
  EQ(name, s.gx, gx);
  EQ(name, s.gy, gy);
  EQ(name, s.gz, gz);
  EQ(name, s.threads, 256);
  EQ(name, s.lds, lds);
  EQ(name, s.tile_cap, cap);
}
static void bounds_is(const char* name, const BoundsShape& s, int own, int split, unsigned nb, int lanes, unsigned gx) {
  EQ(name, s.own, own);
  EQ(name, s.split, split);
  EQ(name, s.nb, nb);
  EQ(name, s.lanes, lanes);
  EQ(name, s.gx, gx);
}
static void tiles_k1_is(const char* name, const TilesK1Shape& s, int own, int halo, int ept, unsigned gx, unsigned threads, size_t lds,
                        int flags) {
  EQ(name, s.own, own);
  EQ(name, s.halo, halo);
  EQ(name, s.ept, ept);
  EQ(name, s.gx, gx);
  EQ(name, s.threads, threads);
  EQ(name, s.lds, lds);
  EQ(name, s.flags, flags);
}
static void pipe_is(const char* name, const K2PipeShape& s, int g, int ppt, unsigned gx, unsigned gy, unsigned blocks, size_t lds,
                    unsigned magic, bool cs) {
  EQ(name, s.use, 1);
  EQ(name, s.g, g);
  EQ(name, s.ppt, ppt);
  EQ(name, s.gx, gx);
  EQ(name, s.gy, gy);
  EQ(name, s.blocks, blocks);
  EQ(name, s.lds, lds);
  EQ(name, s.gx_magic, magic);
  EQ(name, s.consecutive, cs);
}

// C-1M at the benchmark's density: 1 M events per frame, SoA, int64, 16-byte aligned columns
static void real_rig_c1m() {
  const RigPlan p = c1m();
  const EventsView ev = soa(1000000);
  const PathNow idle{}, capt{true, false}, paused{false, true}, capt_paused{true, true};
  EQ("c1m vec16", ev_vec16(ev), 1);
  EQ("c1m tiled", tiled_path(p, ev.n), 1);
  // a lone frame: no K0, event tiles onto the compact key frame, K2 at one pixel per thread
  path_is("c1m lone", frame_path(p, idle, &ev, 1, true), {0, 1, 0, 0, 0, 1, KM_KEY32, 2});
  k1_tiled_is("c1m lone K1", k1_tiled_shape(p, ev.n, ev.n, false), 512, 245, 47040);
  k2_tiled_is("c1m lone K2", k2_tiled_shape(p, 1), 1, 40, 30, 1, 5664, 2800);
  EQ("c1m lone K2 not pipelined", k2_pipe_shape(p, 1).use, 0);
  // groups: K0b, column tiles of 2 time columns, K2 tiled for 2 frames and pipelined from 8 on
  for (int n : {2, 8, 60}) {
    path_is("c1m group", group_path(p, idle, ev, n), {0, 1, 0, 2, 0, 0, KM_COLS, 3});
    EQ("c1m group n_mean", group_path(p, idle, ev, n).n_mean, 1000000);
  }
  bounds_is("c1m K0b", cols_bounds_shape(p, 2), -1, 0, 320, 16, 21);
  tiles_k1_is("c1m K1 cols", tiles_k1_shape(p, ev.n, 2, true, 0, 0), -1, 0, 8, 320, 512, 48640, 2);
  EQ("c1m group 2: K2 tiled", k2_pipe_shape(p, 2).use, 0);
  k2_tiled_is("c1m group 2 K2", k2_tiled_shape(p, 2), 2, 20, 30, 2, 12224, 6080);
  pipe_is("c1m group 8 K2", k2_pipe_shape(p, 8), 1, 2, 20, 30, 1536, 24904, 214748365u, false);
  pipe_is("c1m group 60 K2", k2_pipe_shape(p, 60), 1, 2, 20, 30, 1536, 24904, 214748365u, false);
  // a captured group of 60 with descriptors for the redo: column tiles, the redo decided on the device, and the redo's nodes
  for (PathNow now : {capt, capt_paused}) {
    path_is("c1m captured", group_path(p, now, ev, 60, true), {0, 0, 0, 2, 1, 0, KM_COLS, 3});
    path_is("c1m captured, no redo descriptors", group_path(p, now, ev, 60, false), {0, 0, 0, 0, 0, 0, KM_KEY64, 0});
  }
  tiles_k1_is("c1m captured K1", tiles_k1_shape(p, ev.n, 2, true, 1, 0), -1, 0, 8, 320, 512, 48640, 3);
  EQ("c1m redo K0", k0_blocks(1000000, true, 64), 64);
  k1_tiled_is("c1m redo K1", k1_tiled_shape(p, ev.n, ev.n, true), 512, 32, 47040);
  k2_tiled_is("c1m redo K2", k2_tiled_shape(p, 60, true), 2, 32, 1, 60, 12224, 6080);
  EQ("c1m general K0", k0_blocks(1000000, true, 1024), 245);
  // the compact paths paused: the sorted shortcut on the 64-bit keys
  path_is("c1m lone paused", frame_path(p, paused, &ev, 1, true), {0, 1, 0, 0, 0, 0, KM_KEY64, 1});
  for (int n : {2, 8, 60}) path_is("c1m group paused", group_path(p, paused, ev, n), {0, 1, 0, 0, 0, 0, KM_KEY64, 1});
  k1_tiled_is("c1m group paused K1", k1_tiled_shape(p, ev.n, ev.n, false), 512, 245, 47040);
  k2_tiled_is("c1m group 8 paused K2", k2_tiled_shape(p, 8), 2, 20, 30, 8, 12224, 6080);
}

// the ESL-like rig at the benchmark's density: 153 327 events per frame (the mean), EventCD records
static void real_rig_esl() {
  const RigPlan p = esl();
  const EventsView ev = aos(153327);
  const PathNow idle{}, capt{true, false}, paused{false, true}, capt_paused{true, true};
  EQ("esl not tiled", tiled_path(p, ev.n), 0);
  // a lone frame: K0b, owner tiles of 20 columns, K2 at two pixels per thread
  path_is("esl lone", frame_path(p, idle, &ev, 1, true), {0, 1, 0, 20, 0, 0, KM_COLS, 3});
  bounds_is("esl K0b", cols_bounds_shape(p, 20), 0, 7, 108, 32, 14);
  tiles_k1_is("esl K1 own", tiles_k1_shape(p, ev.n, 20, false, 0, 0), 0, 7, 8, 54, 512, 57456, 2);
  k2_tiled_is("esl lone K2", k2_tiled_shape(p, 1), 2, 34, 120, 1, 2864, 1400);
  // groups (too sparse for the event tiles: `direct` -- which the owner tiles then take precedence over)
  for (int n : {2, 8, 60}) path_is("esl group", group_path(p, idle, ev, n), {0, 1, 1, 20, 0, 0, KM_COLS, 3});
  EQ("esl group 2: K2 tiled", k2_pipe_shape(p, 2).use, 0);
  k2_tiled_is("esl group 2 K2", k2_tiled_shape(p, 2), 2, 34, 120, 2, 2864, 1400);
  pipe_is("esl group 8 K2", k2_pipe_shape(p, 8), 2, 4, 17, 120, 1536, 22112, 252645136u, true);
  pipe_is("esl group 60 K2", k2_pipe_shape(p, 60), 2, 4, 17, 120, 1536, 22112, 252645136u, true);
  // a captured group: sparse frames go K0 -> one thread per event -> tiled K2 on the 64-bit keys; no tiles, no device redo
  for (PathNow now : {capt, capt_paused}) path_is("esl captured", group_path(p, now, ev, 60, true), {0, 0, 1, 0, 0, 0, KM_KEY64, 0});
  EQ("esl captured K0", k0_blocks(153327, false, 1024), 150);
  EQ("esl captured K1", k1_direct_blocks(153327, false), 599);
  k2_tiled_is("esl captured K2", k2_tiled_shape(p, 60), 2, 34, 120, 60, 2864, 1400);
  // paused: no tiles
  path_is("esl lone paused", frame_path(p, paused, &ev, 1, true), {0, 1, 0, 0, 0, 0, KM_KEY64, 1});
  for (int n : {2, 8, 60}) path_is("esl group paused", group_path(p, paused, ev, n), {0, 1, 1, 0, 0, 0, KM_KEY64, 1});
  k2_tiled_is("esl group 8 paused K2", k2_tiled_shape(p, 8), 2, 34, 120, 8, 2864, 1400);
}

// a small plan whose K1 numbers come out round: a block may take n / 2 events (w_ts = 5, 7 time columns)
static RigPlan half_plan() {
  RigPlan p;
  p.dims.xmap_w = 7, p.dims.xmap_h = 64, p.dims.cam_w = 64, p.dims.cam_h = 64, p.dims.proj_w = 64, p.dims.proj_h = 64;
  p.dims.rect_w = 64, p.dims.rect_h = 64;
  p.k1.w_ts = 5, p.k1.w_x = 16, p.k1.lds = 1024;
  p.modes.try_sorted = true;
  return p;
}

static void k1_thresholds() {
  const RigPlan p = half_plan();
  EQ("k1_block_events at 1024", tiled_path(p, 2048), 1);
  EQ("k1_block_events below 1024", tiled_path(p, 2047), 0);
  RigPlan d = p;
  d.modes.k1_direct = true;
  EQ("k1_direct", tiled_path(d, 1000000), 0);
  EQ("k1_threads 512", k1_threads(p, 8192), 512);  // 512 x 8 = 4096 events fit
  EQ("k1_threads 256 below", k1_threads(p, 8191), 256);
  EQ("k1_threads 256", k1_threads(p, 4096), 256);
  EQ("k1_threads 128 below", k1_threads(p, 4095), 128);
  EQ("k1_threads floor", k1_threads(p, 100), 128);
  k1_tiled_is("k1 grid from the largest frame", k1_tiled_shape(p, 10000, 8192, false), 512, 3, 1024);
  k1_tiled_is("k1 redo cap below", k1_tiled_shape(p, 32 * 4096, 8192, true), 512, 32, 1024);
  k1_tiled_is("k1 redo cap", k1_tiled_shape(p, 32 * 4096 + 1, 8192, true), 512, 32, 1024);
  k1_tiled_is("k1 no cap", k1_tiled_shape(p, 32 * 4096 + 1, 8192, false), 512, 33, 1024);
  EQ("k1 direct blocks", k1_direct_blocks(257, false), 2);
  EQ("k1 direct blocks vec4", k1_direct_blocks(1025, true), 2);
  EQ("k1 direct blocks of nothing", k1_direct_blocks(0, false), 1);
  EQ("k0 blocks", k0_blocks(1024 * 1024 + 1, false, 1024), 1024);
  EQ("k0 blocks below the cap", k0_blocks(1024 * 1023, false, 1024), 1023);
  EQ("k0 vec2 blocks", k0_blocks(4097, true, 1024), 2);
  EventsView e = soa(10);
  EQ("k0_vec2", k0_vec2(e), 1);
  e.t = addr(0x30008);
  EQ("k0_vec2 misaligned t", k0_vec2(e), 0);
  EQ("ev_vec16 misaligned t", ev_vec16(e), 0);
  e = soa(10, XM_T_INT64, true);
  e.p = (const int16_t*)addr(0x40002);
  EQ("k0_vec2 misaligned p", k0_vec2(e), 0);
  EQ("ev_vec16 aos", ev_vec16(aos(10)), 0);
}

static void cols_thresholds() {
  RigPlan p = half_plan();
  p.cols.ok = true, p.cols.w_max = 1, p.dims.xmap_w = 1;  // one time column: n events per column
  EQ("cols_width per_col * W at 1024", cols_width(p, 1024), 1);
  EQ("cols_width per_col * W below", cols_width(p, 1023), 0);
  EQ("cols_width n == 0", cols_width(p, 0), 0);
  EQ("cols_width below 1 << 28", cols_width(p, (1ull << 28) - 1), 1);
  EQ("cols_width n at 1 << 28", cols_width(p, 1ull << 28), 0);
  const RigPlan c = c1m();
  EQ("cols_width C-1M", cols_width(c, 1000000), 2);
  EQ("cols_width clamps to w_max", cols_width(c, 192000), 5);  // 300 per column: 12 wanted
  EQ("cols_width sparse after clamping", cols_width(c, 100000), 0);
  RigPlan off = c;
  off.cols.ok = false;
  EQ("cols_width !ok", cols_width(off, 1000000), 0);
  // cols_threads: one time column, W = 1: a tile holds n events
  EQ("cols_threads 256", cols_threads(p, 1835, 1), 256);
  EQ("cols_threads past 256", cols_threads(p, 1836, 1), 512);
  EQ("cols_threads floor", cols_threads(p, 921, 1), 128);
  EQ("cols_threads above the floor", cols_threads(p, 922, 1), 192);
  EQ("cols_threads nearly empty", cols_threads(p, 10, 1), 128);
  bounds_is("K0b 16 lanes", cols_bounds_shape(c, 16), -1, 0, 40, 16, 3);
  bounds_is("K0b 32 lanes", cols_bounds_shape(c, 17), -1, 0, 38, 32, 5);
  EQ("cols lds pad", tiles_k1_shape(c, 1000000, 2, true, 0, 4096).lds, 48640 + 4096);
}

static void own_thresholds() {
  const RigPlan e = esl();
  EQ("own n at tiles * 128", cols_width(e, 54 * 128), 20);
  EQ("own n below tiles * 128", cols_width(e, 54 * 128 - 1), 0);
  EQ("own n at 1 << 28", cols_width(e, 1ull << 28), 0);
  // plan pick: columns per tile (own + halo) x events per column against COLS_EPT * COLS_MAX_THREADS = 4096
  RigPlan p = half_plan();
  p.dims.xmap_w = 1024;
  p.cols.ok = p.cols.own_mode = true;
  p.own[0].ok = true, p.own[0].w = 20, p.own[0].halo = 12;
  p.own[1].ok = true, p.own[1].w = 16, p.own[1].halo = 7;
  EQ("own pick at 4096", own_pick(p, 131072), 0);
  EQ("own pick past 4096", own_pick(p, 131073), 1);
  EQ("own width at 4096", cols_width(p, 131072), 20);
  EQ("own width past 4096", cols_width(p, 131073), 16);
  EQ("own index of the narrow plan", own_index(p, 16), 1);
  EQ("own index default", own_index(p, 20), 0);
  RigPlan one = p;
  one.own[1].ok = false;
  EQ("own pick, one plan", own_pick(one, 10000000), 0);
  // own_ept: four events per thread only when forced, for lane-strided loads, and where the tile then fits one pass
  EQ("own_ept default", own_ept(p, 1000, 20, false), 8);
  p.cols.own_ept_forced = 4;
  EQ("own_ept forced, fits", own_ept(p, 58514, 20, false), 4);
  EQ("own_ept forced, past one pass", own_ept(p, 58515, 20, false), 8);
  EQ("own_ept forced, 16-byte SoA columns", own_ept(p, 1000, 20, true), 8);
  // owner tiles' block: 32 columns x n / 1024 events
  EQ("own threads floor", cols_threads(p, 1024, 20, 8), 128);
  EQ("own threads cap", cols_threads(p, 1024 * 1024, 20, 8), 512);
  EQ("own threads ept 4", cols_threads(p, 32768, 20, 4), 320);  // 1024 per tile x 1.12 / 4 = 286 -> 320
  EQ("own lds, grouped", own_lds_bytes(e.own[0]), 57456);
  EQ("own lds, per row", own_lds_bytes(e.own[2]), 4 * 8 * 664 + 4 * 756 + 4 * 1320);
  bounds_is("own K0b narrow plan", cols_bounds_shape(e, 8), 2, 2, 270, 32, 34);
}

static void k2_thresholds() {
  RigPlan p = half_plan();
  p.dims.proj_w = 512, p.dims.proj_h = 512;  // 16 x 32 = 512 tiles of 32 x 16 pixels
  p.k2.tile_cap[0] = 800, p.k2.tile_cap[1] = 1600;
  EQ("k2_ppt below 1024 blocks", k2_ppt(p, 1), 1);
  EQ("k2_ppt at 1024 blocks", k2_ppt(p, 2), 2);
  p.k2.force_ppt = 1;
  EQ("k2_force_ppt 1", k2_ppt(p, 60), 1);
  p.k2.force_ppt = 2;
  EQ("k2_force_ppt 2", k2_ppt(p, 1), 2);
  p.k2.force_ppt = 3;
  EQ("k2_force_ppt 3 is ignored", k2_ppt(p, 1), 1);
  p.k2.force_ppt = 0;
  k2_tiled_is("k2 one pixel per thread", k2_tiled_shape(p, 1), 1, 32, 32, 1, (800 + 32) * 2, 800);
  k2_tiled_is("k2 two", k2_tiled_shape(p, 2), 2, 16, 32, 2, (1600 + 32) * 2, 1600);
  k2_tiled_is("k2 redo", k2_tiled_shape(p, 2, true), 2, 32, 1, 2, (1600 + 32) * 2, 1600);
  p.dims.proj_w = 64, p.dims.proj_h = 128;  // 2 x 8 = 16 tiles: fewer than the redo's 32 blocks
  k2_tiled_is("k2 redo, small frame", k2_tiled_shape(p, 2, true), 1, 32, 1, 2, (800 + 32) * 2, 800);
  p.dims.proj_h = 112;  // 4 x 7 = 28 tiles at one pixel per thread
  k2_tiled_is("k2 redo, below 32 tiles", k2_tiled_shape(p, 2, true), 1, 28, 1, 2, (800 + 32) * 2, 800);
}

static void k2_pipe_thresholds() {
  // 512 x 384 pixels: 16 x 24 = 384 items per frame; one block per CU: 256 blocks, the pipeline from 768 items on
  RigPlan p = c1m();
  p.dims.proj_w = 512, p.dims.proj_h = 384, p.k2.force_ppt = 2, p.k2pipe.per_cu_max = 1;
  EQ("pipe total below 3 * blocks", k2_pipe_shape(p, 1).use, 0);
  pipe_is("pipe total at 3 * blocks", k2_pipe_shape(p, 2), 1, 2, 16, 24, 256, 24904, 268435456u, false);
  p.k2pipe.force = true;
  pipe_is("pipe forced", k2_pipe_shape(p, 1), 1, 2, 16, 24, 256, 24904, 268435456u, false);
  p.k2pipe.blocks_cap = 100;
  EQ("pipe blocks cap", k2_pipe_shape(p, 1).blocks, 100);
  p.k2pipe.blocks_cap = 1000;
  EQ("pipe blocks cap above", k2_pipe_shape(p, 1).blocks, 256);
  RigPlan c = c1m();
  c.k2pipe.force = true;
  pipe_is("pipe forced, lone C-1M frame: a block per item", k2_pipe_shape(c, 1), 1, 2, 20, 30, 600, 24904, 214748365u, false);
  c.k2pipe.force = false;
  for (int off : {0, 1}) {  // the switches and the rig's conditions
    RigPlan q = c1m();
    if (off) q.k2pipe.on = false;
    EQ("pipe switch", k2_pipe_shape(q, 8).use, !off);
    q = c1m();
    if (off) q.k2pipe.rig_ok = false;
    EQ("pipe rig_ok", k2_pipe_shape(q, 8).use, !off);
    q = c1m();
    if (off) q.k2pipe.nlds = 0;
    EQ("pipe nlds", k2_pipe_shape(q, 8).use, !off);
  }
  // blocks per CU: the smaller of per_cu_max and what 160 KB of LDS hold (a block's LDS + 2 KB)
  c.k2pipe.per_cu_max = 6;
  EQ("per_cu at k2_per_cu_max = the LDS bound", k2_pipe_shape(c, 60).blocks, 1536);
  c.k2pipe.per_cu_max = 5;
  EQ("per_cu at k2_per_cu_max", k2_pipe_shape(c, 60).blocks, 1280);
  c.k2pipe.per_cu_max = 8, c.k2.tile_cap[1] = 4064, c.k2pipe.nlds = 1280;  // 18432 bytes: eight blocks fit exactly
  EQ("per_cu at the LDS bound: lds", k2_pipe_shape(c, 60).lds, 18432);
  EQ("per_cu at the LDS bound", k2_pipe_shape(c, 60).blocks, 2048);
  c.k2pipe.nlds = 1281;
  EQ("per_cu past the LDS bound", k2_pipe_shape(c, 60).blocks, 1792);
  c.k2pipe.per_cu_max = 0;
  EQ("per_cu at least one", k2_pipe_shape(c, 60).blocks, 256);
  // gx_magic
  RigPlan m = c1m();
  m.k2pipe.force = true;
  m.dims.proj_w = 32, m.dims.proj_h = 480;
  EQ("gx_magic, gx == 1", k2_pipe_shape(m, 8).gx_magic, 0);
  EQ("gx_magic, gx == 1: gx", k2_pipe_shape(m, 8).gx, 1);
  m.dims.proj_w = 33;
  EQ("gx_magic, gx == 2", k2_pipe_shape(m, 8).gx_magic, 2147483648u);
  m.dims.proj_w = 32767, m.dims.proj_h = 65520;  // 1024 x 4095 tiles: tile * gx stays below 2^32
  EQ("gx_magic below 2^32", k2_pipe_shape(m, 1).gx_magic, 4194304u);
  m.dims.proj_h = 65536;  // 1024 x 4096
  EQ("gx_magic at 2^32", k2_pipe_shape(m, 1).gx_magic, 0);
  // consecutive pixels: by default on the 64 x 16 tiles; forced either way; never without the u16 pixel table
  RigPlan e = esl();
  EQ("consecutive default, g = 1", k2_pipe_shape(c1m(), 8).consecutive, 0);
  EQ("consecutive default, g = 2", k2_pipe_shape(e, 8).consecutive, 1);
  e.k2pipe.consec = 0;
  EQ("consecutive forced off", k2_pipe_shape(e, 8).consecutive, 0);
  e.k2pipe.consec = 1, e.k2pipe.has_pix16[2] = false;
  EQ("consecutive without the table", k2_pipe_shape(e, 8).consecutive, 0);
  RigPlan f = c1m();
  f.k2pipe.consec = 1;
  EQ("consecutive forced on, g = 1", k2_pipe_shape(f, 8).consecutive, 1);
}

static void key32_thresholds() {
  const PathNow idle{};
  RigPlan cam = c1m();
  cam.dims.projector = false;
  EQ("key32 camera at CAM32_MAX_EVENTS", key32_path(cam, idle, soa(1048575), true), 1);
  EQ("key32 camera past CAM32_MAX_EVENTS", key32_path(cam, idle, soa(1048576), true), 0);
  const RigPlan p = c1m();
  EQ("key32 projector below 1 << 16 tiles", key32_path(p, idle, soa(67108863), true), 1);
  EQ("key32 projector at 1 << 16 tiles", key32_path(p, idle, soa(67108864), true), 0);
  EQ("key32 not sorted", key32_path(p, idle, soa(1000000), false), 0);
  EQ("key32 too sparse for the tiles", key32_path(p, idle, soa(100000), true), 0);
  RigPlan q = p;
  q.modes.k2_direct = true;
  EQ("key32 under k2_direct", key32_path(q, idle, soa(1000000), true), 0);
  q = p, q.modes.k2_flags = true;
  EQ("key32 under k2_flags", key32_path(q, idle, soa(1000000), true), 0);
  q = p, q.compact.key32_ok = false;
  EQ("key32 !key32_ok", key32_path(q, idle, soa(1000000), true), 0);
  q = p, q.modes.try_sorted = false, q.modes.time_sorted = true;
  EQ("key32 needs try_sorted", key32_path(q, idle, soa(1000000), true), 0);
  EQ("key32 capturing", key32_path(p, PathNow{true, false}, soa(1000000), true), 0);
  EQ("key32 compact_paused", key32_path(p, PathNow{false, true}, soa(1000000), true), 0);
  // sorted_path
  EQ("sorted try_sorted", sorted_path(p, idle, soa(10)), 1);
  EQ("sorted capturing", sorted_path(p, PathNow{true, false}, soa(10)), 0);
  EQ("sorted time_sorted while capturing", sorted_path(q, PathNow{true, false}, soa(10)), 1);
  EQ("sorted polarity column", sorted_path(p, idle, soa(10, XM_T_INT64, true)), 0);
  EQ("sorted empty frame", sorted_path(p, idle, soa(0)), 0);
}

static void frame_path_cases() {
  const PathNow idle{}, capt{true, false};
  const RigPlan p = c1m();
  {  // a group with mixed AoS and SoA layout: no tiles
    const EventsView evs[2] = {soa(1000000), aos(1000000)};
    path_is("mixed layouts", frame_path(p, idle, evs, 2, true, true), {0, 1, 0, 0, 0, 1, KM_KEY32, 2});
    const EventsView same[2] = {aos(1000000), aos(1000000)};
    path_is("one layout", frame_path(p, idle, same, 2, true, true), {0, 1, 0, 2, 0, 0, KM_COLS, 3});
  }
  {  // one frame with a polarity column: not sorted, no tiles
    const EventsView evs[2] = {soa(1000000), soa(1000000, XM_T_INT64, true)};
    path_is("a polarity column", frame_path(p, idle, evs, 2, true, true), {0, 0, 0, 0, 0, 0, KM_KEY64, 0});
  }
  {  // one float64 frame in an otherwise int64 group: sorted, the compact key frame, no tiles
    const EventsView evs[3] = {soa(1000000), soa(1000000, XM_T_FLOAT64), soa(1000000)};
    path_is("a float64 frame", frame_path(p, idle, evs, 3, true, true), {0, 1, 0, 0, 0, 1, KM_KEY32, 2});
  }
  {  // allow_sorted = false: the general path
    const EventsView ev = soa(1000000);
    path_is("allow_sorted off", frame_path(p, idle, &ev, 1, false), {0, 0, 0, 0, 0, 0, KM_KEY64, 0});
    path_is("allow_sorted off, group", frame_path(p, idle, &ev, 1, false, true), {0, 0, 0, 0, 0, 0, KM_KEY64, 0});
  }
  {  // per_frame under k2_direct
    RigPlan q = p;
    q.modes.k2_direct = true;
    EQ("per_frame under k2_direct", group_path(q, idle, soa(1000000), 8).per_frame, 1);
    q = p, q.modes.k2_flags = true;
    EQ("per_frame under k2_flags", group_path(q, idle, soa(1000000), 8).per_frame, 1);
  }
  {  // direct for a sparse group of 2, and not for a group of 1
    RigPlan q = esl();
    q.cols.ok = false;
    path_is("sparse group of 2", group_path(q, idle, aos(153327), 2), {0, 1, 1, 0, 0, 0, KM_KEY64, 1});
    EQ("sparse group of 1: per_frame", group_path(q, idle, aos(153327), 1).per_frame, 1);
    EQ("sparse group of 1: not direct", group_path(q, idle, aos(153327), 1).direct, 0);
    RigPlan no_tables = q;
    no_tables.k2.has_tables = false;
    EQ("sparse group without K2 tables", group_path(no_tables, idle, aos(153327), 2).per_frame, 1);
    no_tables.dims.projector = false;
    EQ("sparse group, camera view", group_path(no_tables, idle, aos(153327), 2).direct, 1);
    // p.n_max at 1 << 31 (k1_direct: no frame is dense enough for the tiles)
    q.modes.k1_direct = true;
    const EventsView below[2] = {aos(1000), aos((1ull << 31) - 1)}, at[2] = {aos(1000), aos(1ull << 31)};
    EQ("n_max below 1 << 31", frame_path(q, idle, below, 2, true, true).direct, 1);
    EQ("n_max at 1 << 31: not direct", frame_path(q, idle, at, 2, true, true).direct, 0);
    EQ("n_max at 1 << 31: per_frame", frame_path(q, idle, at, 2, true, true).per_frame, 1);
    EQ("n_max", frame_path(q, idle, at, 2, true, true).n_max, 1ull << 31);
    EQ("n_mean", frame_path(q, idle, at, 2, true, true).n_mean, ((1ull << 31) + 1000) / 2);
  }
  {  // dev_redo only with at least 2 frames and can_redo
    EQ("dev_redo", group_path(p, capt, soa(1000000), 2, true).dev_redo, 1);
    EQ("dev_redo width", group_path(p, capt, soa(1000000), 2, true).cols_w, 2);
    EQ("dev_redo needs 2 frames", group_path(p, capt, soa(1000000), 1, true).dev_redo, 0);
    EQ("dev_redo needs 2 frames: no tiles", group_path(p, capt, soa(1000000), 1, true).cols_w, 0);
    EQ("dev_redo needs can_redo", group_path(p, capt, soa(1000000), 2, false).cols_w, 0);
    EQ("dev_redo only while capturing", group_path(p, idle, soa(1000000), 2, true).dev_redo, 0);
  }
  {  // cols_single off for a lone frame
    const EventsView ev = soa(1000000);
    EQ("cols_single off", frame_path(p, idle, &ev, 1, true).cols_w, 0);
    RigPlan q = p;
    q.cols.single = true;
    path_is("cols_single on", frame_path(q, idle, &ev, 1, true), {0, 1, 0, 2, 0, 0, KM_COLS, 3});
  }
  {  // vec16: every SoA frame's columns
    EventsView evs[2] = {soa(1000000), soa(1000000)};
    EQ("vec16", frame_path(p, idle, evs, 2, true, true).vec16, 1);
    evs[1].x = (const uint16_t*)addr(0x10002);
    EQ("vec16 off", frame_path(p, idle, evs, 2, true, true).vec16, 0);
    EQ("empty group", frame_path(p, idle, evs, 0, true, true).sorted, 0);
  }
}

static void create_arithmetic() {
  {  // size_k1_windows: C-1M
    RigPlan p = c1m();
    p.k1 = RigPlan::K1{}, p.cols.w_max = 0;
    const K1Windows w = size_k1_windows(p, 16);
    EQ("C-1M w_ts", w.w_ts, 5);
    EQ("C-1M w_x", w.w_x, 16);
    EQ("C-1M k1 lds", w.lds, 47040);
    EQ("C-1M k1_direct", w.k1_direct, 0);
    EQ("C-1M cols_w_max", w.cols_w_max, 5);
    EQ("C-1M cols_ok", w.cols_ok, 1);
    EQ("C-1M cols lds at w_max", cols_lds_bytes_at(16, 480, 1320, 5), 16 * 4525);
    EQ("C-1M cols lds past w_max", cols_lds_bytes_at(16, 480, 1320, 6), 16 * 5020);  // > 76 KB = 16 * 4864
  }
  {  // tall X-map: w_ts shrinks to 3
    RigPlan p = c1m();
    p.dims.xmap_h = 4000;
    const K1Windows w = size_k1_windows(p, 16);
    EQ("tall X-map w_ts", w.w_ts, 3);
    EQ("tall X-map w_x", w.w_x, 16);
    EQ("tall X-map lds", w.lds, 16 * 4630);
    EQ("tall X-map cols_w_max", w.cols_w_max, 1);
    EQ("tall X-map cols_ok", w.cols_ok, 1);
  }
  {  // tall camera: w_x halves twice
    RigPlan p = c1m();
    p.dims.cam_h = 4000, p.dims.xmap_h = 100;
    const K1Windows w = size_k1_windows(p, 16);
    EQ("tall camera w_ts", w.w_ts, 5);
    EQ("tall camera w_x", w.w_x, 4);
    EQ("tall camera lds", w.lds, 16 * 4258);
  }
  {  // both too tall: k1_direct, and the column tiles go with it
    RigPlan p = c1m();
    p.dims.cam_h = 30000, p.dims.xmap_h = 30000;
    const K1Windows w = size_k1_windows(p, 16);
    EQ("too tall k1_direct", w.k1_direct, 1);
    EQ("too tall w_ts", w.w_ts, 0);
    EQ("too tall lds", w.lds, 0);
    EQ("too tall cols_ok", w.cols_ok, 0);
    p.cols.own_mode = true;
    EQ("too tall, owner tiles stay", size_k1_windows(p, 16).cols_ok, 1);
  }
  {  // camera view: the slots are the LUT band's pixels
    RigPlan p = c1m();
    p.dims.projector = false;
    EQ("camera view lds", size_k1_windows(p, 16).lds, 47040);
    RigPlan d = c1m();
    d.modes.k1_direct = true;  // the switch: windows are still sized, no column tiles
    EQ("k1_direct switch keeps", size_k1_windows(d, 16).k1_direct, 1);
    EQ("k1_direct switch w_ts", size_k1_windows(d, 16).w_ts, 5);
    EQ("k1_direct switch cols_ok", size_k1_windows(d, 16).cols_ok, 0);
  }
  {  // the tables' extrema, once
    const int16_t mapx[4] = {100, 1402, 700, 101}, xmap[3] = {-5, 5926, 0};
    const TableExtrema e = table_extrema(mapx, 4, xmap, 3);
    EQ("xr_min", e.xr_min, 100);
    EQ("xr_max", e.xr_max, 1402);
    EQ("xp_min", e.xp_min, -5);
    EQ("xp_max", e.xp_max, 5926);
    const RigClass c = classify_tables(e, 4242, true, 1320, 2048);
    EQ("C-1M-like max_disp", c.max_disp, 1584);
    EQ("C-1M-like nlds", c.k2_pipe_nlds, 1585);
    EQ("C-1M-like key32", c.key32_ok, 1);
    EQ("C-1M-like no_wrap", c.no_wrap, 1);
    EQ("xr_min alone", table_extrema(mapx, 4, xmap, 0).xr_min, 100);
  }
  auto ext = [](int xr_min, int xr_max, int xp_min, int xp_max) {
    TableExtrema e;
    e.xr_min = xr_min, e.xr_max = xr_max, e.xp_min = xp_min, e.xp_max = xp_max;
    return e;
  };
  EQ("max_disp 4095", classify_tables(ext(0, 10, 0, 4095), 0, true, 1320, 2048).key32_ok, 1);
  EQ("max_disp 4096", classify_tables(ext(0, 10, 0, 4096), 0, true, 1320, 2048).key32_ok, 0);
  EQ("max_disp from a negative LUT entry", classify_tables(ext(-2049, 10, 0, 100), 4242, true, 1320, 2048).max_disp, -2093);
  EQ("max_disp, xp never below 0", classify_tables(ext(-5000, 10, -7, -3), 0, true, 1320, 2048).max_disp, 5000);
  EQ("nlds capped", classify_tables(ext(0, 10, 0, 5000), 0, true, 1320, 2048).k2_pipe_nlds, 2048);
  EQ("nlds at least one", classify_tables(ext(100, 200, 0, 10), 0, true, 1320, 2048).k2_pipe_nlds, 1);
  EQ("rect_h % 4, projector", classify_tables(ext(0, 10, 0, 100), 0, true, 1322, 2048).key32_ok, 0);
  EQ("rect_h % 4, camera", classify_tables(ext(0, 10, 0, 100), 0, false, 1322, 2048).key32_ok, 1);
  EQ("no_wrap at 32767", classify_tables(ext(0, 10, 0, 32767), 0, true, 1320, 2048).no_wrap, 1);
  EQ("wrap past 32767", classify_tables(ext(-1, 10, 0, 32767), 0, true, 1320, 2048).no_wrap, 0);
  EQ("no_wrap at -32768", classify_tables(ext(0, 32767, -1, 10), 0, true, 1320, 2048).no_wrap, 1);
  EQ("wrap past -32768", classify_tables(ext(0, 32767, -2, 10), 0, true, 1320, 2048).no_wrap, 0);
}

// The dynamic LDS of the five kernels whose layout the host sizes, at shapes where each rounding term of a layout bites.  The
// literals are what the host formulas gave while they still restated the kernels' carve-ups (evaluated from that text).
static void lds_layouts() {
  // column tiles: w_x * cam_h = 1443 (not a multiple of 4); W * xmap_h = 3963 (odd), 1324 (a multiple of 4, not of 8), 2644 likewise
  EQ("cols lds, odd bands", cols_lds_bytes_at(3, 481, 1321, 3), 31648);
  EQ("cols lds, X-map band 4 mod 8", cols_lds_bytes_at(3, 481, 1324, 1), 15808);
  EQ("cols lds, LUT band whole quads, X-map band 4 mod 8", cols_lds_bytes_at(2, 482, 1322, 2), 21808);
  EQ("cols lds, one cell", cols_lds_bytes_at(1, 1, 1, 1), 2128);
  EQ("cols lds, C-1M tile", cols_lds_bytes_at(16, 480, 1320, 2), 48640);
  // owner tiles: the table's pad to 4 words -- grouped: 2 * hrp / 8 = 6 -> 8, 10 -> 12, 330 -> 332; per row: 13 -> 16, 1320 as it is
  EQ("own lds, grouped 6 words", own_plan_lds_bytes(17, 24, 24, 5, true), 1684);
  EQ("own lds, grouped 10 words", own_plan_lds_bytes(17, 24, 40, 5, true), 1700);
  EQ("own lds, grouped 330 words", own_plan_lds_bytes(17, 24, 1320, 5, true), 2980);
  EQ("own lds, per row 13 words", own_plan_lds_bytes(8, 16, 13, 7, false), 604);
  EQ("own lds, per row 16 words", own_plan_lds_bytes(8, 16, 16, 7, false), 604);
  EQ("own lds, per row 1320 words", own_plan_lds_bytes(8, 16, 1320, 7, false), 5820);
  // K2 tiled and pipelined: tile_cap + 32 = 2836 (4 mod 8), 6113 (odd), 10224 (a multiple of 8)
  RigPlan p;
  p.k2.tile_cap[0] = 2804, p.k2.tile_cap[1] = 6081, p.k2.tile_cap[2] = 10192, p.k2pipe.nlds = 1585;
  EQ("k2 lds, 4 mod 8", k2_lds_bytes(p, 1), 5672);
  EQ("k2 lds, odd", k2_lds_bytes(p, 2), 12226);
  EQ("k2 pipe lds, 4 mod 8", k2_pipe_lds_bytes(p, 0), 18360);
  EQ("k2 pipe lds, odd", k2_pipe_lds_bytes(p, 1), 24920);
  EQ("k2 pipe lds, a multiple of 8", k2_pipe_lds_bytes(p, 2), 33128);
  p.k2.tile_cap[1] = 6084, p.k2pipe.nlds = 3;
  EQ("k2 pipe lds, small table", k2_pipe_lds_bytes(p, 1), 12264);
  // tiled K1: the region the slots and the LUT band share takes the larger of the two
  struct Case {
    const char* name;
    bool projector;
    int cam_h, xmap_h, k1_wx, w_ts, w_x;
    size_t lds;
    int cols_w_max;
  };
  const Case cases[] = {{"projector view, LUT band larger", true, 481, 1321, 16, 5, 16, 47120, 5},   // 1652 slots' quads < 1989
                        {"projector view, slots larger", true, 101, 1321, 16, 5, 16, 41728, 8},      // 1652 > 469
                        {"projector view, slots larger, narrow LUT", true, 99, 2001, 3, 5, 3, 62128, 6},
                        {"camera view: always the LUT band", false, 481, 1321, 16, 5, 16, 47120, 5},
                        {"camera view, short X-map", false, 483, 101, 16, 5, 16, 35056, 16}};
  for (const Case& c : cases) {
    RigPlan r;
    r.dims.cam_w = 640, r.dims.cam_h = c.cam_h, r.dims.xmap_w = 640, r.dims.xmap_h = c.xmap_h, r.dims.projector = c.projector;
    r.cols.ok = true;
    const K1Windows w = size_k1_windows(r, c.k1_wx);
    EQ(c.name, w.w_ts, c.w_ts);
    EQ(c.name, w.w_x, c.w_x);
    EQ(c.name, w.lds, c.lds);
    EQ(c.name, w.k1_direct, 0);
    EQ(c.name, w.cols_w_max, c.cols_w_max);
  }
}

int main() {
  lds_layouts();
  real_rig_c1m();
  real_rig_esl();
  k1_thresholds();
  cols_thresholds();
  own_thresholds();
  k2_thresholds();
  k2_pipe_thresholds();
  key32_thresholds();
  frame_path_cases();
  create_arithmetic();
  // the frame kernels without tiles
  const RigPlan p = c1m();
  EQ("cam32 gx", cam32_gx(p), 20);
  EQ("cam32 gy", cam32_gy(p), 15);
  EQ("pixel blocks", pixel_blocks(cam_pixels(p)), 1200);
  printf("ok\n");
  return 0;
}
