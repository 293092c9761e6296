// xm_host.hpp -- error reporting, device scratch, slots (their last-frame record, their redo record; their ordering record is
// xm_slot_order.hpp's, instantiated with HIP here), launch workers, the handle, launch / profile macros
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order)
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail(XM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                      __FILE__, __LINE__);                                          \
  } while (0)

// Variant switches for tests and experiments (XM_COLS, XM_K2_PIPE, XM_OWN_W, ...): set through xm_debug_option(), never read from
// the environment -- the library's behaviour does not depend on what the calling process happens to have exported.  Read when a
// handle (or an ingest) is created, except the few per-call measurement switches ("XM_SHARDED_KEYS", "XM_SHARD_PROFILE").
std::mutex g_opt_mu;
std::map<std::string, const std::string*> g_opts;  // name -> its current text, in g_opt_texts
std::deque<std::string> g_opt_texts;               // every text ever set: never erased, so a pointer handed out stays valid for the
                                                   // life of the process whatever another thread sets or removes meanwhile
const char* dbg_opt(const char* name) {
  std::lock_guard<std::mutex> lk(g_opt_mu);
  auto it = g_opts.find(name);
  return it == g_opts.end() ? nullptr : it->second->c_str();
}

struct DevBuf {  // grow-only device scratch: grows by a quarter beyond what was asked for
  DevMem<unsigned char> mem;
  void* p = nullptr;  // view of mem
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : mem(std::move(o.mem)), p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  int reserve(size_t bytes) {
    if (bytes <= cap) return XM_OK;
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY(mem.alloc(want));
    p = mem.get();
    cap = want;
    return XM_OK;
  }
};

struct HipOrderOps {  // SlotOrder's and ScratchOrder's calls on the HIP runtime
  static int rc(hipError_t e, const char* call) { return e == hipSuccess ? XM_OK : fail(XM_ERR_HIP, "%s failed: %s", call, hipGetErrorString(e)); }
  static hipEvent_t ev(void* e) { return static_cast<hipEvent_t>(e); }
  static hipStream_t st(void* s) { return static_cast<hipStream_t>(s); }
  static int record(void* e, void* s) { return rc(hipEventRecord(ev(e), st(s)), "hipEventRecord"); }
  static int wait(void* s, void* e) { return rc(hipStreamWaitEvent(st(s), ev(e), 0), "hipStreamWaitEvent"); }
  static int sync_event(void* e) { return rc(hipEventSynchronize(ev(e)), "hipEventSynchronize"); }
  static int sync_stream(void* s) { return rc(hipStreamSynchronize(st(s)), "hipStreamSynchronize"); }
  static int create(Event& e) { return rc(e.create(), "hipEventCreateWithFlags"); }  // (ScratchOrder's end-of-call event)
};

struct Slot {
  Stream stream;      // its own, or borrowed from an earlier slot (slots beyond the hardware-queue count share streams)
  int worker = -1;    // launch worker of this slot's stream (-1: none)
  SlotOrder<HipOrderOps> order;  // where the slot's last work ran: every use of its buffers on a stream goes through this first
  // What the slot's last frame was: written by note_enqueued, reset_slot and a graph replay; xm_graph_create copies it out and
  // back around its capture, whose launches run nothing
  struct Last {
    u32 host_tag = 0;  // mirrors st->tag_a after the enqueued work has run
    u32 api_tag = 0;   // the same tag as the API thread counts them (== host_tag once the workers are idle)
    bool sorted = false;
    bool key32 = false;  // it took a compact path (key32 or column tiles): a failure counts against it
    bool cols = false;   // ... the column tiles (K0b was launched in K0's place)
    uint64_t n = 0;
    int t_dtype = XM_T_INT64;  // how xm_last_frame_stats decodes t_min / t_max
  } last;
  // XM_FLAG_TRY_SORTED: pinned host words the kernels report to ([0] tag of the last frame whose shortcut failed, [1] tag of
  // the last frame whose K2 has started) and what is needed to redo the slot's last asynchronous frame on the general path
  PinnedMem<u32> h_flags;
  struct Prev {
    bool valid = false;
    EventsView ev;
    float* depth = nullptr;
    uint8_t* bgr = nullptr;
    bool check = false;           // the frame took the try-sorted shortcut: its verdict decides about a redo
    float* host_depth = nullptr;  // XM_MEM_HOST_PINNED: where the outputs are copied to
    uint8_t* host_bgr = nullptr;
    u32 tag = 0;
    hipStream_t stream = nullptr;  // the stream the frame's launches went to (the group's stream for xm_process_batch)
    void set(const EventsView& ev_, float* depth_, uint8_t* bgr_, float* host_depth_, uint8_t* host_bgr_, u32 tag_,
             hipStream_t stream_, bool check_) {
      valid = true, ev = ev_, depth = depth_, bgr = bgr_, host_depth = host_depth_, host_bgr = host_bgr_;
      tag = tag_, stream = stream_, check = check_;
    }
  } prev;
  DevMem<u64> key_frame;
  DevMem<u32> key32;               // compact key frame of the verified-sorted projector-view path (see key32_tag)
  u32 key32_valid_from = 0;        // tag of the frame before which key32 was last cleared: every key in it has a tag in
                                   // [valid_from, valid_from + 15), so the 4-bit tag field is unambiguous
  DevMem<uint16_t> frame16;        // plain u16 disparity frame of the column-tile path (xmaps_k1cols.hpp): rewritten by every frame
  DevMem<unsigned char> dirty;     // projector view: one flag byte per 128-byte line of key_frame
  SlotState* st = nullptr;  // device: a view into xm_handle::d_states
  // staging for XM_MEM_HOST calls
  DevBuf ev_x, ev_y, ev_t, ev_p, ev_aos, out_depth, out_bgr, dbg[5];
};

using HipScratchOrder = ScratchOrder<HipOrderOps, Event>;

// The time-surface entry (xm_api_surface.hpp): cloud tables + grow-only scratch, allocated by the first call.  One set per handle:
// `order` makes a call's launches wait for the previous call's before they touch it (xm_scratch_order.hpp).
struct SurfaceScratch {
  HipScratchOrder order;
  DevMem<float> mapx, mapy;           // float rectify maps [cam_h][cam_w] (xm_surface_set_cloud_tables)
  Mat4f q{};
  bool has_cloud_tables = false;
  DevBuf part1, part2, seg_cnt, seg_off, wave_oob, code, stats;  // device-side intermediates of a group
  DevBuf in, depth, cloud;                                         // staging of XM_MEM_HOST calls
};

// The frame -> time surface entry (xm_api_framesurface.hpp): grow-only scratch, allocated by the first call and ordered between
// calls like SurfaceScratch.  The winner maps and the accumulators are ALL ZERO between calls: their last readers leave them so
// (xmaps_framesurface.hpp).  `order` is noted dirty while a call's launches are being issued: a call that fails between its event
// pass and its last launch leaves the note, and the next call clears maps and accumulators before it uses them.
struct FrameSurfScratch {
  HipScratchOrder order;
  DevBuf maps, acc, stats;  // [<= FS_GROUP] winner maps / FsAcc; [frames of the call] FsStats
  DevBuf in, out;           // staging of XM_MEM_HOST calls
};

// The frame -> point cloud entry (xm_api_framecloud.hpp): its own cloud tables (handles of either view; the ingest's cloud stage
// reads the same) + grow-only scratch, ordered between calls like SurfaceScratch.  The accumulators are ALL ZERO between calls
// (k_fc_scan leaves them so); the dirty note as in FrameSurfScratch.  Codes, counts and offsets are rewritten by every call before
// it reads them.
struct FrameCloudScratch {
  HipScratchOrder order;
  DevMem<float> mapx, mapy;  // float rectify maps [cam_h][cam_w] (xm_cloud_set_tables)
  Mat4f q{};
  bool has_tables = false;
  DevBuf acc, code, cnt, off, stats;  // [<= FC_GROUP] FcAcc; per event u16; per 64 events uint2 / u32; [frames of the call] FcStats
  DevBuf in, out;                     // staging of XM_MEM_HOST calls
};

// The frame -> EVT 3.0 entry (xm_api_evt3enc.hpp): grow-only scratch, ordered between calls like SurfaceScratch.  Nothing of it is
// under a zero invariant: codes, counts, offsets and statistics are rewritten by every call before it reads them.
struct FrameRecordScratch {
  HipScratchOrder order;
  DevBuf code, cnt, off, stats;  // per event u16; per 64 events uint2 / u32; [frames of the call] EncStats
  DevBuf in, out;                // staging of XM_MEM_HOST calls
};

// ---- launch workers -------------------------------------------------------------------------------------------
// A kernel launch costs the calling thread ~2.7 us in the HIP runtime, three launches per frame; with the GPU at ~12 us per
// frame that single thread is what bounds the asynchronous device-pointer path (tools/only_kernel_eager.sh: 3.2 us per call
// + 2.75 us per launch, whatever the kernels do).  One worker thread per slot stream takes the launches: the API call only
// settles the slot's previous frame, assigns the frame to a slot and posts a job (5 instead of 11.5 us per call).  The frame
// rate does not change -- with the drain fix and own hardware queues the GPU is the bound -- so this is opt-in
// (XM_FLAG_LAUNCH_WORKERS) for hosts whose calling thread has other work to do.
struct Job {
  enum Kind : int { FRAME = 0, STOP = 1 };
  int kind = FRAME;
  int slot = 0;
  EventsView ev;
  float* depth = nullptr;
  uint8_t* bgr = nullptr;
  bool allow_sorted = true;
};

struct Worker {
  JobQueue<Job, 256> q;  // jobs in flight per stream (the producer waits when full)
  FirstError err;        // first failing return code of a job (reported by the next xm_sync)
  std::thread th;
};

}  // namespace

struct xm_handle {
  xm_config cfg{};
  // What xm_create decided about the rig (xm_plan.hpp): filled by its stages through plan_in_create(), read-only from
  // create_slots on.  Every path and shape rule reads this and nothing else of the handle.
  const RigPlan& plan() const { return plan_; }
  RigPlan& plan_in_create() { return plan_; }  // (xm_create and its stages up to apply_k1_windows, own_setup through them)

  // ---- owners of device memory, streams and events ----
  // the handle's own streams and events come before its buffers, which are therefore released first; a Slot orders its own
  // members the same way (every stream has been synchronised by xm_destroy before any of this runs: see xm_res.hpp)
  std::vector<Stream> gstreams;  // default-priority streams the hipGraph batches are captured on and launched from
  Event prof_ev[6];
  Event fork_ev;
  std::vector<Event> join_ev;
  Event k2_chain_ev[16];  // "XM_K2_CHAIN": created on first use (launch_k2_pipe)
  static constexpr int DESC_RING = 16;
  Event desc_ev[DESC_RING];  // recorded after the ring entry's upload: the entry may be rewritten once it fired
  // an event per (stream, ring entry) recorded at the end of a batch: eager work on a slot's own stream waits for it
  std::vector<std::vector<Event>> batch_ev;  // [distinct stream][8]
  Event graph_ev[8];  // end-of-replay events (ring), recorded on the graphs' origin stream
  DevTables tb{};      // what the kernels take by value: every pointer in it is a view of a table owned below
  DevMem<u32> d_lut;   // owner; tb.lut is the view
  DevMem<int16_t> d_xmap;
  DevMem<u32> d_pmap;
  DevMem<uint2> d_dlut;
  // K2's static per-tile / per-pixel tables for its two geometries: [0] one pixel per thread (16 x 16 tiles), [1] two (32 x 16)
  // ([2]: four pixels per thread, 64 x 16 tiles -- the pipelined kernel on rigs whose patches are small against the tile)
  DevMem<int4> d_k2_tiles[3];  // [g]: tiles of 16 << g pixels x 16 rows (owners; tb.k2_tiles1 / tb.k2_tiles view [0] / [1])
  DevMem<u32> d_k2_pix[3];     // (owners; tb.k2_pix1 / tb.k2_pix view [0] / [1])
  DevMem<uint16_t> d_k2_pix16[3];  // the pipelined K2's copy: u16, rows padded to plan().k2pipe.pix_stride
  // the pipelined K2's live-slot masks (xm_k2_live.hpp): per tile, wave and loader register the lanes whose quad some (row, time
  // column) pair of the column tiles can store into; all ones where that is not known (owner tiles, "XM_K2_LIVE"=0)
  DevMem<uint4> d_k2_live[3];
  DevMem<ulonglong2> d_zero16;  // 16 zero bytes: what K2 reads instead of a clean key-frame line
  DevMem<SlotState> d_states;  // n_slots + 1 (last = aux state for stage / shard calls)
  SlotState* aux_st = nullptr;  // view: the last entry of d_states
  DevMem<u64> d_shard_n;  // shards on the column tiles: the piece's own event count (device) + its FrameDesc behind it
  std::vector<Slot> slots;
  DevMem<u64> stage_frame;  // lazily allocated scratch for the stage API (max(rect, cam) cells)
  size_t stage_cells = 0;
  SurfaceScratch surf;      // xm_process_time_surfaces
  FrameSurfScratch fsurf;   // xm_frames_to_time_surfaces
  FrameCloudScratch fcloud; // xm_cloud_set_tables, xm_frames_to_point_clouds
  FrameRecordScratch frecord; // xm_frames_to_evt3_words
  std::vector<std::unique_ptr<Worker>> workers;  // one per slot stream (empty: launches happen in the calling thread)
  struct OwnSet {  // the device tables of the owner tiles' plan i (its scalars: plan().own[i])
    DevMem<uint16_t> d_xmap_own;
    DevMem<uint16_t> d_xmap_extra;
    DevMem<int4> d_tiles;
    DevMem<u32> d_bm;
    DevMem<u32> d_extra_cells;
  } own[OWN_PLANS];
  // multi-frame launches (xm_process_batch, batched hipGraphs, ingest): frame descriptors.  Eager batches stage them
  // through a ring of pinned host entries -> device entries (one memcpy per batch, stream-ordered before its kernels).
  PinnedMem<FrameDesc> h_descs;  // pinned  [DESC_RING][n_slots]
  DevMem<FrameDesc> d_descs;     // device  [DESC_RING][n_slots]
  std::vector<hipStream_t> streams;  // views: the distinct slot streams

  // ---- run-time state: what changes with the calls.  Written by the API thread (the one inside XM_ENTER) unless said otherwise ----
  int next_slot = 0;
  int last_slot = 0;
  bool capturing = false;     // inside xm_graph_create's stream capture (no host-side redo possible there)
  uint64_t sorted_fallbacks = 0;
  // XM_FLAG_ADAPTIVE_BATCH: asynchronous device-pointer frames are submitted as GROUPS (multi-frame launches) whenever the GPU
  // is still busy with earlier ones: a frame is launched at once when no group is in flight (an idle GPU -- the 60 Hz live
  // case -- never waits), otherwise it joins the pending list, which goes out as one group with the first call that finds the
  // GPU idle, when it holds ab_max = n_slots / 4 frames, or at the next synchronising call
  struct Deferred {
    EventsView ev;
    float* depth;
    uint8_t* bgr;
  };
  std::vector<Deferred> pending;
  int ab_max = 0;                                  // 0: off (set by xm_create, constant afterwards)
  hipEvent_t ab_inflight[4] = {nullptr, nullptr, nullptr, nullptr};  // views (events of batch_ev): end-of-group events of the last four groups submitted this way
  uint64_t ab_groups = 0, ab_frames = 0;
  bool desc_used[DESC_RING] = {};  // the descriptor ring
  int desc_next = 0;
  uint64_t batch_counter = 0;
  std::vector<int> batch_ev_next;
  unsigned graph_ev_next = 0;
  // API thread and, with XM_FLAG_LAUNCH_WORKERS, the launch threads (all pass through enqueue_frame): atomics
  std::atomic<uint64_t> path_counts[4] = {};  // frames enqueued per K1 variant (xm_path_counts)
  std::atomic<int> key32_score{0};  // raised by frames that failed the compact path, decays with every frame that took it
  std::atomic<int> key32_pause{0};  // frames for which the compact path stays switched off (it kept failing: sparse / noisy stream)
  // whichever thread launches a group's K2 (launch_k2_pipe)
  uint64_t k2_pipe_frames = 0;  // frames finished by the pipelined K2 since xm_create (xm_debug_k2_pipe_frames)
  std::mutex k2_chain_mu;       // "XM_K2_CHAIN": guards k2_chain_n and the order of the chained launches
  unsigned k2_chain_n = 0;
  // dynamic-LDS caps already raised on this handle's device, per kernel function (launch workers call concurrently: lds_mu)
  std::mutex lds_mu;
  std::vector<std::pair<const void*, size_t>> lds_caps;
  int ensure_lds(const void* fn, size_t bytes);

 private:
  RigPlan plan_;
};

struct xm_graph {
  xm_handle* h = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  std::vector<u32> frames_on_slot;
  int n_frames = 0;
  std::vector<FrameDesc> h_descs;  // batched capture: the frames' descriptors (static for the graph's lifetime)
  DevMem<FrameDesc> d_descs;
};

int flush_pending(xm_handle* h);  // XM_FLAG_ADAPTIVE_BATCH: submit the frames held back (defined beside xm_process_batch)

int xm_handle::ensure_lds(const void* fn, size_t bytes) {
  std::lock_guard<std::mutex> lk(lds_mu);
  for (auto& e : lds_caps)
    if (e.first == fn) {
      if (bytes <= e.second) return XM_OK;
      HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
      e.second = bytes;
      return XM_OK;
    }
  HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  lds_caps.emplace_back(fn, bytes);
  return XM_OK;
}

namespace {

// Profile mode (xm_profile_frame): the three hot-path launches go through hipExtLaunchKernelGGL, which ties a start
// and a stop event to the dispatch packet itself -- the same timestamps rocprofv3 --kernel-trace reports -- instead
// of bracketing the launch with hipEventRecord (which adds ~3-5 us of event processing to every interval).
struct ProfCtx {
  hipEvent_t start = nullptr, stop = nullptr;
};
thread_local ProfCtx g_prof;

#define XM_LAUNCH(kernel, grid, block, lds, stream, ...)                                                   \
  do {                                                                                                      \
    if (g_prof.start)                                                                                       \
      hipExtLaunchKernelGGL(kernel, grid, block, (std::uint32_t)(lds), stream, g_prof.start, g_prof.stop, 0u, __VA_ARGS__); \
    else                                                                                                    \
      hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                    \
  } while (0)

size_t t_size(int t_dtype) { return t_dtype == XM_T_FLOAT32 ? 4 : 8; }

int reset_slot(const RigPlan& pl, Slot& s, hipStream_t stream = nullptr) {
  if (!stream) stream = s.stream;
  hipLaunchKernelGGL(k_reset_slot, dim3(1024), dim3(BLOCK), 0, stream, s.st, s.key_frame, (u64)pl.dims.key_cells, s.dirty);
  HIP_TRY(hipGetLastError());
  if (s.key32) HIP_TRY(hipMemsetAsync(s.key32, 0, pl.dims.key_cells * sizeof(u32), stream));
  s.key32_valid_from = 0;
  s.last.host_tag = 0;
  s.last.api_tag = 0;
  if (s.h_flags) {  // tags start over: forget the verdicts of the old numbering (no frame of this slot is pending here)
    HIP_TRY(hipStreamSynchronize(stream));
    s.h_flags[0] = s.h_flags[1] = 0;
  }
  return XM_OK;
}

}  // namespace
