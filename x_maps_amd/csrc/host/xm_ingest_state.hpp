// xm_ingest_state.hpp -- device-side ingest (N2): its host state, one part per owning thread, and what the threads hand each other
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; see that file for the order.  The
// ingest's files: this one; xm_ingest_out.hpp -- the out side and the frame pool; xm_ingest_launch.hpp -- the launch and copy
// sides; xm_api_ingest.hpp -- the C entry points)
#pragma once

// ---- N2: device-side ingest ----------------------------------------------------------------------------------------
// Who does what:
//   caller thread   xm_ingest_push*: stages the packet (pageable memory: one memcpy into a pinned ring entry) and posts a job
//   copy thread     per packet: what brings it to the device -- the H2D copy of records on the copy stream, or the H2D + the three
//                   decode launches of a RAW chunk on the decoder's stream -- and the event behind it; forwards every job, in order
//   launch thread   per packet: one stream-wait, then k_ing_count / k_ing_append / k_ing_segment on the INGEST stream.
//                   k_ing_segment leaves a 16-byte verdict in pinned memory (did the packet cut a frame, of how many events);
//                   the thread reads the verdicts in packet order and, for a packet that cut a frame, launches K0 -> K1 -> K2 ->
//                   statistics on the FRAME stream with exact grids.
//   out thread      per cut frame: the DMA copies of its outputs (one of three device frames -> the pinned result ring, in 4 MB
//                   pieces) and its sequence number on the OUT stream, behind the frame's K2 -- beside the next frame's kernels.
//                   (A thread of its own because enqueuing a copy behind a running one can block the caller.)
//   xm_ingest_poll  reads the result ring's sequence numbers (pinned memory, no API call)
// Every hand-over between them is a JobQueue (xm_queue.hpp): caller -> copy thread -> launch thread -> out thread.
// The ingest stream may be `ahead` packets in front of the verdict the thread has handled last (0 on small rings: each packet's
// verdict is awaited before the next is issued); k_ing_segment's room rule keeps that many packets' worth of the ring free, and
// the ingest stream waits (on the device) for K1 of a frame -- for a frame under a frame event filter: for the filter stage's last
// read of it -- before anything issued after it appends.  XM_INGEST_NO_LAUNCH_THREAD:
// the caller does the work of all three threads inside xm_ingest_push* (and waits for each packet's verdict).

namespace {

constexpr int ING_NOUT = 3;    // device-side output frames (K2 writes them, a DMA copy takes them to the pinned result ring)
constexpr int ING_STAGE = 16;  // staging (pinned host -> device), a small ring so that the copy of packet k+1 does not wait for packet k's kernels
constexpr int ING_VRING = 64;  // per-packet rings: frame descriptor, frame info (device), verdict (pinned host)

inline double ingest_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The ingest's four streams (ingest / frame / copy / out) come from ONE set per device and process: created by the first ingest,
// lent to one ingest at a time (another one that is alive at the same time makes its own), never destroyed.  Which hardware
// resources a set of streams lands on decides how well the ingest's stages overlap, and it depends on what the process created
// before: the FIRST set runs a stream of records packets at 1055-1105 Mev/s, a set created after another one was destroyed at
// 680-750 (the other way round for one-frame-per-packet EVT 3.0 chunks: 840-890 against 1100-1200) -- measured, not understood
// (profiles/r04_ingest.md section 5).  Keeping the first set makes every ingest of the process behave like its first one.
struct IngestStreamSet {
  hipStream_t s[4] = {nullptr, nullptr, nullptr, nullptr};  // (raw on purpose: created once, never destroyed -- see above)
  const void* lent_to = nullptr;
};
std::mutex g_ing_sets_mu;
std::map<int, IngestStreamSet> g_ing_sets;

// borrow the device's set for `who`: its four streams (created by the borrower where they do not exist yet), or NULL when somebody has it
hipStream_t* ingest_stream_set(int device, const void* who) {
  std::lock_guard<std::mutex> lk(g_ing_sets_mu);
  IngestStreamSet& e = g_ing_sets[device];
  if (e.lent_to) return nullptr;
  e.lent_to = who;
  return e.s;
}

void ingest_stream_release(int device, const void* who) {  // (nothing happens when `who` did not have the set)
  std::lock_guard<std::mutex> lk(g_ing_sets_mu);
  IngestStreamSet& e = g_ing_sets[device];
  if (e.lent_to == who) e.lent_to = nullptr;
}

// ---- what the threads hand each other ----
enum class JobKind : int {
  records,     // a packet of records in pinned host memory
  words,       // a chunk of EVT 3.0 / 2.0 words, decoded on the device
  stop,        // the thread forwards it and leaves
  on_device,   // records that are in d_pkt[k] already (a chunk the caller decoded itself: xm_ingest_push_evt3 with n_events)
  flush,       // every verdict in, every frame's kernels launched and run
  count_only,  // nothing arrived (the copy side failed): the launch side only counts the job
  set_filter,  // the frame event filter for the frames cut by the packets behind this job (xm_ingest_set_frame_filter)
  set_surface, // the surface stage's setting for the frames cut by the packets behind this job (xm_ingest_set_surface_output)
  set_cloud,   // the cloud stage's setting for the frames cut by the packets behind this job (xm_ingest_set_cloud_output)
  set_record,  // the record stage's setting for the frames cut by the packets behind this job (xm_ingest_set_record_output)
};
inline bool carries_packet(JobKind k) { return k == JobKind::records || k == JobKind::words || k == JobKind::on_device; }
inline bool copy_side_has_work(JobKind k) { return k == JobKind::records || k == JobKind::words; }

// caller -> copy thread -> launch thread
struct IngestJob {
  JobKind kind = JobKind::records;
  int k = 0;                         // staging entry
  size_t n = 0;                      // events (records) / words
  const void* host = nullptr;        // pinned source (the staging entry or the caller's pinned memory); words
  xm_evt3* dec = nullptr;
  bool pinned = true;
  bool arrived = false;              // the copy side has issued the packet's H2D copy / the chunk's decoding and recorded copied_ev[k]
  uint64_t push_no = 0;              // number of the push (from 1; the caller's count = the launch side's `issued` + 1 when its turn comes)
  double t_push = 0.0;               // when the xm_ingest_push* call entered (steady clock)
  int filter = 0, intended = 0;      // set_filter: FILTER_* (0: none) and its semantics
  int surf_select = 0, surf_dtype = 0;  // set_surface: XM_SURFACE_* (0: off) and XM_T_FLOAT32 / XM_T_FLOAT64
  int cloud_on = 0;                  // set_cloud: 1 = on, 0 = off
  int record_on = 0, record_vectors = 0;  // set_record: 1 = on, 0 = off; vector words or single events only
};

// launch side -> out thread: one cut frame.  Every cut frame is posted, so frame f is job f + 1 of the out queue.
struct OutJob {
  uint64_t frame_no = 0;
  int slot = 0, o = 0;               // result ring entry, device output frame
  const FrameDesc* desc = nullptr;
  double t_push = 0.0;               // IngestJob::t_push of the packet that completed the frame (the live latency counts from it)
  bool serial = false;               // on the frame stream, in order with the frames' kernels (see IngestLaunch::out_serial_now)
  bool done = false;                 // the launch side has run it itself (serial): the out thread only finishes the job
  bool stop = false;                 // no frame: the out thread leaves
};

// ---- the state, by owner ----

// Fixed: written by xm_ingest_create, constant from the moment it returns (= before any thread of the ingest exists), read by all.
// What the owners below POINT at changes, of course: the device writes the verdict and status rings, see IngestShared.
struct IngestFixed {
  xm_handle* h = nullptr;
  xm_ingest_config cfg{};
  u64 capacity = 0, max_packet = 0;    // capacity: a power of two (the request rounded up)
  double period = 0.0;
  long long act_thresh = 0;
  int ahead = 0;                       // packets the ingest stream may run ahead of the handled verdicts
  int ring = 0;                        // entries of the result ring
  bool threaded = false, copy_threaded = false, out_threaded = false;  // which of the three threads exist
  Stream streams[4];                   // borrowed from the process's set for the device (ingest_stream_set), else the ingest's own
  hipStream_t stream = nullptr;        // views of streams[0..3]: ingest kernels
  hipStream_t frame_stream = nullptr;  // K0 / K1 / K2 / publish of the frames that were cut
  hipStream_t copy_stream = nullptr;   // H2D of packet k+1 runs beside the kernels of packet k
  hipStream_t out_stream = nullptr;    // DMA of a finished frame to the pinned result ring + its sequence number, beside the next frame's
                                       // kernels (two out streams taking turns were slower: two 6 MB copies at once share the link)
  Event k2_ev[ING_NOUT];               // frame stream: K2 has written output frame o (the out stream's DMA waits for it)
  Event out_ev[ING_NOUT];              // out stream: output frame o has left for the result ring (the next K2 into it waits for that)
  Event copied_ev[ING_STAGE];          // per staging entry: its H2D has finished (the ingest stream waits for it)
  Event k1_ev[8];                      // frame stream: K1 of a frame has run (the ingest stream waits for it before appending more)
  // device and pinned memory
  IngestDev dev{};                     // what every ingest kernel gets by value (ring, pause ring, state, result ring, ...), as far as it
                                       // does not change per packet (that copy is IngestLaunch::dev): views of ...
  DevMem<uint4> d_buf;                 // ... these owners
  DevMem<u64> d_pring, d_key_frame;
  DevMem<IngBlk> d_blk; DevMem<IngestState> d_st; DevMem<SlotState> d_slot;
  // Activity filter: TWO sets of per-(bucket, pixel) cells + control words, taken in turn by the packets (set = staging entry & 1):
  // the first pass of packet p (k_act_first: fills the packet's cells) then depends on nothing of packet p - 1 -- only on packet
  // p - 2 having emptied the set (k_ing_append) and reset its flags (k_ing_segment).  When packet p is already on its way to the
  // device while packet p - 1 is being launched (a replay, a camera ahead of the GPU), its first pass goes out INSIDE packet p - 1's
  // k_ing_count launch (k_ing_count_act, ingest_launch3): the stream's chain per packet is count -> append -> segment with the filter
  // on as with it off (round 6: 930-990 -> 1070-1095 Mev/s on the ESL-like stream; the first pass on the copy stream, behind the
  // packet's DMA, held up the next packet's copy and ran 705-1000, on the frame stream 600: profiles/r06_ingest.md).  A packet
  // that arrives alone (a live camera) gets its first pass as a launch of its own in front of its k_ing_count, as in round 5.
  ActMem act_mem;                      // (owner of the filter's state)
  ActDev act_base{};                   // set 0 (ingest_act_set: the packet's set)
  DevMem<FrameDesc> d_descs;           // [ING_VRING]
  DevMem<IngFrameInfo> d_infos;        // [ING_VRING]
  PinnedMem<IngVerdict> h_verdicts;    // [ING_VRING] pinned host ...
  IngVerdict* d_verdicts = nullptr;    // ... and (a view) the address the device writes it at
  DevMem<float> d_out_depth[ING_NOUT];
  DevMem<uint8_t> d_out_bgr[ING_NOUT];
  DevMem<float*> d_depth_ring;         // the ING_NOUT pointers above, in device memory (k_ing_segment picks one per frame)
  DevMem<uint8_t*> d_bgr_ring;
  DevMem<uint4> d_pkt[ING_STAGE];
  DevMem<u32> d_pkt_n;                 // [ING_STAGE] event counts of chunks decoded on the device (written by the decoder's prefix kernel,
                                       // read by the ingest kernels of the packet: one cell per staging entry, free when the entry is)
  PinnedMem<IngestStatus> h_status;    // [ring] the result ring's status entries
  // debug options, read ONCE (the ingest's threads must not look at the option table while another thread changes it)
  size_t out_piece = 4u << 20;         // bytes per D2H copy of a result frame ("XM_INGEST_OUT_PIECE")
  bool out_on_frame_stream = false;    // "XM_INGEST_OUT_SERIAL" = 1: copies + sequence number ALWAYS on the frame stream, in order with the frames' kernels (A/B)
  // The out thread publishes a frame's sequence number ITSELF -- a store into the pinned status ring once the frame's copies have
  // completed (it watches their event anyway) -- instead of a one-thread kernel behind them: the out stream then carries DMA copies
  // only and never occupies a compute queue.  That matters: which hardware queue a stream lands on follows the order in which the
  // process created its streams, and a queue whose head is a barrier packet waiting for a 126 us copy holds up the other queues of
  // its pipe (profiles/r05_ingest.md section 2).  "XM_INGEST_HOST_SEQ" = 0: the kernel form (A/B).
  bool host_seq = true;
  bool opt_out_no_query = false;       // "XM_INGEST_OUT_NO_QUERY"
  bool opt_evt3_out_stream = false;    // "XM_INGEST_EVT3_OUT_STREAM"
  bool opt_trace = false;              // "XM_INGEST_TRACE"
  bool opt_act_fuse = true;            // "XM_INGEST_ACT_FUSE" = 0: never ride k_act_first of the NEXT packet on this packet's k_ing_count launch (A/B)
  // The slot's frame tag advances by one per cut frame: the slot is cleared (k_reset_slot: tags back to 0, key frame emptied)
  // before the tag can reach KEY_MAX_TAG -- the tag field of the packed keys is 19 bits wide
  uint64_t clear_every = KEY_MAX_TAG - 16;  // ("XM_INGEST_CLEAR_EVERY": tests exercise the clear)
};

// Frame event filters (N3) on the frame stream (xmaps_ingest_filter.hpp).  Scratch, made ONCE by the caller's first
// xm_ingest_set_frame_filter that selects a filter, before it posts the set_filter job: the launch side looks at it only for
// packets behind that job (the job queue orders the two), and nothing of it changes afterwards.
constexpr u64 ING_YT_MAX_CELLS = XM_INGEST_YT_MAX_CELLS;  // (include/xmaps.h)
struct IngestFrameFilter {
  bool ready = false;
  bool yt_ok = false;                  // cam_h x (LUT's largest entry + 1) cells fit ING_YT_MAX_CELLS
  bool yt_wrap = false;                // the LUT has a negative entry: FirstEventPerYT's columns may wrap at the frame's own width
  int yt_w = 0;                        // the LUT's largest entry + 1
  u32 cells_xy = 0, cells_yt = 0;
  Event read_ev[8];                    // frame stream: the stage's last read of a cut frame has run (the ingest stream waits for it
                                       // before appending more, as it waits for K1 of an unfiltered frame)
  DevMem<u32> d_last, d_first, d_sums; // the cell maps (u32 per cell, zero between frames) and the per-block counts
  DevMem<uint4> d_survivors;           // max(frame capacity, cells) records
  DevMem<FrameDesc> d_descs;           // [ING_VRING] the entries' second descriptors
  DevMem<FrameFilterInfo> d_infos;     // [ING_VRING]
  DevMem<FrameFilterCtl> d_ctl;
};

// A stage's ring of per-frame outputs (xm_ring_tag.hpp: entry and tag), as far as the surface and the cloud stage share it.  Made
// ONCE by the caller's first xm_ingest_set_*_output that switches the stage on, before it posts the stage's job: the launch side
// looks at it only for packets behind that job, and nothing of it changes afterwards.  An entry's tag lies in pinned host memory
// and is written by the device; its statistics lie beside it.
template <class Stats>
struct IngestRing {
  bool ready = false;
  int ring = 0;
  DevMem<Stats> d_stats;               // [ring] the statistics in device memory (the kernels' own copy)
  PinnedMem<u64> h_tag;                // [ring]
  PinnedMem<Stats> h_stats;            // [ring]

  int alloc(int entries) {             // (the device is current; the caller synchronises the device behind the memset)
    ring = entries;
    HIP_TRY(d_stats.alloc(ring));
    HIP_TRY(h_tag.alloc(ring, hipHostMallocMapped));
    HIP_TRY(h_stats.alloc(ring, hipHostMallocMapped));
    memset(h_tag, 0, sizeof(u64) * ring);
    memset(h_stats, 0, sizeof(Stats) * ring);
    HIP_TRY(hipMemset(d_stats, 0, sizeof(Stats) * ring));
    return XM_OK;
  }
  // the ring length a call asks for (0: `dflt`); fixed by the first call that switched the stage on
  int want_ring(int arg, int dflt) const { return arg ? arg : dflt; }
  size_t entry(uint64_t seq) const { return ring_entry(seq, ring); }
  // Frame seq's entry, if it still holds the frame: 1 and its statistics, else 0 (or copy's error).  The tag names the frame only
  // between the stage's last launch for it and the first launch of the frame that takes the entry next (the stage's first kernel
  // clears it in front of the pass that rewrites the entry): named before AND after the copy = intact.
  // names(tag): does the tag name seq; copy(entry, tag, stats): takes the payload out of the entry, 0 = done.
  template <class Names, class Copy>
  int read(uint64_t seq, Names&& names, Copy&& copy, void* stats_out) const {
    if (!ready) return 0;
    const size_t e = entry(seq);
    const u64* tag = h_tag + e;
    const u64 t0 = __atomic_load_n(tag, __ATOMIC_ACQUIRE);
    if (!names(t0)) return 0;
    Stats st;
    memcpy(&st, h_stats + e, sizeof st);
    if (int rc = copy(e, t0, st)) return rc;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (__atomic_load_n(tag, __ATOMIC_ACQUIRE) != t0) return 0;
    if (stats_out) memcpy(stats_out, &st, sizeof st);
    return 1;
  }
  void clear() {                       // reset: what the ring holds belongs to the stream that ended (nothing is in flight: flushed)
    if (ready)
      for (int e = 0; e < ring; ++e) __atomic_store_n(h_tag + e, 0ull, __ATOMIC_RELEASE);
  }
};

// Time surfaces of the cut frames (xmaps_framesurface.hpp) on the frame stream, in front of any frame event filter.  Frame f goes
// to ring entry f % ring; its tag carries its dtype (surface_tag).
struct IngestSurface {
  IngestRing<FsStats> r;
  size_t cells = 0, stride = 0;        // cam_w * cam_h; the same rounded up to FS_CPT (the winner map)
  DevMem<u32> d_map;                   // one winner map, all zero between frames
  DevMem<FsAcc> d_acc;                 // one accumulator, all zero between frames
  DevMem<unsigned char> d_ring;        // [ring][cells] of 8 bytes: room for either dtype
  u32 max_chunk_blocks = 4096;         // ("XM_FS_MAX_BLOCKS", read once)
};

// Point clouds of the cut frames (xmaps_framecloud.hpp) on the frame stream, behind the surface stage and in front of any frame
// event filter.  Frame f goes to ring entry f % ring, which holds its first max_points rows (cloud_tag).
struct IngestCloud {
  IngestRing<FcStats> r;
  size_t max_points = 0;
  u32 cap = 0;                         // events the scratch holds: the longest frame the event ring can cut
  DevMem<FcAcc> d_acc;                 // one accumulator, all zero between frames
  DevMem<uint16_t> d_code;             // [cap]
  DevMem<uint2> d_cnt;                 // [cap / 64 + 1]
  DevMem<u32> d_off;                   // [cap / 64 + 1]
  DevMem<float> d_ring;                // [ring][max_points][3]
  u32 max_chunk_blocks = 4096;         // ("XM_FC_MAX_BLOCKS", read once)
};

// EVT 3.0 words of the cut frames (xmaps_evt3enc.hpp) on the frame stream, behind the cloud stage and in front of any frame event
// filter.  Frame f goes to ring entry f % ring, which holds max_words words: all of the frame's or none (cloud_tag names it).
struct IngestRecord {
  IngestRing<EncStats> r;
  size_t max_words = 0;
  u32 cap = 0;                         // events the scratch holds: the longest frame the event ring can cut
  DevMem<uint16_t> d_code;             // [cap]
  DevMem<uint2> d_cnt;                 // [cap / 64 + 1]
  DevMem<u32> d_off;                   // [cap / 64 + 1]
  DevMem<uint16_t> d_ring;             // [ring][max_words]
  u32 max_chunk_blocks = 4096;         // ("XM_ENC_MAX_BLOCKS", read once)
};

// Caller side: the thread that calls xm_ingest_push* / poll* / backlog / flush (one at a time, by the API's contract).
struct IngestCaller {
  uint64_t posted = 0;                 // pushes accepted so far
  int pkt_next = 0;                    // the staging entry the next push takes
  uint64_t pkt_push[ING_STAGE] = {};   // number of the push that used the entry last (0: never): free once that push's verdict is in
  PinnedMem<uint4> h_pkt[ING_STAGE];   // the entries' pinned twins (pageable pushes only; the other threads see them as IngestJob::host)
  uint64_t next_seq = 0;               // frames delivered through xm_ingest_poll so far
  xm_frame_pool* pool = nullptr;       // made by the first xm_ingest_poll_owned
  uint64_t last_kept = 0;              // IngestStatus::n_used of the frame xm_ingest_poll* returned last (xm_ingest_last_frame_kept)
  // host time spent inside xm_ingest_push* (what the calling thread pays per packet), for xm_ingest_host_stats
  double push_host_s = 0.0, push_wait_s = 0.0;
  uint64_t push_calls = 0, stage_waits = 0;
};

// Launch side: the launch thread, or the caller without one.  (xm_ingest_destroy's trace and xm_ingest_fused_first_passes read
// it from the caller's thread once the launch thread has left / finished a flush: the join and wait_done order that.)
struct IngestLaunch {
  uint64_t issued = 0;                 // packets whose ingest kernels have been launched
  uint64_t next_verdict = 1;           // the first packet whose verdict has not been handled
  uint64_t frames_issued = 0;          // frames whose kernels have been launched
  uint64_t frames_since_clear = 0;     // (IngestFixed::clear_every)
  uint64_t entry_frame[ING_VRING] = {};  // frame number + 1 that the packet which used the ring entry last cut (0: none): the entry is
                                       // read by that frame's K2 / publishing launches, so it is reused only once the frame is out
  double push_t[ING_VRING] = {};       // IngestJob::t_push of packet p, p % ING_VRING, until its verdict says whether it cut a frame
  int filter = 0, intended = 0;        // the frame event filter selected by the last set_filter job (0: none) ...
  unsigned char push_filter[ING_VRING] = {};  // ... and what packet p was pushed under: filter | intended << 3 (its frame's filter)
  int surf_select = 0, surf_dtype = 0; // the surface stage's setting from the last set_surface job (select 0: off) ...
  unsigned char push_surface[ING_VRING] = {};  // ... and what packet p was pushed under: select | dtype << 2
  int cloud_on = 0;                    // the cloud stage's setting from the last set_cloud job ...
  unsigned char push_cloud[ING_VRING] = {};    // ... and what packet p was pushed under
  int record_on = 0, record_vectors = 0;       // the record stage's setting from the last set_record job ...
  unsigned char push_record[ING_VRING] = {};   // ... and what packet p was pushed under: on | use_vectors << 1
  IngestDev dev{};                     // = IngestFixed::dev with the CURRENT packet's desc / info / verdict / act: passed by value to its kernels
  int act_toggle = 0;                  // the set of cells the next non-empty packet takes (ingest_act_set)
  uint64_t act_fused_push = 0;         // the packet whose k_act_first went out with its predecessor's k_ing_count (k_ing_count_act)
  uint64_t act_fused_count = 0;        // ... how many did (statistics)
  const IngestJob* next_job = nullptr; // the job queued behind the one being run, if it is a packet that has arrived (else NULL)
  // The frames cut from now on leave on the frame stream.  Set while the packets are EVT 3.0 chunks decoded on the device
  // (typically one frame per chunk: there the in-order form measured 1000 Mev/s against 840-920 on the out stream,
  // tools/esl_evt3_probe.py), cleared for packets of records (1055-1105 on the out stream against 950).
  bool out_serial_now = false;
  // XM_INGEST_TRACE: seconds waiting for verdicts / issuing frames / inside jobs / waiting for the out side to have enqueued
  // frame f - ING_NOUT / enqueuing the out work of the frames this side took itself
  double t_block_s = 0.0, t_frames_s = 0.0, t_jobs_s = 0.0, t_out_wait_s = 0.0, t_out_s = 0.0;
};

// Out side.  The out stream's work is enqueued by a thread of its own (with a launch thread; inline without): hipMemcpyAsync of a
// second copy onto a stream whose previous copy is still running BLOCKS its caller in the HIP 7.0 runtime PyTorch bundles (seen:
// 160 us per frame, 7 ms per 43 frames, whenever the copies ran slower than the frames came) -- it must not be the launch thread.
struct IngestOutSide {
  JobQueue<OutJob, 8> q;               // launch side -> out thread (the launch side never runs more than ING_NOUT frames ahead of its
                                       // finished jobs).  A job is finished once the frame's copies + sequence number have been
                                       // ENQUEUED (out_ev[o] recorded)
  FirstError err;                      // the out side's first error, noted by whichever thread ran the frame: it stays (every later
                                       // call of the launch side reports it)
  double t_out_s = 0.0;                // out thread only.  XM_INGEST_TRACE: host seconds it spent enqueuing (read after its join)
};

// Shared: everything that more than one running thread touches, with writer -> reader and what orders them.
struct IngestShared {
  // copy thread (or caller) -> launch thread, and caller -> copy thread.  An IngestJob carries everything the caller knows about
  // the packet, its push time included: no array beside the queues is written by one thread and read by another.
  JobQueue<IngestJob, 64> launch_q, copy_q;
  // launch side -> caller: = IngestLaunch::next_verdict - 1 (release / acquire): staging flow control, xm_ingest_backlog
  std::atomic<uint64_t> handled{0};
  // launch side -> caller: = IngestLaunch::frames_issued (release / acquire): xm_ingest_backlog
  std::atomic<uint64_t> frames_issued_pub{0};
  // launch and copy threads -> caller: their first error; the caller's next call takes and reports it
  FirstError err;
  // Result ring: which buffer a slot holds changes under res_mu (out side <-> caller) -- the out side takes the slot's pointers
  // for frame f and notes f there in one step, the poller (xm_ingest_poll_owned) swaps a slot's buffers only while the slot
  // still says "frame next_seq" (so a slot the ring has lapped is never handed out while a DMA writes it).
  // (raw pointers on purpose: a slot's buffers leave with a frame and are replaced from the pool: ownership crosses the C ABI)
  std::mutex res_mu;
  std::vector<float*> h_depth;
  std::vector<uint8_t*> h_bgr;
  std::vector<uint64_t> slot_frame;    // frame number + 1 whose copies were enqueued into the slot's buffers last (0: none)
  // In pinned memory (owners in IngestFixed): h_verdicts[] device -> launch side, push_no read with acquire behind the device's
  // system-scope store; h_status[].seq device or out thread (release store, the entry's last field) -> caller and launch side
  // (acquire load, re-read after the entry: xm_ingest_poll).
};

}  // namespace

struct xm_ingest {
  IngestFixed fx;
  IngestFrameFilter ff;
  IngestSurface sf;
  IngestCloud cl;
  IngestRecord rec;
  IngestCaller ca;
  IngestLaunch la;
  IngestOutSide out;
  IngestShared sh;
  std::thread th, copy_th, out_th;     // started last by xm_ingest_create, stopped through their queues and joined by xm_ingest_destroy
};
