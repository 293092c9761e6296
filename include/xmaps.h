/*
 * xmaps.h -- C-ABI of the MI355X-native X-maps hot path (libxmaps_hip.so).
 *
 * Plain C, plain pointers and sizes, no torch / C++ types.  Every entry point returns XM_OK (0) or a
 * negative error code and never throws; xm_last_error() gives the text for the calling thread.
 *
 * What it replaces (all file:line relative to the reference repo, python/ directory):
 *   xm_create            <- table setup consumed by the hot path: CamProjMaps LUTs
 *                           (cam_proj_calibration.py:246-270), XMapsDisparity.proj_x_map
 *                           (x_maps_disparity.py:44-67), DisparityToDepth (disp_to_depth.py:66-74)
 *   xm_process_frame*    <- DepthReprojectionPipe.process_ev_frame (depth_reprojection_pipe.py:121-167):
 *                           rectify_cam_coords_i16 -> compute_event_disparity ->
 *                           compute_disp_map_{projector,camera}_view -> remap_rectified_disp_map_to_proj
 *                           -> colorize_depth_from_disp, fused into three kernels
 *   xm_stage_*           <- the same stages one by one, with the reference's per-stage signatures
 *                           (cam_proj_calibration.py:277-281,299-317; x_maps_disparity.py:9-32,69-82;
 *                            disp_to_depth.py:46-63,76-115)
 *   xm_shard_*           <- (new) the event buffer sharded by index over several GPUs; the caller
 *                           max-reduces the packed key frame between xm_shard_scatter and
 *                           xm_shard_finish (RCCL all-reduce, MAX on int64)
 *
 * Threading: one handle = one device + its own HIP streams; a handle is not thread-safe.
 * Ownership: the caller owns every pointer it passes; tables are copied to the device in xm_create.
 */
#ifndef XMAPS_H
#define XMAPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XM_API_VERSION 5  /* 5: xm_activity_set_rule, XM_INGEST_ACT_SELF (round 6) */

/* error codes */
#define XM_OK 0
#define XM_ERR_INVALID (-1)  /* bad argument / config                                              */
#define XM_ERR_HIP (-2)      /* a HIP runtime call failed (xm_last_error has the hipError string)   */
#define XM_ERR_NOMEM (-3)
#define XM_ERR_INDEX (-4)    /* >= 1 event indexed outside a table/frame: where NumPy raises
                                IndexError in the reference.  The frame is still produced with the
                                offending events dropped; stats.n_index_errors counts them.        */
#define XM_ERR_TOO_MANY (-5) /* more events in one frame than the key's index field can hold       */
#define XM_ERR_UNSORTED (-6) /* XM_FLAG_TIME_SORTED was set but a frame processed asynchronously since the
                                last xm_sync() was not sorted by t: its output is invalid (see the flag)  */

/* xm_config.flags */
#define XM_FLAG_TIME_SORTED 1u /* The caller declares every frame sorted by t -- true for the frames the trigger
                                  finder cuts out of the camera stream (trigger_finder.py:172) unless a frame event
                                  filter re-ordered them.  Then (tmin, tmax) = (t[0], t[n-1]) and the extrema pass
                                  (K0, 8 B/event re-read) is skipped.  The declaration is VERIFIED on the device for
                                  every frame: synchronous calls (XM_MEM_HOST) transparently redo an unsorted frame on
                                  the general path (result always exact); asynchronous calls report it through
                                  xm_frame_stats.n_unsorted and xm_sync() -> XM_ERR_UNSORTED.  Ignored when a polarity
                                  column is given. */

#define XM_FLAG_TRY_SORTED 2u  /* THE DEFAULT since API version 2 (the bit is accepted and ignored).  No promise from the caller:
                                  every frame is first run with (tmin, tmax) = (t[0], t[n-1]) (no extrema pass, 8 B/event
                                  less HBM traffic, one launch less) while the device checks that every event lies inside that
                                  range; a frame for which that fails is redone on the general path automatically -- inside the
                                  call for XM_MEM_HOST, otherwise when its slot comes round again (n_slots calls later) or in
                                  xm_sync(), whichever is first.  Results are always exact.  Contract for asynchronous
                                  calls: a frame's input and output buffers stay untouched by the caller until n_slots
                                  further frames have been submitted or xm_sync() has returned (the redo reads the inputs
                                  again and rewrites the outputs).  Not used when a polarity column is given, inside
                                  xm_graph_create, and for frames too sparse for the tiled kernel: those run the extrema pass. */
#define XM_FLAG_GENERAL 16u    /* Run the extrema pass (K0) on every frame instead of the verified shortcut above: one more
                                  launch and 8 B/event more traffic, but no frame is ever run twice -- for streams that are
                                  known to be unsorted (raster-ordered frame filters). */

#define XM_FLAG_DEFAULT_STREAMS 4u /* Create the slots' streams at the default priority.  By default they are created at the
                                     highest priority, which gives them hardware queues of their own (HIP multiplexes all
                                     streams of one priority, the application's included, onto 4 queues; sharing them cost
                                     up to 17 % of the pipelined frame rate).  hipGraph replays (xm_graph_*) however lose
                                     their branch concurrency when the process owns non-default-priority streams: set this
                                     flag on handles that replay graphs. */

#define XM_FLAG_ADAPTIVE_BATCH 32u /* Asynchronous device-pointer frames (XM_MEM_DEVICE, stats == NULL) are submitted as GROUPS -- one
                                    * set of multi-frame launches, the path xm_process_batch takes -- whenever the GPU is still busy:
                                    * a frame is launched at once when no group is in flight (an idle GPU, e.g. the 60 Hz live pipe,
                                    * never waits); otherwise it is held back and goes out together with the frames that follow --
                                    * with the first call that finds the GPU idle, when n_slots / 4 (at most 32) frames are held, or
                                    * at the next synchronising call (xm_sync, any synchronous call, xm_destroy).  Needs n_slots >= 8.
                                    * A group holds frames of ONE layout (AoS or SoA, one t_dtype, polarity column or not): a frame of
                                    * another layout closes the pending group first.  Contract of asynchronous calls on such a handle:
                                    * inputs and outputs of a frame stay untouched until xm_sync() has returned or n_slots + n_slots / 4
                                    * further frames have been submitted (a slot's previous frame is resolved -- and, if its time-sorted
                                    * shortcut failed, redone from its inputs -- when the GROUP that reuses the slot is launched, and up
                                    * to n_slots / 4 - 1 frames can be held in front of it).  Held frames are not on any stream yet:
                                    * synchronising xm_stream() alone does not launch them, xm_sync() does. */
#define XM_FLAG_LAUNCH_WORKERS 8u /* One launch thread per slot stream: asynchronous device-pointer calls (XM_MEM_DEVICE) only post
                                    a job (~5 us per call instead of ~11.5 us for the three kernel launches); everything else
                                    waits for the workers to be idle first, so ordering and results are unchanged.  Does not
                                    raise the frame rate (the GPU bounds it); for hosts whose calling thread has other work. */

/* view (RuntimeParams.camera_perspective, depth_reprojection_processor.py:34) */
#define XM_VIEW_PROJECTOR 0
#define XM_VIEW_CAMERA 1

/* where the event / output buffers of a call live */
#define XM_MEM_HOST 0   /* host pointers: staged H2D/D2H inside the call, call returns synchronised  */
#define XM_MEM_DEVICE 1 /* device pointers: everything is enqueued on the handle's stream; xm_sync() */
#define XM_MEM_HOST_PINNED 2 /* PINNED host pointers (xm_host_alloc / hipHostMalloc / hipHostRegister): asynchronous like
                                XM_MEM_DEVICE -- H2D copies, the three kernels and the D2H copies are enqueued on the next
                                slot's stream and the call returns; with n_slots > 1 the copies of one frame overlap the
                                kernels of another.  Buffers must stay valid and untouched until xm_sync(). */

/* dtype of the time column: int64 microseconds (Metavision EventCD) or an already-normalised
 * float time surface (python/eval/compute_depth_x_maps.py:89-96) */
#define XM_T_INT64 0
#define XM_T_FLOAT32 1
#define XM_T_FLOAT64 2

/* packed last-writer-wins key:  [63]=0 | tag:19 | event index:28 | disparity:16 */
#define XM_KEY_DISP_BITS 16
#define XM_KEY_IDX_BITS 28
#define XM_KEY_TAG_BITS 19
#define XM_KEY_MAX_EVENTS (1ull << XM_KEY_IDX_BITS)

typedef struct xm_handle xm_handle;

typedef struct xm_config {
  uint32_t struct_size; /* = sizeof(xm_config), for forward compatibility */
  int32_t device;       /* HIP device ordinal */
  int32_t cam_width, cam_height;
  int32_t proj_width, proj_height;
  int32_t rect_width, rect_height; /* rectified frame (calib.rect_image_{width,height})            */
  int32_t xmap_width;              /* X_MAP_WIDTH; T_PX_SCALE = xmap_width - 1 (xmd:58-59)         */
  int32_t xmap_height;             /* rows of proj_x_map (0 => rect_height)                        */
  int32_t x_offset;                /* X_OFFSET = 4242 (xmd:49); must fit int16                     */
  int32_t view;                    /* XM_VIEW_*                                                    */
  int32_t n_slots;                 /* frames that may be in flight at once (>=1; own stream each)  */
  uint32_t flags;                  /* XM_FLAG_*                                                    */
  double p03;                      /* P2[0,3] (calib:207, d2d:104-107)                              */
  float z_near, z_far;             /* d2d:71-72                                                     */
  /* host tables, reference layouts (row-major int16); copied + re-packed for the device in xm_create */
  const int16_t* cam_mapx_i16;        /* [cam_height][cam_width]   disp_cam_mapx_i16 (calib:253)    */
  const int16_t* cam_mapy_i16;        /* [cam_height][cam_width]   disp_cam_mapy_i16 (calib:254)    */
  const int16_t* proj_x_map;          /* [xmap_height][xmap_width] proj_x_map (xmd:61-67)           */
  const int16_t* disp_proj_mapxy_i16; /* [proj_height][proj_width][2] (x,y) (calib:270); may be NULL
                                         for XM_VIEW_CAMERA                                         */
} xm_config;

typedef struct xm_frame_stats {
  uint64_t n_events;       /* events handed in                                                       */
  uint64_t n_used;         /* after the polarity mask (== n_events when p == NULL)                    */
  uint64_t n_inliers;      /* events that passed both inlier masks (xmd:23,29) and were scattered    */
  uint64_t n_index_errors; /* events that would raise IndexError in the reference                    */
  double t_min, t_max;     /* frame extrema of t (over the used events), as double                   */
  float gpu_ms[4];         /* HIP-event time of {minmax, scatter, frame kernel, start of first .. end of
                              last}; filled only by xm_profile_frame, else 0                           */
  uint64_t n_unsorted;     /* XM_FLAG_TIME_SORTED: > 0 if the frame was NOT sorted (wavefronts that saw an event
                              outside [t[0], t[n-1]]); synchronous calls have already redone such a frame    */
} xm_frame_stats;

/* ---- lifetime ---------------------------------------------------------------------------------- */
/* Variant switches for tests and experiments ("XM_COLS", "XM_K2_PIPE", "XM_K2_PIPE_PPT", "XM_K2_CONSEC", "XM_K2_LIVE", "XM_K2_NLDS_MAX",
 * "XM_K2_PPT", "XM_K2_FLAGS", "XM_K1_DIRECT", "XM_K2_DIRECT", "XM_KEY32", "XM_OWN_W", "XM_OWN_SHEAR", "XM_OWN_GROUPED",
 * "XM_OWN_ROW_PASSES", "XM_OWN_EPT", "XM_K2_PER_CU", "XM_K2_CHAIN", "XM_WORKERS", "XM_XMAP_SCAN",
 * "XM_INGEST_CLEAR_EVERY", "XM_INGEST_TRACE", "XM_INGEST_OUT_PIECE", "XM_INGEST_OUT_SERIAL", "XM_INGEST_OUT_INLINE",
 * "XM_INGEST_OUT_NO_QUERY", "XM_INGEST_EVT3_OUT_STREAM", "XM_INGEST_OWN_STREAMS", "XM_INGEST_PRIOS", "XM_SHARDED_KEYS",
 * "XM_FS_MAX_BLOCKS" -- the most blocks per frame of the frame -> time surface event pass, read at every group call and when an ingest's
 * surface stage is first switched on; values as text).  Process-wide, read when a handle / an ingest is created (XM_XMAP_SCAN:
 * at every call).  "XM_K2_LIVE": 0 = the pipelined K2 loads every quad (all ones in its live-slot masks), 1 = the derived masks
 * (default), 2 = the same and their live fractions on stderr, one line per tile geometry.  The library never reads them from the environment.  value == NULL removes an option, name == NULL all. */
int xm_debug_option(const char* name, const char* value);
int xm_api_version(void);
const char* xm_last_error(void);
int xm_create(const xm_config* cfg, xm_handle** out);
void xm_destroy(xm_handle* h);
int xm_sync(xm_handle* h); /* wait for everything enqueued on every slot of the handle; XM_ERR_UNSORTED see above */
/* Frames redone on the general path because a time-sorted shortcut (XM_FLAG_TIME_SORTED in synchronous calls,
 * XM_FLAG_TRY_SORTED always) did not hold, since xm_create. */
int xm_sorted_fallbacks(xm_handle* h, uint64_t* count);
/* Frames enqueued per K1 variant since xm_create: counts[0] general (K0 + 64-bit packed keys), counts[1] verified-sorted
 * shortcut on the 64-bit key frame, counts[2] compact 32-bit key frame, counts[3] column tiles + plain u16 disparity frame
 * (no atomics; needs an injective X-map -> frame-cell relation, checked in xm_create).  A redone frame counts twice. */
int xm_path_counts(xm_handle* h, uint64_t counts[4]);
/* Which no-atomics K1 the rig qualified for in xm_create, and its geometry: info[0] = 0 none (sparse / wild tables: packed
 * keys only), 1 column tiles (injective X-map), 2 owner tiles (several time columns per frame cell -- the reference's own
 * calibration, python/cam_proj_calibration.py:299-303 with X_MAP_WIDTH = projector_width, python/x_maps_disparity.py:58-59);
 * owner tiles: info[1] = time columns per tile, [2] = halo columns read behind them, [3] = widest cell band of a tile
 * (sheared frame columns), [4] = shear per 8-row group in 1/4096 columns, [5] = extra frame columns of the sheared
 * u16 frame, [6] = first row / [7] = rows the rectify LUT can reach, [8] = owner cells outside their tile's band ("extras":
 * one slot each, flushed one by one), [9] = the most extras of one tile -- all of the plan frames take by default (ownership per
 * 8-row group on wide tiles where the rig allows it); [10], [11] = tile width and halo of the second plan (ownership per row, for
 * frames too dense for the first plan's tiles), 0 = none. */
int xm_cols_info(xm_handle* h, int32_t info[12]);
/* The owner-tile analysis of xm_create on its own (host code, no device needed): would this rig's tables qualify?  info as
 * xm_cols_info (info[0] = 2 or 0), plus [10] = the largest distance of a time column from its cell's first column, [11] = LDS
 * bytes per tile.  (The injective case, info[0] = 1, is decided on the device in xm_create.) */
int xm_own_plan_info(const xm_config* cfg, int32_t info[12]);

/* ---- the fused hot path: one projector frame of events -> depth frame (+ BGR) -------------------- */
/*
 * SoA events x[n], y[n], t[n] (dtype t_dtype), optional p[n] (NULL = all events used; otherwise only
 * events with p == 1 belong to the frame, which is what PolarityFilterAlgorithm(1) does upstream,
 * depth_reprojection_pipe.py:43,114).  Outputs (either may be NULL):
 *   depth_out f32 [H][W]      -- disparity_to_depth_rectified of the final disparity frame (A5)
 *   bgr_out   u8  [H][W][3]   -- the array process_ev_frame hands to frame_callback (A6+A7)
 * with H x W = projector size (XM_VIEW_PROJECTOR) or camera size (XM_VIEW_CAMERA).
 * mem == XM_MEM_HOST  : synchronous; stats (may be NULL) filled; returns XM_ERR_INDEX if any event
 *                       indexed out of range (frame still written).
 * mem == XM_MEM_DEVICE: asynchronous on the next slot's stream; the buffers must stay valid until
 *                       xm_sync(); stats of the most recent frame via xm_last_frame_stats() after it.
 * n == 0 and t_max == t_min are defined: an empty frame, resp. every event in X-map column 0.
 * Time stamps: any finite values whose t_max - t_min does not overflow their type -- int64 frames of up to 2^63 - 1 us from any
 * (also negative) base, float32 / float64 of any order -- give NumPy's columns bit for bit; the column and owner tiles take
 * frames of up to 2^32 - 2 us and longer ones are redone on the 64-bit path.  Overflowing spans, NaN and inf are undefined.
 */
int xm_process_frame(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p,
                     size_t n, int t_dtype, int mem, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats);

/* Same for Metavision's 16-byte EventCD records {u16 x; u16 y; i16 p; (pad) ; i64 t} (AoS), the
 * layout `evs` has when trigger_finder.py:172 calls process_ev_frame.  use_polarity != 0 applies p==1. */
int xm_process_frame_aos(xm_handle* h, const void* eventcd16, size_t n, int use_polarity, int mem,
                         float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats);

int xm_last_frame_stats(xm_handle* h, xm_frame_stats* stats);

/* HIP-event time of an EMPTY event pair on slot 0's stream (milliseconds, median of `reps`): what every
 * gpu_ms[] interval of xm_profile_frame contains on top of the kernel itself.  bench.py subtracts it. */
int xm_profile_event_overhead(xm_handle* h, int reps, float* ms_out);

/* Instrumented run of one frame (device-resident SoA buffers): each of the three kernels is launched with
 * hipExtLaunchKernelGGL, i.e. with a start and a stop HIP event attached to its own dispatch packet on the
 * stream it runs on (the timestamps rocprofv3 --kernel-trace reports); synchronous; stats->gpu_ms filled.
 * Used by bench.py for the roofline line. */
int xm_profile_frame(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p,
                     size_t n, int t_dtype, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats);

/* ---- a group of frames in ONE set of multi-frame launches (grid = frames x tiles) ------------------- */
/* All pointers are device pointers; frame f reads events [offsets_host[f], offsets_host[f+1]) of the SoA columns and
 * writes depth_out + f*H*W (and bgr_out + f*H*W*3); n_frames <= n_slots (every frame of the group owns a slot = a key
 * frame + state).  Asynchronous like XM_MEM_DEVICE calls: successive groups rotate over the handle's streams, so with
 * n_slots >= 2 * n_frames the tail of one group overlaps the head of the next; xm_sync() to wait.  XM_FLAG_TRY_SORTED /
 * XM_FLAG_TIME_SORTED apply per frame exactly as for single frames (a frame whose shortcut failed is redone when its
 * slot comes round again or in xm_sync()).  Frames too sparse for the tiled kernels are run one by one on the group's
 * stream.  Why: a single C-1M frame is 245 K1 blocks for 256 CUs, each a ~10 us dependent chain -- its launches leave
 * the chip half idle while they ramp up and drain; a group's launch keeps every CU fed. */
int xm_process_batch(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                     const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out);
/* The same for Metavision EventCD records (16-byte AoS, `python/frame_event_filter.py:33-37`) resident in device memory: frame f
 * = records [offsets_host[f], offsets_host[f+1]); every event is used (no polarity selection).  What an offline replay of a
 * recording feeds: `DepthReprojectionPipe.process_ev_frames` in x_maps_amd/depth_reprojection_pipe.py stages a list of host
 * frames and calls this. */
int xm_process_batch_aos(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, float* depth_out,
                         uint8_t* bgr_out);
/* The same group, synchronously, with start / stop events attached to the dispatch packets of its launches (the time
 * stamps rocprofv3 --kernel-trace reports): gpu_ms[0] = the extrema pass K0 (general path) or the boundary pass K0b
 * (column tiles), 0 when neither ran; [1] = K1; [2] = K2; [3] = start of the first .. end of the last. */
int xm_profile_batch(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, int t_dtype,
                     const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out, float gpu_ms[4]);

/* ---- a batch of frames captured once into a hipGraph and replayed (BASELINE config 5) ------------ */
/* The capture uses the multi-frame launches above: with n_slots >= n_frames the whole batch is three kernel nodes;
 * otherwise groups of n_slots / 2 frames alternate between two branches of the graph. */
/* All pointers are device pointers that stay valid for the graph's lifetime.  Frame f reads events
 * [offsets[f], offsets[f+1]) of the SoA columns and writes depth_out + f*H*W (and bgr_out + f*H*W*3). */
typedef struct xm_graph xm_graph;
int xm_graph_create(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p,
                    int t_dtype, const uint64_t* offsets_host, int n_frames, float* depth_out, uint8_t* bgr_out,
                    xm_graph** out);
int xm_graph_launch(xm_graph* g); /* asynchronous; xm_sync(handle) to wait */
void xm_graph_destroy(xm_graph* g);

/* ---- per-event debug view: every intermediate of A1/A2 for bit-exact tests ------------------------ */
/* Host or device SoA in (mem), host or device out (same mem).  Any output may be NULL.
 *   xr, yr  : rectify_cam_coords_i16            ts : X-map column (t_scaled, xmd:19)
 *   disp    : xp - xr - x_offset (int16 wrap), defined where the y-mask holds, else 0
 *   mask    : final inlier mask (u8 0/1), y-mask & disp >= 0 (& p == 1 when p given)              */
/* tests: the column-tile path's exact integer time thresholds thr[0 .. xmap_width] of a frame whose first / last stamps are
 * t_first / t_last: thr[c] = the smallest a in [0, t_last - t_first + 1] with column(t_first + a) >= c, column() being
 * `rint(((t - tmin) / (tmax - tmin)) * (xmap_width - 1))` in float64 exactly as python/x_maps_disparity.py:16-19 computes it. */
int xm_debug_cols_thresholds(xm_handle* h, long long t_first, long long t_last, uint32_t* out_host);
/* tests: A3's output of the handle's last frame when it took the column / owner tiles (xm_path_counts; not after a redo): the
 * u16 disparity frame as [rect_height][rect_width] row-major (python/cam_proj_calibration.py:299-303's disp_map, 0 = empty). */
int xm_debug_last_disp_frame(xm_handle* h, uint16_t* out_host);
/* tests: frames finished by the software-pipelined K2 (groups on the u16 frame) since xm_create; XM_K2_PIPE=2 in the environment
 * sends every group there, XM_K2_PIPE=0 none. */
int xm_debug_k2_pipe_frames(xm_handle* h, uint64_t* count);
/* tests: the group frame kernel (the pipelined K2 where it takes the group -- xm_debug_k2_pipe_frames tells --, else the
 * one-block-per-tile kernel) on n_frames (1 .. 64) caller-supplied u16 disparity frames in host memory, each plain column-major
 * [rect_width][rect_height] as xm_shard_finish_u16 takes them; the entry puts them into the slots' (sheared) frame layout.
 * valid_host (nullable): 0 = frame f is not run, its outputs keep what they held.  depth_out / bgr_out: device pointers, either
 * may be NULL; frame f writes depth_out + f*H*W and bgr_out + f*H*W*3.  Projector view only.  Synchronous; touches no slot. */
int xm_debug_k2_group_u16(xm_handle* h, const uint16_t* frames_host, int n_frames, const uint8_t* valid_host,
                          float* depth_out, uint8_t* bgr_out);
int xm_debug_event_outputs(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p,
                           size_t n, int t_dtype, int mem, int16_t* xr, int16_t* yr, int16_t* ts, int16_t* disp,
                           uint8_t* mask);

/* ---- the reference's stages one by one (host pointers, synchronous) -------------------------------- */
/* A1  CamProjMaps.rectify_cam_coords_i16(events) -> (xr, yr) */
int xm_stage_rectify(xm_handle* h, const uint16_t* x, const uint16_t* y, size_t n, int16_t* xr, int16_t* yr);
/* A1f CamProjMaps.rectify_cam_coords_f32(events) (cam_proj_calibration.py:272-275): gather from the caller's float
 *     rectify maps, row-major [cam_h][cam_w]; the offline evaluation caller needs it for the point cloud
 *     (eval/compute_depth_x_maps.py:99).  Out-of-range coordinates -> XM_ERR_INDEX. */
int xm_stage_rectify_f32(xm_handle* h, const float* mapx_f32, const float* mapy_f32, const uint16_t* x,
                         const uint16_t* y, size_t n, float* xr, float* yr);
/* CamProjMaps.construct_point_cloud(xpr, ypr, disp) (cam_proj_calibration.py:319-331): Q is the 4x4 float64
 *     reprojection matrix (row-major; cast to float32 like the reference), cloud is float32 [n][3]. */
int xm_stage_point_cloud(xm_handle* h, const double* Q, const float* xpr, const float* ypr, const float* disp, size_t n,
                         float* cloud);
/* A2  compute_disparity(xr, yr, t, X, T_PX_SCALE, X_OFFSET): full-length disp[n] (0 where masked out)
 *     and mask[n]; the caller compacts disp[mask] to get the reference's first return value */
int xm_stage_event_disparity(xm_handle* h, const int16_t* xr, const int16_t* yr, const void* t, size_t n,
                             int t_dtype, int16_t* disp, uint8_t* mask);
/* A3  compute_disp_map_projector_view: full-length xr, yr, disp + mask -> f32 [rect_h][rect_w] */
int xm_stage_disp_map_projector_view(xm_handle* h, const int16_t* xr, const int16_t* yr, const int16_t* disp,
                                     const uint8_t* mask, size_t n, float* disp_map);
/* A3' compute_disp_map_camera_view: x, y, disp + mask -> f32 [cam_h][cam_w] */
int xm_stage_disp_map_camera_view(xm_handle* h, const uint16_t* x, const uint16_t* y, const int16_t* disp,
                                  const uint8_t* mask, size_t n, float* disp_map);
/* A4  DisparityToDepth.remap_rectified_disp_map_to_proj: f32 [rect_h][rect_w] -> f32 [proj_h][proj_w] */
int xm_stage_remap_rectified_disp_map_to_proj(xm_handle* h, const float* rect_disp, float* proj_disp);
/* A5  disparity_to_depth_rectified(disp, P2): f32 [h][w] -> f32 [h][w] */
int xm_stage_disparity_to_depth(xm_handle* h, const float* disp, int height, int width, float* depth);
/* A5+A6+A7 DisparityToDepth.colorize_depth_from_disp: f32 disparity frame -> BGR u8 [h][w][3] */
int xm_stage_colorize_depth_from_disp(xm_handle* h, const float* disp, int height, int width, uint8_t* bgr);

/* ---- multi-GPU: one shard of a frame ---------------------------------------------------------------- */
/* All pointers are DEVICE pointers.  key_frame is a caller-owned u64 [H][W] buffer (H x W = rect size
 * for the projector view, camera size for the camera view), e.g. a torch.int64 tensor, so that the
 * caller can all-reduce it (MAX) between scatter and finish.  Calls are enqueued on slot 0's stream
 * and are asynchronous unless noted. */
/* extrema of this shard's t (over p == 1 events when p given), written as 2 values of t's dtype to
 * minmax_out_host; synchronous.  An empty shard returns (+max, -max) sentinels of the dtype. */
int xm_shard_minmax(xm_handle* h, const void* t, const int16_t* p, size_t n, int t_dtype, void* minmax_out_host);
/* The same without a host round trip: the shard's extrema are left in a 16-byte DEVICE buffer as {tmin, -tmax} -- int64
 * for XM_T_INT64, float64 for the float dtypes (exact) -- so that ONE MIN all-reduce of that buffer over the ranks gives
 * the frame's extrema; an empty shard writes {+max, +max} resp. {+inf, +inf} (neutral).  Asynchronous on slot 0's stream. */
int xm_shard_minmax_device(xm_handle* h, const void* t, const int16_t* p, size_t n, int t_dtype, void* mm_dev);
/* xm_shard_scatter with the frame's {tmin, -tmax} read from that device buffer when the kernel runs (after the
 * all-reduce, ordered on slot 0's stream): minmax -> all-reduce -> scatter -> all-reduce -> finish without a single
 * host synchronisation. */
int xm_shard_scatter_device(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n,
                            int t_dtype, uint64_t idx_offset, const void* frame_mm_dev, uint32_t tag, uint64_t* key_frame);
/* zero the key frame (once per buffer, or when the tag wraps) */
int xm_shard_clear(xm_handle* h, uint64_t* key_frame);
/* scatter this shard's events; idx_offset = global index of the shard's first event; frame_minmax_host
 * = the FRAME's (tmin, tmax) in t's dtype; tag in [1, 2^19) must grow from frame to frame */
int xm_shard_scatter(xm_handle* h, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n,
                     int t_dtype, uint64_t idx_offset, const void* frame_minmax_host, uint32_t tag,
                     uint64_t* key_frame);
/* key frame (after the reduce) -> depth / BGR device buffers */
int xm_shard_finish(xm_handle* h, const uint64_t* key_frame, uint32_t tag, float* depth_out, uint8_t* bgr_out);
/* Cheaper exchange for many ranks: instead of all-reducing the whole 8-byte key frame, REDUCE-SCATTER it (MAX; rank r gets
 * cells [r*C, (r+1)*C) reduced), decode the own chunk to u16 disparities (xm_shard_decode_u16: 0 where the tag differs),
 * ALL-GATHER the u16 chunks (2 bytes per cell) and run the frame kernel on the plain disparity frame
 * (xm_shard_finish_u16; same cell order as the key frame).  Per rank (W-1)/W * (8 + 2) bytes per cell cross the links
 * instead of (W-1)/W * 16.  All asynchronous on slot 0's stream. */
int xm_shard_decode_u16(xm_handle* h, const uint64_t* key_cells, size_t n_cells, uint32_t tag, uint16_t* disp_out);
int xm_shard_finish_u16(xm_handle* h, const uint16_t* disp_frame, float* depth_out, uint8_t* bgr_out);
/* Band-sharded finish ("reduce-scatter by bands + halo, K2 band-sharded, gather the projector frame"): after the
 * reduce-scatter a rank holds the merged disparities of a band of frame columns; with a halo of xm_k2_patch_cols_max() columns
 * from either neighbour it can finish every projector tile whose patch is centred on one of its columns [col_lo, col_hi).
 * disp_frame is a full-size u16 frame ([rect_w][rect_h], column-major) of which only the band and its halos need to be valid;
 * depth_out / bgr_out are full-size projector frames: pixels of other ranks' tiles are left as they were (zero them first; a MAX
 * all-reduce over the ranks -- depth >= 0, an owner's BGR >= the zeros of the others -- assembles the frame).  Projector view. */
int xm_shard_finish_u16_band(xm_handle* h, const uint16_t* disp_frame, int col_lo, int col_hi, float* depth_out, uint8_t* bgr_out);

/* ---- shards on the column tiles (time-sorted int64 frames on rigs whose X-map is injective: the path xm_process_batch takes) ----
 * A shard is a contiguous index range of the sorted stream = whole time columns, except that its last column may go on in the
 * next shard.  Each rank but the last leaves the events of its last column to its successor; then every column is processed by
 * ONE rank, the ranks' plain u16 disparity frames are disjoint and merge by SUM (2 bytes per cell on the wire instead of the
 * 8-byte packed keys; no atomics, no extrema pass).  Per frame and rank, all enqueued on xm_stream(h, 0), TWO collectives:
 *   xm_shard_cols_pack      send_buf <- {t[0], t[n-1], n, count | x[cap] | y[cap] | t[cap]}: the shard's first / last stamp and its last
 *                           min(n, cap) events                               then ALL-GATHER of the send buffers (send_bytes each)
 *   xm_shard_cols_scatter   the frame's extrema out of the gathered headers; the own part ends where the own last column starts
 *                           (not on the last rank); the predecessor's last column out of its buffer in front of the own events
 *                           -- x / y / t (16-byte aligned) MUST have cap_events + 8 events of writable headroom in front of them
 *                           and 8 behind --; boundary pass + column-tile K1 into frame16
 *                                                                            then SUM all-reduce of reduce_u32 uint32 of frame16
 *   xm_shard_finish_u16     the frame kernel on the merged frame
 * xm_shard_cols_info: sizes for frames of n_frame_events events (frame16 holds frame_bytes: the frame + the boundary pass'
 * scratch behind it; XM_ERR_INVALID when the rig / density does not qualify).  A piece that cannot be handled (a shard without
 * events or inside one column, a last column beyond cap_events, events out of order, >= 2^32 us) raises a sticky flag instead
 * of producing a wrong frame: xm_shard_cols_failed (synchronises) reports and clears it -- MAX-all-reduce it over the ranks and
 * redo the frames since the last check with the packed keys (xm_shard_scatter_device ...). */
int xm_shard_cols_info(xm_handle* h, uint64_t n_frame_events, size_t* frame_bytes, size_t* reduce_u32, size_t* send_bytes,
                       size_t* cap_events);
int xm_shard_cols_pack(xm_handle* h, const uint16_t* x, const uint16_t* y, const int64_t* t, size_t n, void* send_buf_dev,
                       size_t cap_events);
int xm_shard_cols_scatter(xm_handle* h, uint16_t* x, uint16_t* y, int64_t* t, size_t n, uint64_t n_frame_events,
                          const void* gathered_dev, size_t send_bytes, int rank, int world, size_t cap_events, uint16_t* frame16);
int xm_shard_cols_failed(xm_handle* h, int* failed);
/* measurement: milliseconds of the column-tile K1 alone in the last xm_shard_cols_scatter issued while
 * xm_debug_option("XM_SHARD_PROFILE", "1") was set (HIP events tied to that dispatch; synchronises the handle's stream) */
int xm_shard_cols_last_k1_ms(xm_handle* h, float* ms);

/* ---- one frame over several GPUs of ONE process (xm_create_sharded owns the RCCL communicators) ----------------
 * The entry for hosts that are not Python / torch.distributed (x_maps_amd/sharded.py is the multi-process form of the same
 * exchange).  dev_ids[n_dev]: distinct HIP devices; the tables of cfg are uploaded to each (cfg->device is ignored).  Per frame
 * the event buffer (HOST memory, pageable or pinned) is split by index -- device g takes [g n / n_dev, (g + 1) n / n_dev) --,
 * one host thread per device enqueues on its device's stream: H2D, the shard's extrema, ncclAllReduce(MIN) of {tmin, -tmax},
 * the scatter with GLOBAL event indices in the packed keys, ncclAllReduce(MAX, uint64) of the key frame, and device dev_ids[0]
 * runs the frame kernel and copies depth / BGR to the caller's host buffers (either may be NULL).  Synchronous.  Results equal
 * xm_process_frame on one device bit for bit (the largest global index wins a cell = NumPy's last-writer-wins).
 * RCCL is looked up at run time (the copy already loaded into the process, else ROCm's librccl); without it only n_dev = 1 works.
 * stats (may be NULL): n_events, t_min / t_max, gpu_ms[0] / gpu_ms[1] = the two all-reduces on dev_ids[0]'s stream. */
typedef struct xm_sharded xm_sharded;
int xm_create_sharded(const int* dev_ids, int n_dev, const xm_config* cfg, xm_sharded** out);
int xm_sharded_process_frame(xm_sharded* s, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n,
                             int t_dtype, float* depth_out, uint8_t* bgr_out, xm_frame_stats* stats);
int xm_sharded_info(xm_sharded* s, int* n_dev, int* uses_rccl, uint64_t* key_frame_bytes);
/* Which exchange the frames so far took: time-sorted int64 frames without a polarity column on rigs whose X-map is injective go
 * through the columns exchange (xm_shard_cols_*: all-gather of the shards' last events + SUM all-reduce of plain u16 frames, 2
 * bytes per cell on the wire); a frame one of whose pieces objected is redone with the packed keys (frames_redone); everything
 * else takes the keys (frames_keys).  Results are the same bit for bit. */
int xm_sharded_stats(xm_sharded* s, uint64_t* frames_columns, uint64_t* frames_keys, uint64_t* frames_redone);
void xm_sharded_destroy(xm_sharded* s);

/* ---- one rank of a frame sharded over several PROCESSES (one per GPU), the library driving RCCL itself (new, round 4) --------
 * The xm_shard_* calls above leave the collectives to the host (x_maps_amd/sharded.py issues them through torch.distributed:
 * five calls and two collectives from Python per frame, ~64 us of host time).  Here the library owns the communicator: ONE
 * call per frame enqueues kernels and collectives on xm_stream(h, 0) (~15 us of host time), and a C / C++ host needs no Python.
 *   xm_shard_comm_id        rank 0: XM_SHARD_COMM_ID_BYTES opaque bytes (an RCCL unique id) for the host to hand to every rank
 *                           by whatever transport it has (MPI_Bcast, a file, torch.distributed.broadcast ...)
 *   xm_shard_comm_create    every rank, collective: the communicator on h's device + the exchange buffers for frames of
 *                           n_frame_events events.  Destroy it BEFORE h.  Several communicators per process (one per handle:
 *                           frames in flight on different streams) are fine -- each from an id of its own.
 *   xm_shard_comm_frame     the columns merge (see xm_shard_cols_*): pack -> ncclAllGather -> prepare + boundary pass +
 *                           column-tile K1 -> ncclAllReduce(SUM) of the u16 frame -> frame kernel into depth_out / bgr_out
 *                           (DEVICE pointers; both NULL: the merged frame stays in the communicator, e.g. on ranks that do not
 *                           need the result).  x / y / t: this rank's shard, 16-byte aligned, with cap_events + 8 events of
 *                           writable headroom in front and 8 behind (xm_shard_comm_info).  Asynchronous.
 *   xm_shard_comm_frame_keys  the packed-key merge (any rig, any event order, optional polarity column p): extrema ->
 *                           ncclAllReduce(MIN) -> clear + scatter with global indices (first_index = the shard's offset in the
 *                           frame) -> ncclAllReduce(MAX, uint64) -> frame kernel.  Also the redo of flagged columns frames.
 *   xm_shard_comm_failed    collective + synchronises: did ANY rank flag a columns frame since the last call?
 * RCCL is looked up at run time like for xm_create_sharded. */
#define XM_SHARD_COMM_ID_BYTES 128
typedef struct xm_shard_comm xm_shard_comm;
int xm_shard_comm_id(void* id_out);
int xm_shard_comm_create(xm_handle* h, const void* id, int rank, int world, uint64_t n_frame_events, xm_shard_comm** out);
int xm_shard_comm_info(xm_shard_comm* c, int* takes_columns, size_t* cap_events, size_t* send_bytes, size_t* frame_bytes);
int xm_shard_comm_frame(xm_shard_comm* c, uint16_t* x, uint16_t* y, int64_t* t, size_t n_own, float* depth_out, uint8_t* bgr_out);
int xm_shard_comm_frame_keys(xm_shard_comm* c, const uint16_t* x, const uint16_t* y, const void* t, const int16_t* p, size_t n_own,
                             int t_dtype, uint64_t first_index, float* depth_out, uint8_t* bgr_out);
int xm_shard_comm_failed(xm_shard_comm* c, int* failed);
void xm_shard_comm_destroy(xm_shard_comm* c);
int xm_k2_patch_cols_max(xm_handle* h, int* cols_out);
/* the stream the shard calls run on (hipStream_t as void*), so the caller can order its collective */
void* xm_stream(xm_handle* h, int slot);

/* ---- setup-time table construction ("next" row N1) --------------------------------------------------- */
/* compute_x_map_from_time_map (x_map.py:5-55): rectified projector time map f32 [height][width] (0 = undefined)
 * -> X-map int16 [height][x_map_width] (values x + x_offset, 0 = undefined) and, optionally, the matched time
 * differences f32 [height][x_map_width] (t_diffs may be NULL).  Host pointers, synchronous, no handle needed. */
int xm_build_x_map(int device, const float* time_map, int height, int width, int x_map_width, int t_px_scale,
                   int x_offset, int num_scanlines, int16_t* x_map_out, float* t_diffs_out);

/* ---- a rig's rectification maps, time map and X-map on the device ------------------------------------------------------
 * x_maps_amd/calibration.py's init_undistort_rectify_map, init_undistort_rectify_map_inverse, mapf_to_i16 and remap_nearest
 * (with esl_init._pair_i16 and the linear projector time map), one thread per pixel, float64, every float32 bit equal to that
 * NumPy code's (csrc/xmaps_rigmaps.hpp states the evaluation order; the pin is to the project's NumPy, not to OpenCV).
 * stereo_rectify, rodrigues and the 3 x 3 inverse stay with the caller.  Like xm_build_x_map these take a device ordinal, no
 * xm_handle, and are synchronous.  mem == XM_MEM_HOST: every pointer of cfg / outputs is host memory; XM_MEM_DEVICE: device
 * memory of `device`.  Matrices are row-major; K = (fx, fy, cx, cy); D = (k1, k2, p1, p2, k3).  Every output is nullable; at
 * least one must be asked for.  kernel_ms (written by the call): the kernel's time between two HIP events. */
#define XM_RIG_BORDER_CONSTANT 0
#define XM_RIG_BORDER_REPLICATE 1
#define XM_RIG_SRC_NONE 0
#define XM_RIG_SRC_IMAGE 1       /* src: f32 [src_height][src_width] */
#define XM_RIG_SRC_LINEAR_TIME 2 /* generate_linear_projector_time_map(src_width, src_height, scan_upwards), evaluated at the
                                    gathered pixel: (float)((double)(col * H + row') / (double)(W * H)), row' = H - 1 - row when
                                    scan_upwards; no table exists (esl_init.get_projector_time_surface: scan_upwards = 0) */
/* Forward map (rectified pixel -> source pixel) of a width x height target frame; ir = inv(P[:3,:3] @ R).  With mapx_in / mapy_in
 * (both or neither; f32 [height][width], follow `mem`) the map is read instead of computed: remap_nearest on a caller's map.
 * remap: src sampled at (rint(mapx), rint(mapy)), half to even.  XM_RIG_BORDER_CONSTANT: border_value where that pixel is
 * outside the source (NaN, +-inf and values beyond int32 are outside).  XM_RIG_BORDER_REPLICATE: clamped by sign, NaN to the
 * first row / column (NumPy's own result is undefined for NaN, +-inf and beyond int64).  pair_i16: interleaved (x, y), NaN ->
 * -32768, everything else clipped to int16, then rint.  src_width, src_height <= 2^24; width * height < 2^31. */
typedef struct xm_rig_forward_config {
  uint32_t struct_size; /* sizeof(xm_rig_forward_config) */
  int32_t width, height;
  int32_t src_kind, src_width, src_height, border, scan_upwards;
  float border_value;
  uint32_t reserved;
  double K[4], D[5], ir[9];
  const float* src;
  const float* mapx_in;
  const float* mapy_in;
} xm_rig_forward_config;
typedef struct xm_rig_forward_outputs {
  float* mapx;
  float* mapy;
  int16_t* pair_i16; /* [height][width][2]; 4-byte aligned */
  float* remap;
  float kernel_ms;
  uint32_t reserved;
} xm_rig_forward_outputs;
int xm_rig_forward_map(int device, const xm_rig_forward_config* cfg, xm_rig_forward_outputs* outputs, int mem);
/* Inverse map (source pixel -> rectified coordinates) of a width x height source frame: undistort_points on the float32 pixel
 * coordinate (five fixed-point rounds), rotated by R, projected with P = (P00, P11, P02, P12).  mapx_i16 / mapy_i16 / pair_i16:
 * rint, half to even; an entry outside int16 (or NaN) is XM_ERR_INVALID naming the map -- mapf_to_i16's assertion; the float
 * maps of such a call are still written for XM_MEM_DEVICE. */
typedef struct xm_rig_inverse_config {
  uint32_t struct_size; /* sizeof(xm_rig_inverse_config) */
  int32_t width, height;
  uint32_t reserved;
  double K[4], D[5], R[9], P[4];
} xm_rig_inverse_config;
typedef struct xm_rig_inverse_outputs {
  float* mapx;
  float* mapy;
  int16_t* mapx_i16;
  int16_t* mapy_i16;
  int16_t* pair_i16; /* [height][width][2]; 4-byte aligned */
  float kernel_ms;
  uint32_t reserved;
} xm_rig_inverse_outputs;
int xm_rig_inverse_map(int device, const xm_rig_inverse_config* cfg, xm_rig_inverse_outputs* outputs, int mem);
/* calibration.build_tables' chain in one call: the projector's forward map -> the linear time map sampled through it
 * (time_map_rect, left in device memory) -> xm_build_x_map's kernels on that buffer -> the X-map; the camera's inverse map as
 * f32 and int16, the projector's as an interleaved int16 pair.  time_map_rect_in (nullable, f32 [rect_height][rect_width]): a
 * caller-supplied rectified time map, uploaded instead of the forward map.  Every pointer is HOST memory, every output is
 * required; only these arrays come back.  The X-map's arguments and limits are xm_build_x_map's.  kernel_ms: forward map (0
 * with time_map_rect_in), X-map, camera inverse map, projector inverse map. */
typedef struct xm_rig_tables_config {
  uint32_t struct_size; /* sizeof(xm_rig_tables_config) */
  int32_t cam_width, cam_height, proj_width, proj_height, rect_width, rect_height;
  int32_t scan_upwards, border, x_map_width, t_px_scale, x_offset, num_scanlines;
  uint32_t reserved;
  double cam_K[4], cam_D[5], cam_R[9], cam_P[4];     /* camera inverse map */
  double proj_K[4], proj_D[5], proj_R[9], proj_P[4]; /* projector inverse map */
  double proj_fwd_D[5], proj_ir[9];                  /* projector forward map (its K is proj_K) */
  const float* time_map_rect_in;
} xm_rig_tables_config;
typedef struct xm_rig_tables_outputs {
  float* time_map_rect;       /* [rect_height][rect_width] */
  int16_t* x_map;             /* [rect_height][x_map_width] */
  float* cam_mapx_f32;        /* [cam_height][cam_width], like the next three */
  float* cam_mapy_f32;
  int16_t* cam_mapx_i16;
  int16_t* cam_mapy_i16;
  int16_t* proj_mapxy_i16;    /* [proj_height][proj_width][2] */
  float kernel_ms[4];
} xm_rig_tables_outputs;
int xm_rig_build_xmaps_tables(int device, const xm_rig_tables_config* cfg, xm_rig_tables_outputs* outputs);

/* ---- evaluation metrics ("next" row N4), python/eval/create_evaluation_table.py:14-63 --------------------------------- */
/* evaluation_stats(estimate, groundtruth) on two f32 depth maps [height][width] (host pointers, synchronous, no handle):
 * fill rate, RMSE, % of pixels off by more than 1 / 5 / 10 (the script's unit is cm), and the margin (1 % of the mean
 * ground-truth depth).  filter != 0 first applies load_and_filter(estimate, gt, min_depth, max_depth) (:57-62). */
typedef struct xm_eval_result {
  double fillrate, rmse, perc_1, perc_5, perc_10, margin;
  uint64_t n_valid;   /* pixels with gt > 0 and estimate > 0 (the RMSE's support) */
  uint64_t n_gt_zero; /* pixels without ground truth */
} xm_eval_result;
int xm_eval_stats(int device, const float* estimate, const float* groundtruth, int height, int width, int filter,
                  float min_depth, float max_depth, xm_eval_result* out);

/* ---- per-frame de-duplication filters ("next" row N3), frame_event_filter.py:19-128 --------------------------- */
#define XM_FILTER_FIRST_PER_YT 1      /* FirstEventPerYTFilter          (:68-97)  cell = (y, xp[i])          */
#define XM_FILTER_FIRST_PER_XY 2      /* FirstEventPerXYFilter          (:43-65)  cell = (y, x)              */
#define XM_FILTER_LAST_PER_XY 3       /* LastEventPerXYFilter           (:19-40)                            */
#define XM_FILTER_MEAN_FIRST_LAST_PER_XY 4 /* MeanFirstLastEventPerXYFilter (:100-128)                       */
/* EventCD records in (host, n), events with p != 1 are ignored; xp_i16[n] only for XM_FILTER_FIRST_PER_YT.  The
 * reference sizes its maps map_height = max(y)+1, map_width = max(x)+1 (or max(xp)+1): pass those.  Output: EventCD
 * records in raster order of the cells (capacity map_height*map_width), *n_out of them.  Synchronous.
 * intended_semantics == 0 reproduces what the reference computes: its "first event" maps are written through
 * reversed views (`map[y[::-1], x[::-1]] = t[::-1]`), which NumPy iterates in memory order, so every filter keeps
 * the LAST event per cell (golden vectors g5_filters).  != 0: the first event, as the class names say. */
int xm_frame_event_filter(xm_handle* h, int filter, int intended_semantics, const void* eventcd16_in, size_t n,
                          const int16_t* xp_i16, int map_height, int map_width, void* eventcd16_out, size_t* n_out);

/* ---- device-side ingest ("next" row N2): inter-event pauses of a stream ------------------------------------------ */
/* np.nonzero(np.diff(t) >= thresh_us)[0] (trigger_finder.py:153-155) for a stream of n events.  Exactly one of t
 * (int64[n]) / eventcd16 (n 16-byte EventCD records) is given; mem = XM_MEM_HOST or XM_MEM_DEVICE for that input.
 * idx_out: host buffer of capacity idx_capacity (uint32 indices, ascending); *n_out = number of pauses found (may
 * exceed idx_capacity: then only the first idx_capacity are written).  Synchronous. */
int xm_find_pauses(xm_handle* h, const int64_t* t, const void* eventcd16, size_t n, int mem, int64_t thresh_us,
                   uint32_t* idx_out, size_t idx_capacity, size_t* n_out);

/* ---- device-side ingest ("next" row N2): raw camera packets -> frames, the stream never leaves HBM ----------------------- */
/* Replaces, per packet, what depth_reprojection_pipe.py:110-119 + trigger_finder.py:128-189 do on the host: polarity filter
 * (p == 1), activity-noise filter, buffering, pause detection (diff(t) >= 40 us), frame cut (> 1/2 period, <= 1 period,
 * > 1000 events, 2 events trimmed on both sides) -- as kernels over a device-resident event RING (capacity_events rounded up to
 * a power of two; its first half is mirrored behind its end, so a frame of up to capacity / 2 events is contiguous wherever it
 * starts and nothing is ever moved).  Per packet: three ingest launches (four with the activity filter) (count, append, trigger finder -- pauses are found once,
 * when an event is appended, and kept in a ring of stream indices), the frame kernels K0 -> K1 -> K2 on the frame the DEVICE
 * described (a record in device memory; the host learns from a 16-byte verdict per packet WHETHER it cut a frame and launches
 * the frame kernels with exact grids only then), the frame's statistics, and -- on a stream of their own, beside the next frame's
 * kernels -- the DMA copies of its outputs to the result ring and the sequence number behind them.  xm_ingest_push only copies
 * the packet H2D (pinned staging ring, its own stream) and enqueues those launches; finished frames appear in a ring of pinned
 * host buffers and are picked up with xm_ingest_poll.  One frame at most is cut per push, exactly like
 * RobustTriggerFinder.process_events.  Threads: a launch thread (per packet: the copy and the launches) and an out thread (per
 * cut frame: the result copies) unless XM_INGEST_NO_LAUNCH_THREAD.  The four HIP streams come from one set per device and
 * process, lent to one ingest at a time and never destroyed (an ingest alive beside another one creates its own).
 * Activity filter (the reference builds and runs one unconditionally, depth_reprojection_pipe.py:65-67,116-117): Metavision's
 * ActivityNoiseFilterAlgorithm comes as a binary with the SDK; the rule implemented here (own definition, same in
 * oracle/ingest_oracle.py, which lists what is known of the differences): an event is kept iff an EARLIER event of the stream at
 * one of its 8 neighbouring pixels has t - t' <= activity_thresh_us; every (positive) event then joins its pixel's history.
 * Evaluated on the device for every kind of packet -- records, pinned records, EVT 3.0 / 2.0 chunks decoded there -- by one more
 * launch per packet; exact for any event order (a packet whose stamps run backwards or span more than 8 thresholds is judged
 * sequentially on the device: slow, same result).  A stricter comparison (t - t' < T) is activity_thresh_us = T - 1. */
typedef struct xm_ingest xm_ingest;
typedef struct xm_ingest_config {
  uint32_t struct_size;            /* = sizeof(xm_ingest_config) */
  int32_t projector_fps;           /* frame period = 1e6 / fps us (RuntimeParams.projector_fps) */
  int32_t use_polarity;            /* != 0: only events with p == 1 (PolarityFilterAlgorithm(1), pipe:43,114) */
  int32_t activity_filter;         /* != 0: the activity rule above */
  int64_t activity_thresh_us;      /* 0 => int(1e6 / fps) (pipe:65-68) */
  int64_t pause_thresh_us;         /* 0 => 40 (trigger_finder.py:98) */
  int32_t min_events_per_frame;    /* 0 => 1000 (trigger_finder.py:8) */
  int32_t result_ring;             /* finished frames kept in pinned host memory before they are overwritten; 0 => 8 */
  uint64_t capacity_events;        /* resident event ring, events (rounded up to a power of two; a frame may hold at most half of
                                      it, a full ring drops the incoming events and counts them in `overflow`); 0 => 2^21 */
  uint64_t max_packet_events;      /* largest packet xm_ingest_push accepts (<= capacity / 2, <= 2^21); 0 => 2^19 */
  uint64_t expected_events_per_frame; /* hint for the first frames' kernel choice (0: one thread per event until a frame
                                         has been delivered; afterwards the stream's own density decides) */
  int32_t want_depth, want_bgr;    /* which outputs the result ring holds */
  uint32_t flags;                  /* XM_INGEST_* */
  uint32_t reserved;               /* 0 */
} xm_ingest_config;
#define XM_INGEST_NO_LAUNCH_THREAD 1u /* By default xm_ingest_push* only stages the packet and posts it to a launch thread owned
                                       * by the ingest, which issues the copy and the ~10 launches (the caller pays ~2 us per pinned
                                       * packet instead of ~35).  With this flag the calling thread issues them itself. */
#define XM_INGEST_ACT_SELF 2u          /* activity filter: an earlier event at the event's OWN pixel qualifies too (a 3 x 3 window that
                                       * includes its centre).  The rule is this build's own definition (Metavision's filter is a
                                       * binary); the variants it may turn out to need are configuration: this flag, and a strict
                                       * comparison (t - t' < T) = activity_thresh_us - 1 on integer stamps. */
typedef struct xm_ingest_frame {
  uint64_t seq;                    /* frame number, from 0 */
  uint64_t n_events;               /* events of the cut frame */
  int64_t t_first, t_last;         /* its first / last time stamp */
  uint64_t n_inliers, n_index_errors;
  uint64_t live_after;             /* events left in the device buffer after the cut */
  uint32_t overflow;               /* events dropped so far because the device buffer was full */
  uint32_t lost;                   /* != 0: the ring was lapped, frames between the previous one and this were overwritten */
  const float* depth;              /* f32 [H][W] in the pinned ring (NULL if !want_depth); valid until result_ring - 1 */
  const uint8_t* bgr;              /* u8 [H][W][3]                   further frames have been produced                 */
  uint64_t push_seq;               /* number (from 1) of the xm_ingest_push* call whose packet cut the frame (API version 3) */
  float push_to_publish_us;        /* live latency measured by the library: that push call entered -> the frame's sequence number
                                      published (0 when the frame left in order on the frame stream: EVT chunks, no out thread) */
  uint32_t owned;                  /* xm_ingest_poll_owned: != 0 = depth / bgr belong to the caller now (API version 4) */
} xm_ingest_frame;
int xm_ingest_create(xm_handle* h, const xm_ingest_config* cfg, xm_ingest** out);
void xm_ingest_destroy(xm_ingest* g);
/* one packet of raw EventCD records (host memory, any polarity, time-ordered as the camera delivers them); asynchronous */
int xm_ingest_push(xm_ingest* g, const void* eventcd16, size_t n);
/* the same from PINNED host memory (xm_host_alloc / hipHostMalloc): no staging copy on the host; the packet must stay
 * untouched until 16 further packets have been pushed or xm_ingest_flush() has returned */
int xm_ingest_push_pinned(xm_ingest* g, const void* eventcd16_pinned, size_t n);
/* next finished frame, if any: returns 1 and fills *out, 0 if none is ready (never blocks), < 0 on error */
int xm_ingest_poll(xm_ingest* g, xm_ingest_frame* out);
/* The same, but the frame's buffers LEAVE the ring with it (out->owned = 1): they are the caller's -- no lifetime rule -- until
 * each has been given back with xm_frame_pool_release(*pool, buffer, kind) (kind 0: depth, 1: bgr), from any thread, also after
 * xm_ingest_destroy.  This is the reference's contract for frame_callback -- a fresh array per frame, which the window's thread
 * keeps as long as it likes (depth_reprojection_pipe.py:164-167, depth_reprojection_processor.py:62-64) -- without copying the
 * frame a second time on the host: the pinned buffer the DMA filled is handed out and the ring slot gets a spare one (released
 * buffers are reused; a pool of pinned buffers grows to what the consumer holds at once, at most 1024, "XM_INGEST_POOL_CAP").
 * out->owned = 0 (no spare buffer could be had): the frame is a view into the ring exactly as xm_ingest_poll returns it. */
typedef struct xm_frame_pool xm_frame_pool;
int xm_ingest_poll_owned(xm_ingest* g, xm_ingest_frame* out, xm_frame_pool** pool);
void xm_frame_pool_release(xm_frame_pool* pool, void* buffer, int kind);
/* buffers the pool has made so far / in consumers' hands / spare (only while a consumer still holds one of them, or the ingest
 * is alive: the pool goes with the later of the two).  Any pointer may be NULL. */
int xm_frame_pool_stats(xm_frame_pool* pool, uint64_t* allocated, uint64_t* outstanding, uint64_t* spare);
/* Upper bound of the frames the host has not polled yet: frames whose kernels have been issued and not been handed out by
 * xm_ingest_poll* + packets pushed whose verdict (did it cut a frame?) is still out.  While it stays below result_ring - 1 no
 * frame can be lost to the ring being lapped.  wait_below > 0: first wait -- for verdicts only, nothing is synchronised -- until
 * the bound is below that number or no packet is in flight any more (then the caller has frames to poll). */
int xm_ingest_backlog(xm_ingest* g, int wait_below, uint64_t* backlog);
/* 1 if the result ring still holds frame `seq` (xm_ingest_frame.seq) intact, 0 if a later frame has been or is being written
 * over it: a caller that copies a frame out of the ring asks this AFTER the copy (the ring is lapped only when the host falls
 * result_ring - 1 frames behind; never in a pipe that polls after every push with result_ring >= 3) */
int xm_ingest_frame_valid(xm_ingest* g, uint64_t seq);
/* Frame event filters (the reference's key E, python/frame_event_filter.py) as a stage of the ingest: `filter` = 0 (none) or
 * XM_FILTER_*, with xm_frame_event_filter's semantics for both values of intended_semantics.  The frames cut by packets pushed
 * AFTER the call go through the filter on the device, between the cut and the frame kernels (ordered like a push: nothing is
 * flushed, nothing is reset; the filter selected when a packet is handed in is the one its frame gets, as in the reference).
 * Cells: (y, x) on the cam_height x cam_width sensor; XM_FILTER_FIRST_PER_YT: (y, xr) with xr from the handle's rectify table
 * (cam_mapx_i16), on a map as wide as the frame's own max(xr) + 1, a negative xr wrapping like NumPy's negative index.  An
 * event whose cell lies outside the map (x >= cam_width, y >= cam_height, a column still negative after the wrap: the reference
 * raises IndexError) is left out and counted in the frame's n_index_errors.
 * xm_ingest_frame of a filtered frame: n_events / t_first / t_last are the CUT frame's (what the trigger finder reports),
 * n_inliers / n_index_errors the filtered frame's; xm_ingest_last_frame_kept gives the survivors' count.
 * XM_ERR_INVALID (nothing changes): an unknown filter; XM_FILTER_FIRST_PER_YT on a rig whose cell map, cam_height x (largest
 * entry of cam_mapx_i16 + 1), would exceed XM_INGEST_YT_MAX_CELLS cells.  The stage's scratch (two u32 maps of that many
 * cells, a survivors buffer) is allocated by the first call that selects a filter. */
#define XM_INGEST_YT_MAX_CELLS (1u << 22)
int xm_ingest_set_frame_filter(xm_ingest* g, int filter, int intended_semantics);
/* events of the frame most recently returned by xm_ingest_poll* that survived the frame event filter (= its n_events when none
 * was selected) */
int xm_ingest_last_frame_kept(xm_ingest* g, uint64_t* n_kept);
int xm_ingest_flush(xm_ingest* g); /* wait for everything pushed so far */
int xm_ingest_reset(xm_ingest* g); /* RobustTriggerFinder.reset(): discard the buffered events (and the activity filter's
                                     * per-pixel history: the stream starts over) */
/* the device's counters once everything pushed so far has run (synchronises like xm_ingest_flush): frames cut, events appended
 * behind the filters, events dropped because the ring had no room (also the `overflow` of every frame), events still buffered.
 * Any pointer may be NULL. */
int xm_ingest_device_stats(xm_ingest* g, uint64_t* frames_cut, uint64_t* events_appended, uint64_t* events_dropped, uint64_t* events_live);
/* what the calling thread has paid so far: number of xm_ingest_push* calls, seconds spent inside them, how often a push had to
 * wait for a staging entry (the GPU more than 16 packets behind) and the seconds spent waiting (part of host_seconds_in_push).
 * Any pointer may be NULL. */
int xm_ingest_host_stats(xm_ingest* g, uint64_t* pushes, double* host_seconds_in_push, uint64_t* staging_waits, double* seconds_waiting);

/* ---- the activity filter alone ---------------------------------------------------------------------------------------
 * For a host that keeps the trigger finder on the CPU (the default DepthReprojectionPipe of this build): what
 * `self.act_filter.process_events(self.pos_events_buf, act_out_buf)` is in the reference (depth_reprojection_pipe.py:116-117,
 * the filter built at :65-67 as ActivityNoiseFilterAlgorithm(width, height, int(1e6 / fps))).  One packet of 16-byte EventCD
 * records in host memory, one keep flag (0 / 1) per event out; the per-pixel history stays on the device between calls.  EVERY
 * event handed in takes part (the pipe hands the filter positive events only).  Same rule, kernels and exactness as the
 * ingest's filter above.  Synchronous; thresh_us as activity_thresh_us there (but not defaulted: pass int(1e6 / fps)). */
typedef struct xm_activity xm_activity;
int xm_activity_create(xm_handle* h, int64_t thresh_us, size_t max_packet_events /* 0 => 2^19; longer packets go through in pieces */,
                       xm_activity** out);
void xm_activity_destroy(xm_activity* f);
int xm_activity_process(xm_activity* f, const void* eventcd16, size_t n, uint8_t* keep_out, size_t* n_kept /* nullable */);
int xm_activity_reset(xm_activity* f); /* forget the history */
int xm_activity_set_rule(xm_activity* f, int self_counts); /* != 0: as XM_INGEST_ACT_SELF, from the next packet on */
/* packets (pieces) so far whose stamps ran backwards or spanned more than 8 thresholds: judged sequentially on the device */
int xm_activity_stats(xm_activity* f, uint64_t* sequential_packets);
int xm_ingest_activity_stats(xm_ingest* g, uint64_t* sequential_packets); /* the same for an ingest's filter (synchronises) */
/* packets so far whose first pass of the activity filter went out inside the packet before's counting launch (they were queued
 * when that one was launched: a replay, a camera ahead of the GPU) instead of as a launch of their own (synchronises) */
int xm_ingest_fused_first_passes(xm_ingest* g, uint64_t* n);

/* ---- EVT 3.0 words -> EventCD records on the device --------------------------------------------------------------
 * The reader in front of the ingest for recordings (Prophesee RAW files, EVT 3.0: a public format; the reference reads them
 * through Metavision's closed RawReaderBase, python/bias_events_iterator.py:53-96).  The 16-bit words cross PCIe as they are
 * stored (about 2-4 bytes per event) and are decoded by three kernels (scans over the format's state machine:
 * x_maps_amd/csrc/xmaps_evt3.hpp); the decoder keeps the state (row, time, vector base, 24-bit wrap count) from chunk to chunk.
 * Same results as x_maps_amd/evt3.py's host decoder, word for word (unpinned against Metavision, like that one).
 * max_words = the largest chunk (0 = 2^20), max_events = room for xm_evt3_decode's records (0 = 2 * max_words). */
typedef struct xm_evt3 xm_evt3;
int xm_evt3_create(xm_handle* h, size_t max_words, size_t max_events, xm_evt3** out);
void xm_evt3_destroy(xm_evt3* d);
int xm_evt3_reset(xm_evt3* d); /* forget the state: the next chunk starts a stream */
/* Start-of-stream rule (either encoding; takes effect from the next chunk).  off (default): events in front of the stream's first
 * EVT_TIME_HIGH word are emitted with the time base at its initial 0 (only their low time bits are known); on: they are NOT
 * emitted -- a reader that waits for the first time base.  Which of the two Metavision's reader does is unpinned here
 * (tools/pin_thirdparty.py, case "no_first_time_high", decides). */
int xm_evt3_wait_for_time_base(xm_evt3* d, int on);
/* Synchronous.  *events_dev = the records in device memory (16-byte EventCD, valid until the next call), *n_events their number;
 * XM_ERR_TOO_MANY if the chunk has more words than max_words or decodes to more events than max_events. */
int xm_evt3_decode(xm_evt3* d, const uint16_t* words_host, size_t n_words, const void** events_dev, size_t* n_events);
/* One chunk of words as ONE packet of the ingest: decoded straight into the packet's slot on the decoder's own stream, then
 * everything xm_ingest_push does behind the copy (the activity filter included, when the ingest has it on).
 * words_pinned != 0: the words lie in pinned host memory (xm_host_alloc) and are copied from there (untouched until 16 further chunks have been
 * pushed or xm_ingest_flush() has returned).
 * n_events != NULL: the decoding is waited for and *n_events = the packet's events; a chunk that decodes to more than
 * max_packet_events returns XM_ERR_TOO_MANY with decoder and ingest unchanged (push it again in halves).
 * n_events == NULL: nothing is waited for -- the ingest's kernels read the chunk's event count from device memory; a chunk that
 * decodes to more than max_packet_events is truncated to that and the excess counted in the frames' `overflow`. */
int xm_ingest_push_evt3(xm_ingest* g, xm_evt3* d, const uint16_t* words_host, size_t n_words, int words_pinned, size_t* n_events);
/* The same for EVT 2.0 ("EVT2/EVT3 RAW reader"), the oldest of Prophesee's three public RAW encodings: 32-bit
 * little-endian words, [31:28] type -- 0x0 CD_OFF / 0x1 CD_ON {t[5:0], x[10:0], y[10:0]}: one event, p = type; 0x8 EVT_TIME_HIGH
 * {t[33:6]}: the time base of the words behind it; triggers and vendor words are skipped (x_maps_amd/csrc/xmaps_evt2.hpp; host
 * form x_maps_amd/evt2.py, independent checker oracle/evt2_oracle.py).  xm_evt2_create makes a decoder OBJECT OF THE SAME TYPE
 * for that encoding: xm_evt3_destroy / xm_evt3_reset serve it, xm_evt2_decode / xm_ingest_push_evt2 take its 32-bit words (the
 * EVT 3.0 entry points refuse it and vice versa).  max_events = 0: max_words (a word is at most one event). */
typedef xm_evt3 xm_raw_decoder; /* the decoder object, whichever encoding it was created for */
int xm_evt2_create(xm_handle* h, size_t max_words, size_t max_events, xm_raw_decoder** out);
int xm_evt2_decode(xm_raw_decoder* d, const uint32_t* words_host, size_t n_words, const void** events_dev, size_t* n_events);
int xm_ingest_push_evt2(xm_ingest* g, xm_raw_decoder* d, const uint32_t* words_host, size_t n_words, int words_pinned, size_t* n_events);
/* The same for EVT 2.1, the 64-bit vectorised RAW encoding of Gen4 / IMX636 cameras: little-endian 64-bit words, [63:60] type --
 * 0x0 EVT_NEG / 0x1 EVT_POS {t[5:0] at 59:54, x_base[10:0] at 53:43, y[10:0] at 42:32, valid[31:0]}: one event at (x_base + n, y)
 * for every set bit n of valid, in ascending n, p = type (x_base is decoded as it stands, a multiple of 32 or not); 0x8
 * EVT_TIME_HIGH {t[33:6] at 59:32}: the time base of the words behind it, loops as in EVT 2.0; triggers and vendor words are
 * skipped (x_maps_amd/csrc/xmaps_evt21.hpp; host form x_maps_amd/evt21.py, independent checker tests/evt21_ref.py).  A word is
 * 0..32 events: max_words must be < 2^27, max_events = 0 means 4 * max_words, and a chunk that decodes to more than max_events is
 * XM_ERR_TOO_MANY with the true count and the state unchanged, as for the other encodings.
 * xm_evt21_set_legacy_halves(on): the file stores each word as two 32-bit little-endian halves with the HIGH half first
 * ("endianness=legacy" in the header's format line); the halves are put back on the device where a word is loaded.  Takes effect
 * from the next chunk; XM_ERR_INVALID on a decoder of another format. */
int xm_evt21_create(xm_handle* h, size_t max_words, size_t max_events, xm_raw_decoder** out);
int xm_evt21_set_legacy_halves(xm_raw_decoder* d, int on);
int xm_evt21_decode(xm_raw_decoder* d, const uint64_t* words_host, size_t n_words, const void** events_dev, size_t* n_events);
int xm_ingest_push_evt21(xm_ingest* g, xm_raw_decoder* d, const uint64_t* words_host, size_t n_words, int words_pinned, size_t* n_events);
/* And for DAT (version 2, CD events), the other container the reference's --input takes: 8-byte records behind the header (its
 * '%' lines and the two bytes event type 0x0C, event size 8 are the caller's to skip: x_maps_amd/dat.py), u32 ts (us) then u32
 * data {x at 13:0, y at 27:14, p at 31:28}, every record one event; t = (loops << 32) | ts, a loop where ts falls back by more than
 * 2^31 against the record before it (x_maps_amd/csrc/xmaps_dat.hpp; independent checker tests/dat_ref.py).  max_events = 0:
 * max_words (= records).  xm_evt3_wait_for_time_base has nothing to wait for in this format. */
int xm_dat_create(xm_handle* h, size_t max_records, size_t max_events, xm_raw_decoder** out);
int xm_dat_decode(xm_raw_decoder* d, const void* records_host, size_t n_records, const void** events_dev, size_t* n_events);
int xm_ingest_push_dat(xm_ingest* g, xm_raw_decoder* d, const void* records_host, size_t n_records, int records_pinned, size_t* n_events);

/* ---- frames cut at a recording's external trigger events -----------------------------------------------------------
 * A rig whose projector is wired to the camera's sync jack records one EXT_TRIGGER word (type 0xA) per pulse: the exact frame
 * boundaries, in stream order (the paper's section 3.4: the pause finder is the fallback for rigs without a sync line).  The
 * word, per encoding (the vendor's published format description; unpinned against Metavision, like the decoders):
 *   EVT 3.0  [15:12] = 0xA, id [11:8], value [0]; the time is the state machine's current TIME_HIGH / TIME_LOW exactly as for a CD
 *            event at that word (a TIME_HIGH that changed the field restarts the low field at 0; the 24-bit wrap count applies)
 *   EVT 2.0  [31:28] = 0xA, t[5:0] at [27:22], id [12:8], value [0]; t = (loops << 34) | (time_high << 6) | t[5:0], as for CD words
 *   EVT 2.1  [63:60] = 0xA, t[5:0] at [59:54], id [44:40], value [32]; composed as in EVT 2.0 (legacy halves swapped back first)
 * A trigger word changes no decoder state.  event_index = the number of records the decoder writes for the chunk IN FRONT of the
 * word: the boundary is exact in stream order whatever the time stamps are.  Records come out in word order.  Start-of-stream
 * rule as for the events (xm_evt3_wait_for_time_base): in front of the stream's first TIME_HIGH a trigger carries the time
 * base 0 (off) or is not emitted (on).  (x_maps_amd/csrc/xmaps_exttrigger.hpp: two further launches per chunk; host form
 * x_maps_amd/ext_trigger.py, independent checker tests/ext_trigger_ref.py) */
typedef struct xm_ext_trigger {
  int64_t t;            /* us                                                             */
  uint32_t event_index; /* records of the chunk in front of the word                      */
  uint8_t id;           /* the trigger channel                                            */
  uint8_t value;        /* 1: rising edge, 0: falling edge                                */
  uint16_t reserved;    /* 0                                                              */
} xm_ext_trigger;
/* max_triggers = room for one chunk's records; 0 (default) = off: the two launches are not issued, nothing is allocated.  Takes
 * effect from the next chunk.  XM_ERR_INVALID on a DAT decoder (CD DAT files carry no trigger words).  Only the synchronous
 * decode entries (xm_evt3_decode / xm_evt2_decode / xm_evt21_decode, xm_trigframes_push) extract; xm_ingest_push_evt* ignore it.
 * A chunk with more trigger words than max_triggers: the decode returns XM_ERR_TOO_MANY with the decoder's state unchanged, as
 * for too many events (decode it again in halves). */
int xm_evt_set_ext_triggers(xm_raw_decoder* d, size_t max_triggers);
/* The records of the last successful xm_evt*_decode (at most cap of them are copied, *n = their number): *n = 0 when extraction
 * is off, after xm_evt3_reset and after an empty chunk. */
int xm_evt_last_ext_triggers(xm_raw_decoder* d, xm_ext_trigger* out_host, size_t cap, size_t* n);

/* THE CUT RULE of this build (pure host code: x_maps_amd/csrc/host/xm_trigger_cut.hpp; Python mirror TriggerFrameCutter).
 *  - A trigger is SELECTED when (cfg.id < 0 || id == cfg.id) and its value matches cfg.edge (XM_TRIG_RISING: 1, XM_TRIG_FALLING:
 *    0, XM_TRIG_BOTH: either).
 *  - I_k = the absolute stream index of the k-th selected trigger since create / reset: the events kept so far plus the trigger's
 *    index among the chunk's kept events.  Frame k holds the kept events [I_k, I_k+1).  Nothing is trimmed (the reference's +-2
 *    events belong to its pause heuristic).
 *  - Events in front of the first selected trigger belong to no frame: events_before_first_trigger.
 *  - min_events > 0: a frame with n <= min_events is not delivered: frames_skipped.  min_events = 0: every frame is delivered,
 *    empty ones included (an empty frame is defined in xm_process_batch_aos, xm_frames_to_time_surfaces, xm_frames_to_point_clouds).
 *  - The buffer holds cap_events records; its live part is the undelivered and unreleased frames and the open one.  A chunk of n
 *    decoded events needs n records of room behind the live part ("a chunk's worth": the count BEFORE positive_only, so that
 *    nothing waits for the compaction).  If live + n > cap_events the open frame is dropped -- its events so far and those up to
 *    the next selected trigger are counted in events_dropped_open_frame, cutting resumes at that trigger (the analogue of the
 *    ingest's "stream without a usable pause": bookkeeping, not an error).  If the ready frames alone leave no room, the push
 *    returns XM_ERR_TOO_MANY (release them first; the chunk is decoded and lost: reset).  Otherwise, only if the chunk does not
 *    fit behind the live part, that part is first moved to the buffer's front (front_moves; non-overlapping copies).
 *  - The open frame at reset / destroy is not a frame.
 * xm_trigframes_push: decodes the chunk with the decoder's synchronous path (extraction must be on: XM_ERR_INVALID otherwise),
 * appends the chunk's records behind the live ones -- positive_only: a stable compaction that keeps the p == 1 records (count per
 * block, fold of the earlier blocks' counts, write; the chunk's trigger indices are remapped in the same pass to "kept records
 * with chunk index < event_index", the chunk's event count to the kept total); otherwise a plain copy -- and runs the cutter.
 * *n_ready = frames waiting.  Synchronous.
 * xm_trigframes_ready: the next run of ready frames that lie back to back in the buffer (a skipped frame ends a run), at most
 * min(cap_frames, max_frames_ready if > 0): *events_dev = the buffer's base (16-byte aligned), offsets_host[0 .. *n_frames] ascending
 * record offsets into it -- ready for the three frame entries with XM_MEM_DEVICE --, opening[f] (nullable) = frame f's opening
 * trigger (event_index: its index among its chunk's kept events).  Valid until the next push / release / reset.
 * xm_trigframes_release(n): the first n ready frames are done with (call it after xm_sync). */
#define XM_TRIG_RISING 0
#define XM_TRIG_FALLING 1
#define XM_TRIG_BOTH 2
typedef struct xm_trigframes_config {
  uint32_t struct_size;     /* sizeof(xm_trigframes_config)                                  */
  int32_t id;               /* the trigger channel, < 0: any                                 */
  int32_t edge;             /* XM_TRIG_*                                                     */
  int32_t positive_only;    /* != 0: keep p == 1 records only                                */
  uint64_t cap_events;      /* the buffer, in records (0 = 2^22)                             */
  uint64_t min_events;      /* see above                                                     */
  int32_t max_frames_ready; /* per xm_trigframes_ready, 0: no limit                          */
  int32_t reserved;         /* 0                                                             */
} xm_trigframes_config;
typedef struct xm_trigframes_counters {
  uint64_t events_in, events_kept, triggers_seen, triggers_selected, frames_cut /* delivered to the ready queue */;
  uint64_t frames_skipped, events_before_first_trigger, events_dropped_open_frame, front_moves;
} xm_trigframes_counters;
typedef struct xm_trigframes xm_trigframes;
int xm_trigframes_create(xm_handle* h, const xm_trigframes_config* cfg, xm_trigframes** out);
void xm_trigframes_destroy(xm_trigframes* tf);
int xm_trigframes_reset(xm_trigframes* tf); /* drops every frame, open or ready, and the stream position; the counters stay */
int xm_trigframes_push(xm_trigframes* tf, xm_raw_decoder* d, const void* words_host, size_t n_words, int words_pinned, int* n_ready);
int xm_trigframes_ready(xm_trigframes* tf, const void** events_dev, uint64_t* offsets_host, int cap_frames, int* n_frames,
                        xm_ext_trigger* opening /* nullable */);
int xm_trigframes_release(xm_trigframes* tf, int n_frames);
int xm_trigframes_stats(xm_trigframes* tf, xm_trigframes_counters* out);

/* THE TWO FILTERS of the triggered chain (x_maps_amd/csrc/xmaps_trigfilter.hpp), what the reference's pipe does to every packet in
 * front of the cut and to every cut frame (python/depth_reprojection_pipe.py:110-119, :130-139).  Both are off by default; with
 * both off xm_trigframes_push and xm_trigframes_ready do exactly what is said above.
 * STAGE 1, the activity filter, inside xm_trigframes_push (in place of the two append launches: the first pass over the chunk,
 * the sequential judge, count, write -- four launches):
 *  - A record of the chunk is KEPT iff p == 1, it lies on the sensor (x < cam_width, y < cam_height) and the rule keeps it: some
 *    positive on-sensor record EARLIER IN THE STREAM at one of the 8 neighbouring pixels (self_counts != 0: or at its own) has
 *    t - t' <= thresh_us.  This build's definition, the ingest's (oracle/ingest_oracle.py); unpinned against Metavision.
 *  - Every positive on-sensor record joins its pixel's history, kept or not.  A record off the sensor is not kept and joins none.
 *  - The history lives in device memory between pushes: the result does not depend on how the stream is cut into chunks.
 *    xm_trigframes_reset empties it; switching the stage on starts from an empty one.
 *  - A chunk whose stamps run backwards by more than a bucket of thresh_us + 1 us, or that spans more than 8 such buckets, is
 *    judged sequentially by one block (exact, slow: ~20 ms per million records): chunks_sequential.
 *  - Everything behind it sees the filtered stream: the trigger remap ("kept records with chunk index < event_index", kept = both
 *    filters), xm_trigframes_counters.events_kept, min_events and every other line of the cut rule.  The room rule still uses the
 *    chunk's count before any filter.
 * STAGE 2, the frame event filters (the reference's key E), on the run of ready frames xm_trigframes_ready_filtered hands out:
 *  - Per frame, xm_ingest_set_frame_filter's semantics: one record per cell that fired, in raster order of the cells, cells (y, x)
 *    or -- XM_FILTER_FIRST_PER_YT -- (y, xr) on a map as wide as the frame's own max(xr) + 1 with NumPy's negative-index wrap.
 *  - An event whose cell lies outside the map is left out and counted in the frame's n_index_errors.
 *  - The survivors of the run's frames lie back to back in a buffer of the stage's own; the buffer of records is untouched (the
 *    unfiltered run stays available through xm_trigframes_ready until it is released).
 *  - Four launches for the whole run (three without the wrap), one copy of the per-frame totals back. */
/* thresh_us < 0: off (default).  Otherwise the ingest's activity rule (this build's definition, xmaps_ingest.hpp /
 * oracle/ingest_oracle.py) on the POSITIVE events of the stream, in stream order, across chunks; requires positive_only
 * (XM_ERR_INVALID otherwise; thresh_us must lie in [0, 2^31 - 2)).  Ordered like a push: takes effect with the next chunk;
 * switching it on starts from an empty history. */
int xm_trigframes_set_activity(xm_trigframes* tf, int64_t thresh_us, int self_counts);
typedef struct xm_trigframes_filter_counters {
  uint64_t events_positive, events_active, chunks_sequential;        /* stage 1: p == 1 records judged, records kept, see above */
  uint64_t frames_filtered, events_after_frame_filter, index_errors; /* stage 2 */
} xm_trigframes_filter_counters;
int xm_trigframes_filter_stats(xm_trigframes* tf, xm_trigframes_filter_counters* out);
/* filter: 0 (none, default) or XM_FILTER_*, both values of intended_semantics, with xm_ingest_set_frame_filter's cells, wrap rule,
 * XM_INGEST_YT_MAX_CELLS limit and XM_ERR_INVALID cases (nothing changes then).  max_frames (1 .. 4096): the longest run one call
 * filters (scratch: two u32 maps of max_frames x cells, a survivors buffer; allocated here). */
int xm_trigframes_set_frame_filter(xm_trigframes* tf, int filter, int intended_semantics, int max_frames);
/* xm_trigframes_ready's run (also capped by max_frames), each frame replaced by what the selected filter hands on: *events_dev =
 * the survivors buffer, offsets_host[0] = 0, frame f = [offsets_host[f], offsets_host[f+1]) in raster order of its cells;
 * n_index_errors[f] (nullable) = events of frame f whose cell lies outside the map.  filter 0: exactly xm_trigframes_ready.
 * Synchronous (one copy of the per-frame totals back).  Valid until the next push / release / reset / ready*. */
int xm_trigframes_ready_filtered(xm_trigframes* tf, const void** events_dev, uint64_t* offsets_host, int cap_frames, int* n_frames,
                                 xm_ext_trigger* opening /* nullable */, uint64_t* n_index_errors /* nullable */);

/* ---- time surfaces in, depth maps and point clouds out ("next" row N4) --------------------------------------------------
 * The reference's offline evaluation (python/eval/compute_depth_x_maps.py:79-131) for a GROUP of camera time surfaces in one
 * device call: each surface is [cam_height][cam_width] row-major, XM_T_FLOAT32 or XM_T_FLOAT64, 0 = no event.  Per surface:
 * lo / hi over the non-zero entries; every pixel v -> v' = ((double)v - lo) / (hi - lo), negatives to 0 -- the surface is
 * widened to float64 BEFORE it is normalised, whatever its dtype (the reference normalises float32 files in float32: the time
 * stamps can differ in the last bit; an existing property of this build, pinned by golden G7); a pixel is an event iff v' > 0
 * (the pixel holding lo lands on 0 and is dropped, as in the reference); (t_min, t_max) = extrema of the events' v'; then A1 ->
 * A2 -> both inlier masks -> A5 per pixel and ONE plain store of depth[y][x] (0 where no inlier event).  A surface holds at most
 * one event per pixel and in camera view an event's frame cell is its own pixel: no key frame, no atomics, no clear --
 * xm_path_counts does not move.  Results equal the stage calls (xm_stage_rectify .. xm_stage_disparity_to_depth,
 * xm_stage_rectify_f32, xm_stage_point_cloud) on the events of time_surface_to_events (x_maps_amd/eval_depth.py) bit for bit.
 * None of the kernels waits for another block of its launch: every dependency between blocks is a kernel boundary.
 * Camera-view handles only.  Defined, not errors: an all-zero surface and a surface with fewer than two distinct non-zero
 * values (hi == lo) have no events -- an all-zero depth map, n_inliers 0, visible in the statistics.  Surfaces that hold NaN or
 * +-inf are out of contract (results undefined); they neither fault nor write out of bounds. */
typedef struct xm_surface_stats {
  uint64_t n_nonzero;      /* pixels != 0                                                                 */
  uint64_t n_events;       /* pixels with v' > 0                                                          */
  uint64_t n_inliers;      /* events that passed both inlier masks = valid rows of the surface's cloud    */
  uint64_t n_index_errors; /* as xm_frame_stats.n_index_errors                                            */
  double lo, hi;           /* extrema of the non-zero entries (0, 0 for an all-zero surface)              */
  double t_min, t_max;     /* extrema of the events' v' (0, 0 without events)                             */
} xm_surface_stats;
/* The float rectify maps ([cam_height][cam_width] row-major, CamProjMaps.disp_cam_map{x,y}_f32) and the 4x4 float64 Q
 * (row-major; cast to float32 like the reference), copied to the device once.  Needed only when clouds are wanted. */
int xm_surface_set_cloud_tables(xm_handle* h, const float* mapx_f32, const float* mapy_f32, const double* Q);
/* depth_out: f32 [n_surfaces][cam_height][cam_width].  cloud_out (may be NULL): f32 [n_surfaces][cam_height * cam_width][3] -- a
 * fixed stride per surface, of which the first n_inliers rows are valid: the inlier events in raster order (the order of
 * xr_f[mask]) through construct_point_cloud (cam_proj_calibration.py:319-331; disparity 0 gives the reference's inf / nan).
 * stats_out (may be NULL): xm_surface_stats[n_surfaces], host memory for XM_MEM_HOST, device memory for XM_MEM_DEVICE.
 * mem == XM_MEM_HOST: synchronous (only the valid cloud rows are copied back).  XM_MEM_DEVICE: enqueued on the next slot's stream,
 * xm_sync() waits; buffers stay valid and untouched until then.  Scratch is allocated by the first call and grown when a larger
 * group arrives.  XM_ERR_INVALID: a handle that is not XM_VIEW_CAMERA, cloud_out without xm_surface_set_cloud_tables, a dtype
 * other than the two float types, n_surfaces <= 0. */
int xm_process_time_surfaces(xm_handle* h, const void* surfaces, int dtype, int n_surfaces, int mem, float* depth_out,
                             float* cloud_out, xm_surface_stats* stats_out);

/* ---- frames of events in, camera time surfaces out: what joins the live half to the evaluation entries -------------------------
 * For every frame the camera image that holds, per pixel, the time of the event that fired there: the input of
 * xm_process_time_surfaces, xm_esl_init_*, xm_esl_optim_* and xm_mc3d_* (the `scans_np` files of the ESL dataset), built from a
 * frame of EventCD records.  This build's own definition -- ESL's events-to-scan converter is not part of the reference
 * (DESIGN.md section 5).  The surface of one frame on the handle's cam_height x cam_width sensor:
 *   - with use_polarity != 0 only the events with p == 1 exist at all (as in xm_process_frame_aos); otherwise every event exists;
 *   - an event TAKES PART iff x < cam_width and y < cam_height; every other existing event is left out and counted in
 *     n_index_errors (how the ingest's frame filters treat them);
 *   - base = the smallest t over all existing events, those left out included;
 *   - per pixel the event with the largest (XM_SURFACE_LAST) or the smallest (XM_SURFACE_FIRST) INDEX in the frame is selected:
 *     stream order, not time, so the result is defined for any event order;
 *   - S[y][x] = t_selected - base + 1 in int64, converted ONCE to the output type by the IEEE round-to-nearest-even conversion
 *     (NumPy's astype).  A frame shorter than 2^24 us -- every frame the trigger finder can cut -- is exact in float32.  A pixel
 *     without an event holds 0; the + 1 keeps the earliest event apart from "no event";
 *   - an empty frame is defined: an all-zero surface and zero statistics.
 * The result depends on the frame alone: not on the run, on the frame's place in a group or on earlier calls.  Winners are picked
 * by integer atomics on event indices; there is no floating-point atomic and no kernel waits for another block of its launch
 * (x_maps_amd/csrc/xmaps_framesurface.hpp). */
#define XM_SURFACE_LAST 1
#define XM_SURFACE_FIRST 2
typedef struct xm_frame_surface_stats {
  uint64_t n_events;       /* existing events (all, or those with p == 1)                                   */
  uint64_t n_pixels;       /* non-zero pixels of the surface                                                */
  uint64_t n_index_errors; /* existing events left out (x >= cam_width or y >= cam_height)                  */
  int64_t t_base;          /* the smallest t over the existing events (0 for a frame without any)           */
  int64_t t_span;          /* the largest t - t_base over the existing events, those left out included      */
} xm_frame_surface_stats;
/* Frame f = records [offsets_host[f], offsets_host[f + 1]) of eventcd16 (16-byte EventCD records; 16-byte aligned in device
 * memory); a frame holds at most 2^32 - 2 events.  surfaces_out: [n_frames][cam_height][cam_width] of dtype (XM_T_FLOAT32 /
 * XM_T_FLOAT64).  stats_out (may be NULL): xm_frame_surface_stats[n_frames].  mem == XM_MEM_HOST: records, surfaces and
 * statistics are host memory, the call is synchronous.  XM_MEM_DEVICE: all three are device memory; everything is enqueued on the
 * next slot's stream, xm_sync() waits, the buffers stay valid and untouched until then (offsets_host is read inside the call).
 * Works on handles of either view.  Groups of any length are accepted (they go out as launch sequences of 32 frames).  Scratch is
 * allocated by the first call and grown when a larger group arrives.  XM_ERR_INVALID: an unknown select or dtype, n_frames <= 0,
 * decreasing offsets, a mem other than the two. */
int xm_frames_to_time_surfaces(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_polarity,
                               int select, int dtype, int mem, void* surfaces_out, xm_frame_surface_stats* stats_out);
/* The same as a stage of the device ingest.  Ordered like a push, exactly as xm_ingest_set_frame_filter: the frames cut by packets
 * pushed AFTER the call get a surface -- built on the frame stream from the CUT frame (every event in the ring has passed the
 * ingest's polarity and activity filters; use_polarity is therefore not applied again), in front of any frame event filter --
 * in a ring of `ring` surfaces in device memory (0: the ingest's result_ring).  select == 0 switches the stage off: the ingest
 * then launches nothing for it.  Scratch and ring are allocated by the first call that switches the stage on, for either dtype;
 * a later call may change select and dtype, not the ring's length (XM_ERR_INVALID).  The stage's last launch that reads a cut
 * frame runs in front of the frame's filter / K1, for which the ingest stream waits before it appends over the frame. */
int xm_ingest_set_surface_output(xm_ingest* g, int select /* 0 = off */, int dtype, int ring);
/* The surface of frame `seq` (xm_ingest_frame.seq) -> dst ([cam_height][cam_width] of the dtype the frame was built with; host
 * or device memory by `mem`), its statistics -> *stats (host memory, may be NULL).  Returns 1: copied, and the ring entry was
 * still intact after the copy; 0: never produced, not complete yet, or already overwritten (dst may have been written);
 * < 0: an error.  Once xm_ingest_poll* has handed out frame seq its surface is complete.  xm_ingest_reset keeps the stage's setting and drops the ring's contents.  Synchronous. */
int xm_ingest_copy_surface(xm_ingest* g, uint64_t seq, void* dst, int mem, xm_frame_surface_stats* stats);
/* the dtype (XM_T_*) the surface of frame seq was built with, or 0 when the ring does not hold it */
int xm_ingest_surface_dtype(xm_ingest* g, uint64_t seq);

/* ---- frames of events in, per-event point clouds out: the live half's 3-D output ------------------------------------------------
 * The reference's CamProjMaps.construct_point_cloud (cam_proj_calibration.py:319-331) as eval/compute_depth_x_maps.py:99-122
 * applies it per event -- construct_point_cloud(xr_f32[mask], yr_f32[mask], disparity) -- on a frame of EventCD records, from the
 * same int64 stamps and X-map columns as the frame's depth map.  Nothing of the definition is this build's own.  For one frame, on a
 * handle of EITHER view:
 *   - with use_polarity != 0 only the events with p == 1 exist at all (as in xm_process_frame_aos); otherwise every event exists;
 *   - (t_min, t_max) are taken over ALL existing events, those left out below included;
 *   - an existing event with x >= cam_width or y >= cam_height is LEFT OUT and counted in n_index_errors; so is one whose time
 *     column falls outside the X-map;
 *   - every other existing event goes through A1 and A2 -- the packed int16 rectify LUT, the int64 time normalisation (ties round
 *     to even; t_max == t_min puts every event in column 0) and the X-map lookup, the code K1 runs -- and is an INLIER iff both
 *     masks of x_maps_disparity.py:23,29 hold (0 <= yr < xmap_height - 1, disparity >= 0);
 *   - the cloud holds one row per inlier event IN STREAM ORDER (stable, duplicates kept: the order of xr_f[mask]):
 *     row = [x + d, y, -d, 1] through Q in float32, perspective divide, y and z negated, with x = mapx_f32[y][x],
 *     y = mapy_f32[y][x] and d = (float)disparity -- xm_stage_point_cloud's arithmetic.  disparity == 0 gives the reference's
 *     inf / nan row;
 *   - an empty frame is defined: no rows, zero statistics.
 * The result depends on the frame alone: not on the run, on the frame's place in a group or on earlier calls.  There is no
 * floating-point atomic and no kernel waits for another block of its launch (x_maps_amd/csrc/xmaps_framecloud.hpp).
 * Debug option "XM_FC_MAX_BLOCKS" (xm_debug_option): the most blocks per frame of the per-event passes, read at every group call
 * and when an ingest's cloud stage is first switched on. */
typedef struct xm_frame_cloud_stats {
  uint64_t n_events;       /* existing events (all, or those with p == 1)                                              */
  uint64_t n_inliers;      /* rows of the frame's cloud                                                                */
  uint64_t n_index_errors; /* existing events left out (off the sensor, or a time column outside the X-map)            */
  int64_t t_min;           /* the smallest / largest t over the existing events, those left out included (0, 0 for a   */
  int64_t t_max;           /*   frame without any)                                                                     */
} xm_frame_cloud_stats;
/* The float rectify maps [cam_height][cam_width] and the 4x4 float64 Q (cast to float32 as xm_stage_point_cloud does) of the two
 * entries below; copied.  Accepted on handles of either view (xm_surface_set_cloud_tables and its camera-view rule are another
 * entry's and stay as they are).  Set them before an ingest on the handle switches its cloud stage on; a later call rewrites the
 * same device tables once the device is idle. */
int xm_cloud_set_tables(xm_handle* h, const float* mapx_f32, const float* mapy_f32, const double* Q);
/* Frame f = records [offsets_host[f], offsets_host[f + 1]) of eventcd16 (16-byte EventCD records; 16-byte aligned in device
 * memory).  cloud_out: f32 [offsets_host[n_frames] - offsets_host[0]][3]; frame f's rows start at row offsets_host[f] -
 * offsets_host[0], the first n_inliers of them are valid, the rest are left untouched.  cloud_out == NULL: statistics only.
 * stats_out (may be NULL): xm_frame_cloud_stats[n_frames].  mem == XM_MEM_HOST: records, cloud and statistics are host memory,
 * the call is synchronous and only valid rows are copied back.  XM_MEM_DEVICE: all three are device memory; everything is enqueued
 * on the next slot's stream, xm_sync() waits, the buffers stay valid and untouched until then (offsets_host is read inside the
 * call).  Groups of any length are accepted (they go out as launch sequences of 32 frames).  Scratch is allocated by the first
 * call and grown when a larger group arrives.  XM_ERR_INVALID: cloud_out without xm_cloud_set_tables, n_frames <= 0, decreasing
 * offsets, a mem other than the two. */
int xm_frames_to_point_clouds(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_polarity,
                              int mem, float* cloud_out, xm_frame_cloud_stats* stats_out);
/* The same as a stage of the device ingest, ordered and ring-managed exactly like xm_ingest_set_surface_output: the frames cut by
 * packets pushed AFTER the call get a cloud -- built on the frame stream from the CUT frame (polarity is not applied again), in
 * front of any frame event filter -- in a ring of `ring` entries (0: the ingest's result_ring) of max_points rows in device memory.
 * on != 0 needs max_points > 0 and the handle's xm_cloud_set_tables.  A frame with more inliers keeps its FIRST max_points rows in
 * stream order; n_inliers reports the true count, so truncation is visible.  on == 0 switches the stage off: the ingest then
 * launches nothing for it.  Scratch and ring are allocated by the first call that switches the stage on; a later call may not
 * change max_points or the ring's length (XM_ERR_INVALID). */
int xm_ingest_set_cloud_output(xm_ingest* g, int on, int64_t max_points, int ring);
/* The cloud of frame `seq` (xm_ingest_frame.seq): its min(n_inliers, max_points) rows -> dst (f32 [..][3]; host or device memory
 * by `mem`; NULL: statistics only), its statistics -> *stats (host memory, may be NULL).  Returns 1: copied, and the ring entry was
 * still intact after the copy; 0: never produced, not complete yet, or already overwritten (dst may have been written); < 0: an
 * error.  Once xm_ingest_poll* has handed out frame seq its cloud is complete.  xm_ingest_reset keeps the stage's setting and
 * drops the ring's contents.  Synchronous. */
int xm_ingest_copy_cloud(xm_ingest* g, uint64_t seq, float* dst, int mem, xm_frame_cloud_stats* stats);

/* ---- frames of events in, EVT 3.0 words out: a replayable recording of what the pipeline processed -------------------------------
 * For one frame of 16-byte EventCD records in stream order the words are exactly x_maps_amd.evt3.encode_evt3(frame, use_vectors)
 * -- the host encoder is the definition, its state fresh for every frame, so a frame's words begin with its own EVT_TIME_HIGH,
 * EVT_TIME_LOW and EVT_ADDR_Y.  The same rule in the form that evaluates in parallel (x, y the raw u16, p the raw int16, t the
 * int64 of the record; hi = (t >> 12) & 0xfff, lo = t & 0xfff):
 *   - LINKS: event i >= 1 is linked to event i - 1 iff t, y and p are equal and x[i] > x[i - 1].  A CHAIN is a maximal sequence of
 *     linked events; its head is the frame's first event or an event that is not linked.  With use_vectors == 0 nothing is linked;
 *   - RUN STARTS: within a chain, the orbit of the head under next(i) = the first j of the chain with x[j] - x[i] >= 12.  A run is
 *     a start and the chain's events in front of its next; its columns grow strictly, so next(i) <= i + 12, and a chain holds at
 *     most 65 536 events (x is u16): the walk is bounded, and it may cross any 64-event segment or block of the kernels;
 *   - a run of one event is EVT_ADDR_X (x & 0x7ff, p & 1 in bit 11); a run of >= 2 events is VECT_BASE_X (the same fields) and ONE
 *     VECT_12 with bit x[k] - x[start] set for every event k of the run.  use_vectors == 0: every event is a run of one
 *     (= encode_evt3_singles);
 *   - in front of run start i: EVT_TIME_HIGH (hi) iff i is the frame's first event or hi differs from event i - 1's;
 *     EVT_TIME_LOW (lo) iff EVT_TIME_HIGH is sent or lo differs; EVT_ADDR_Y (y & 0x7ff) iff i is the first event or y differs.  (Only a
 *     chain's head can have any: a linked event shares t and y with its predecessor.)  Events that start no run send nothing;
 *   - fields are masked as the host encoder masks them and bits of t above bit 23 are dropped: two events whose stamps differ
 *     only there are not linked, and no time word separates them.  What that loses is counted, not refused: n_out_of_range;
 *   - a frame of n events encodes to at most 4 * n words; an empty frame is defined: no words, zero statistics.
 * The result depends on the frame alone: not on the run, on the frame's place in a group or on earlier calls.  No atomics, and no
 * kernel waits for another block of its launch (x_maps_amd/csrc/xmaps_evt3enc.hpp).  Debug option "XM_ENC_MAX_BLOCKS"
 * (xm_debug_option): the most blocks per frame of the per-event passes, read at every group call and when an ingest's record stage
 * is first switched on. */
typedef struct xm_evt3_record_stats {
  uint64_t n_events;       /* records of the frame                                                                      */
  uint64_t n_words;        /* words of the frame                                                                        */
  uint64_t n_vector_runs;  /* runs of >= 2 events (VECT_BASE_X + VECT_12)                                               */
  uint64_t n_out_of_range; /* events with x > 2047, y > 2047, p not in {0, 1} or t < 0 (encoded with their fields masked) */
  int64_t t_first;         /* the first / last record's stamp in stream order (0, 0 for an empty frame)                 */
  int64_t t_last;
} xm_evt3_record_stats;
/* Frame f = records [offsets_host[f], offsets_host[f + 1]) of eventcd16, as in xm_frames_to_point_clouds.  words_out: u16
 * [4 * (offsets_host[n_frames] - offsets_host[0])]; frame f's words start at word 4 * (offsets_host[f] - offsets_host[0]), the
 * first n_words of them are valid, the rest are left untouched.  stats_out (may be NULL): xm_evt3_record_stats[n_frames].
 * mem == XM_MEM_HOST: records, words and statistics are host memory, the call is synchronous and only valid words are copied back.
 * XM_MEM_DEVICE: all three are device memory; everything is enqueued on the next slot's stream, xm_sync() waits, the buffers stay
 * valid and untouched until then (offsets_host is read inside the call).  Handles of either view; groups of any length (launch
 * sequences of 32 frames) of fewer than 2^30 events together (XM_ERR_TOO_MANY).  Scratch is allocated by the first call and grown
 * when a larger group arrives.  XM_ERR_INVALID: n_frames <= 0, decreasing offsets, a mem other than the two, a NULL array that
 * would be used. */
int xm_frames_to_evt3_words(xm_handle* h, const void* eventcd16, const uint64_t* offsets_host, int n_frames, int use_vectors, int mem,
                            uint16_t* words_out, xm_evt3_record_stats* stats_out);
/* The same as a stage of the device ingest, ordered and ring-managed exactly like xm_ingest_set_cloud_output: the frames cut by
 * packets pushed AFTER the call get their words -- built on the frame stream from the CUT frame (behind the polarity and activity
 * filters, in front of any frame event filter) -- in a ring of `ring` entries (0: the ingest's result_ring) of max_words words in
 * device memory.  on != 0 needs max_words > 0.  Overflow is all or nothing (a truncated word stream is worse than none): a frame
 * with n_words > max_words publishes its statistics with the true n_words and no word.  on == 0 switches the stage off: the ingest
 * then launches nothing for it.  use_vectors may change from call to call; scratch and ring are allocated by the first call that
 * switches the stage on, and a later call may not change max_words or the ring's length (XM_ERR_INVALID). */
int xm_ingest_set_record_output(xm_ingest* g, int on, int use_vectors, int64_t max_words, int ring);
/* The words of frame `seq` (xm_ingest_frame.seq): its n_words words -> dst (u16; host or device memory by `mem`; NULL: statistics
 * only) unless n_words > max_words (then none), its statistics -> *stats (host memory, may be NULL).  Returns 1: copied, and the
 * ring entry was still intact after the copy; 0: never produced, not complete yet, or already overwritten (dst may have been
 * written); < 0: an error.  Once xm_ingest_poll* has handed out frame seq its words are complete.  xm_ingest_reset keeps the
 * stage's setting and drops the ring's contents.  Synchronous. */
int xm_ingest_copy_record(xm_ingest* g, uint64_t seq, uint16_t* dst, int mem, xm_evt3_record_stats* stats);

/* ---- ESL-init: the baseline of the reference's evaluation table, on the device ------------------------------------------------
 * What python/eval/compute_depth_esl.py:204-226 computes up to depth_init (the optimisation behind it: xm_esl_optim_* below; MC3D: xm_mc3d_*),
 * for a GROUP of camera time surfaces in one device call.  Per surface:
 *   1. lo / hi over the non-zero pixels, v' = ((double)v - lo) / (hi - lo), negatives to 0 -- widened to float64 first, exactly
 *      as xm_process_time_surfaces does (golden G7's convention);
 *   2. cam_rect[r][c] = v'[my][mx], (mx, my) = cam_to_rect_map[r][c], 0 where the entry lies outside the camera (nearest remap,
 *      constant border 0);
 *   3. disparity_init (:72-85): for every rectified pixel with cam_rect > 0 the window proj_rect[r][c + min_disp : c + max_disp],
 *      clipped at the row's end; candidates = its non-zero entries; with MORE THAN ONE candidate the disparity is (column of the
 *      FIRST minimum of ((double)p - e)^2, float64, no contraction) - c, otherwise 0;
 *   4. disp_cam[y][x] = disparity[ry][rx], (rx, ry) = rect_to_cam_map[y][x], 0 outside the rectified frame;
 *   5. depth = (float)(p1_03 / (double)disp_cam), 0 where the disparity is 0 (never inf).
 * The fused kernel searches only the rectified pixels step 4 references and materialises no rectified image; results equal the
 * staged composition bit for bit (golden G11 pins step 3 against the reference's own code).  No kernel has atomics or waits for
 * another block.  UNPINNED: the float -> int16 rounding of the two maps is the table builder's (x_maps_amd/esl_init.py, np.rint
 * like every other map here), not checked against a cv2.remap(INTER_NEAREST) run.
 * Defined, not errors: an all-zero surface and one with hi == lo search nothing -- zero maps, n_searched 0, visible in the
 * statistics.  NaN / +-inf surfaces are out of contract; they neither fault nor index outside a table.
 * No xm_handle is involved: like xm_build_x_map / xm_eval_stats these take a device ordinal.  An object serves one thread at a time. */
typedef struct xm_esl_init xm_esl_init;
typedef struct xm_esl_init_config {
  uint32_t struct_size; /* sizeof(xm_esl_init_config) */
  int32_t cam_width, cam_height;
  int32_t rect_width, rect_height; /* the reference: 3 x the projector */
  int32_t min_disp, max_disp;      /* 0, 0 = the reference's 5, 900; invalid: min_disp < 0, max_disp <= min_disp, max_disp > 65535 */
  int32_t reserved;
  double p1_03;                    /* P1[0, 3] of the rectification (either sign; 0 is allowed and gives zero depth) */
  const int16_t* cam_to_rect_map;  /* host, [rect_height][rect_width][2] (x, y): rectified pixel -> camera pixel   */
  const int16_t* rect_to_cam_map;  /* host, [cam_height][cam_width][2]  (x, y): camera pixel -> rectified pixel    */
  const float* proj_rect;          /* host, [rect_height][rect_width]: the rectified projector time surface, 0 = no data */
} xm_esl_init_config;              /* the three tables are copied to the device; the caller keeps ownership */
typedef struct xm_esl_init_stats {
  uint64_t n_nonzero;  /* pixels != 0                                                                        */
  uint64_t n_searched; /* camera pixels whose rectified pixel holds v' > 0 (their windows were walked)       */
  uint64_t n_matched;  /* ... of which the disparity is non-zero                                             */
  double lo, hi;       /* extrema of the non-zero pixels (0, 0 for an all-zero surface)                      */
} xm_esl_init_stats;
int xm_esl_init_create(int device, const xm_esl_init_config* cfg, xm_esl_init** out);
void xm_esl_init_destroy(xm_esl_init* e);
/* surfaces: [n_surfaces][cam_height][cam_width], XM_T_FLOAT32 or XM_T_FLOAT64.  depth_out: f32, the same shape.  disp_cam_out
 * (may be NULL): u16, the same shape.  stats_out (may be NULL): xm_esl_init_stats[n_surfaces].  mem == XM_MEM_HOST: every pointer
 * is host memory; XM_MEM_DEVICE: every pointer is device memory of the object's device.  Synchronous in both: the results are
 * there when the call returns.  Scratch is allocated by the first call and grown when a larger group arrives. */
int xm_esl_init_time_surfaces(xm_esl_init* e, const void* surfaces, int dtype, int n_surfaces, int mem, float* depth_out,
                              uint16_t* disp_cam_out, xm_esl_init_stats* stats_out);
/* Step 3 alone, on a caller-supplied rectified camera image (host, f64 [rect_height][rect_width]) against the object's proj_rect:
 * the reference's disparity_init as a function -> u16 [rect_height][rect_width] (host).  Synchronous. */
int xm_esl_init_stage_disparity(xm_esl_init* e, const double* cam_rect_host, uint16_t* disparity_rect_out);

/* ---- ESL depth optimisation: the solver behind ESL-init, on the device ----------------------------------------------------------
 * What python/eval/compute_depth_esl.py:104-129 (depth_optimization, with cost_calculator :45-69 and project_and_backproject_punkt
 * :27-42) computes for a GROUP of camera time surfaces and their depth_init maps in one device call: the maps the reference stores
 * as esl/depth_optim.  The bilateral filter and the TV denoiser behind it (:243-244), hence esl/depth_optim_filtered, are
 * xm_esl_filter_* below, which takes this call's output buffer as it is.  Per surface s with depth_init d0 (f32, as xm_esl_init_time_surfaces writes it):
 *   1. v' = max(((double)v - lo) / (hi - lo), 0) with lo / hi over the non-zero pixels, exactly as xm_esl_init_time_surfaces step 1;
 *   2. f = 1.0 / v'[0][0] (+inf when that is 0, as NumPy); every v' == 0 becomes f (:212).  The image is NOT rectified;
 *   3. pixels y in [ws, cam_height - ws), x in [ws, cam_width - ws) with d0 > 0 are optimised, ws = window_size; every other pixel
 *      is written 0.  The patch half-width is w = ws / 2 (integer division): the reference's border and patch (:107-108, :53);
 *   4. diff = (double)(d0 * d0) / p1_03 -- a float32 product, a float64 quotient, as NumPy evaluates depth**2 / P1[0, 3];
 *      a = (double)d0 - diff, b = (double)d0 + diff.  Where scipy raises (a or b not finite, a > b) the pixel is written 0 and
 *      counted in n_bad_bounds;
 *   5. xf = scipy.optimize.minimize_scalar(cost, bounds = (a, b), method = "bounded"), xatol and at most max_iter evaluations:
 *      _minimize_scalar_bounded of scipy 1.15 restated operation for operation in float64 without contraction (golden section,
 *      parabolic fit and its three acceptance tests, the tol1 step near a bound, np.sign / np.maximum with their NaN propagation,
 *      every branch of the three-point bookkeeping, the num >= maxfun exit).  (float)xf is stored;
 *   6. cost(rho): pu = the pixel (float32) through undistortPoints(cam_K, cam_D, P = cam_K) -- five fixed-point rounds, the result
 *      rounded to float32; X = ((pu_x - cx) / fx) * rho, Y likewise, Z = rho; Xp = R' (X, Y, Z) + t with Rt = {R' row-major, t};
 *      perspective divide, Brown distortion proj_D, proj_K; (xp, yp) = truncation toward zero to int32 (not finite or not
 *      representable: outside); inside iff yp - w > 0 && yp + w < proj_height && xp - w > 0 && xp + w < proj_width; inside:
 *      sqrt(sum d^2) over the (2w+1)^2 patch in raster order, d = cam'[y+i][x+j] - (double)proj[yp+i][xp+j], the sum accumulated
 *      as s = fma(d, d, s) from 0 (np.linalg.norm's dot); outside: 100000.
 * Rt is the caller's: the reference sends the float32-rounded rotation through cv2.Rodrigues and back and adds the float32-rounded
 * translation (x_maps_amd/esl_optim.py make_rt).  PINNED against the reference's own depth_optimization running on the installed
 * scipy: the solver, the cost, the truncation, the fill and the bounds (golden G13, bit for bit).  UNPINNED: the three geometry
 * functions against a real cv2.
 * Defined, not errors: an all-zero surface and one with hi == lo give zero maps and zero counts.  NaN / +-inf surfaces are out of
 * contract; they neither fault nor index outside a table.  No kernel has atomics or waits for another block; every loop is bounded
 * by max_iter.  No xm_handle is involved; an object serves one thread at a time. */
typedef struct xm_esl_optim xm_esl_optim;
typedef struct xm_esl_optim_config {
  uint32_t struct_size; /* sizeof(xm_esl_optim_config) */
  int32_t cam_width, cam_height;   /* each at least 2 * window_size + 1 */
  int32_t proj_width, proj_height; /* the reference: 1080 x 1920 */
  int32_t window_size;             /* 0 = the reference's 3; odd, at most 7 */
  int32_t max_iter;                /* 0 = scipy's 500; 1 .. 65535 (the solver evaluates at least twice) */
  int32_t reserved;
  double xatol;                    /* 0 = scipy's 1e-5; positive and finite */
  double p1_03;                    /* P1[0, 3] of the rectification; finite and non-zero (a negative one inverts every bound) */
  double cam_K[9], cam_D[5];       /* row-major K; k1 k2 p1 p2 k3 */
  double proj_K[9], proj_D[5];
  double Rt[12];                   /* R' row-major, then t: camera frame -> projector frame */
  const float* proj_surface;       /* host, [proj_height][proj_width]: get_projector_time_surface (:94-101), unrectified */
} xm_esl_optim_config;             /* the surface is copied to the device; the caller keeps ownership */
typedef struct xm_esl_optim_stats {
  uint64_t n_optimised;  /* pixels minimised                                                                */
  uint64_t n_evals;      /* cost evaluations over them                                                      */
  uint64_t n_hit_limit;  /* ... of which left the solver through num >= max_iter                            */
  uint64_t n_bad_bounds; /* pixels inside the border with d0 > 0 whose bounds scipy would refuse: written 0 */
  double lo, hi;         /* extrema of the non-zero pixels (0, 0 for an all-zero surface)                   */
} xm_esl_optim_stats;
int xm_esl_optim_create(int device, const xm_esl_optim_config* cfg, xm_esl_optim** out);
void xm_esl_optim_destroy(xm_esl_optim* e);
/* surfaces: [n_surfaces][cam_height][cam_width], XM_T_FLOAT32 or XM_T_FLOAT64.  depth_init, depth_optim_out: f32, the same shape.
 * nfev_out (may be NULL): u16, the same shape: the evaluations of each pixel, 0 where none ran.  stats_out (may be NULL):
 * xm_esl_optim_stats[n_surfaces].  mem == XM_MEM_HOST: every pointer is host memory; XM_MEM_DEVICE: every pointer is device memory
 * of the object's device -- depth_init may be the buffer xm_esl_init_time_surfaces has just filled.  Synchronous in both.  Scratch
 * is allocated by the first call and grown when a larger group arrives; a group of any size is accepted.  XM_ERR_INVALID: a dtype
 * other than the two float types, n_surfaces <= 0. */
int xm_esl_optim_time_surfaces(xm_esl_optim* e, const void* surfaces, int dtype, int n_surfaces, int mem, const float* depth_init,
                               float* depth_optim_out, uint16_t* nfev_out, xm_esl_optim_stats* stats_out);

/* ---- ESL ground truth: the bilateral filter and the TV denoiser behind the depth optimisation, on the device ---------------------
 * What python/eval/compute_depth_esl.py:243-244 computes for a GROUP of depth_optim maps (f32 [n][height][width]) in one device
 * call: cv2.bilateralFilter(depth_optim, 5, 3, 3), then esl_utilities.py:194-224 denoise_tv(., mu = 0.5) -> the maps the
 * reference stores as esl/depth_optim_filtered (f64: pylops returns float64).  This text is the contract of both stages;
 * tests/esl_filter_ref.py states it in NumPy.
 * Stage 1 (float32 throughout, no contraction; OpenCV's 32F bilateral filter as documented):
 *   lo / hi = the map's extrema.  hi - lo < FLT_EPSILON: the map is copied.  Otherwise radius = d / 2, and the taps are the (i, j)
 *   in [-radius, radius]^2 with sqrt(i*i + j*j) <= radius (13 for d = 5) in raster order, the border BORDER_REFLECT_101; space
 *   weight ws = (float)exp(r*r * -0.5 / sigma_space^2); len = (float)(hi - lo), scale = 4096 / len; colour table of 4098 entries,
 *   lut[i] = (float)exp(t*t * -0.5 / sigma_color^2) with t = (double)((float)i / scale), taken in float64; per tap a = |v - v0| *
 *   scale, idx = (int)a, w = ws * (lut[idx] + (a - idx) * (lut[idx + 1] - lut[idx])), sum = sum + v * w, wsum = wsum + w; out =
 *   sum / wsum.  |v - v0| = len reaches lut[4097].  Where OpenCV's code may differ from this text (UNPINNED):
 *   its builds take the centre tap first with weight 1 and vectorise the sums with fused multiply-adds, which moves last bits only.
 * Stage 2 (float64 throughout): split Bregman as pylops 1.18 runs it for Op = Identity and two L1 regularisers, around scipy
 *   1.15's lsqr.  With N = height * width, the flat index k = row * width + col, and Hs = HEIGHT (the reference hands pylops
 *   dims = (ny, nx) with nx, ny = y.shape, so the image is differenced as if it were width x height):
 *     D0 x[k] = x[k] - x[k - Hs] for k >= Hs, else 0;  D1 x[k] = x[k] - x[k - 1] for k % Hs != 0, else 0;
 *     A = [I; e0 D0; e1 D1], e_i = sqrt(lambda_i / 2) / sqrt(mu / 2);  A v = [v; e0 (D0 v); e1 (D1 v)];
 *     A'u = (u0 + e0 (D0'u1)) + e1 (D1'u2);
 *     x = 0, xold = inf, b_i = d_i = 0; while norm(x - xold) > tol and it < niter_outer: xold = x; niter_inner times {
 *     rhs = [y; e_i (d_i - b_i)] - A x; x = x + lsqr(A, rhs, damp, atol = btol = 1e-6, conlim = 1e8, iter_lim)[0];
 *     d_i = max(|D_i x + b_i| - lambda_i, 0) * sign(D_i x + b_i) }; b_i = b_i + tau (D_i x - d_i).
 *   lsqr is scipy's restated operation for operation: _sym_ortho, the damping rotation, the anorm / ddnorm / xnorm / acond
 *   recurrences, all seven stopping tests in their order, the beta > 0 and alfa > 0 guards and the arnorm == 0 return.  Every
 *   vector norm is a sum over fixed tiles of pixels in a fixed order: the result of a map depends neither on the group it arrives
 *   in nor on its neighbours there, and differs from a NumPy run by the summation order alone (about 1e-14 on the maps of the tests;
 *   the trip counts are equal).
 * PINNED (golden G14): the reference's own denoise_tv -- its call, the dims swap, every parameter -- on scipy's own lsqr.
 * UNPINNED: pylops' loop, stacking, stencil and threshold; its float32 operator dtype; cv2's bilateral filter.
 * Defined, not errors: an all-zero map (lsqr returns x = 0; one outer iteration) and a constant map (two).  NaN / +-inf maps are out
 * of contract; they neither fault nor index outside a table.  No kernel has atomics or waits for another block; the host issues a
 * fixed schedule of launches -- 3 + niter_outer * niter_inner * (2 * iter_lim + 4) + 1 for both stages -- and reads nothing back
 * inside it.  No xm_handle is involved; an object serves one thread at a time. */
#define XM_ESL_FILTER_NO_BILATERAL 1u /* stage 2 alone: it takes the f32 input cast to f64 */
#define XM_ESL_FILTER_NO_TV 2u        /* stage 1 alone: filtered_out is its f32 result cast to f64 */
typedef struct xm_esl_filter xm_esl_filter;
typedef struct xm_esl_filter_config {
  uint32_t struct_size;         /* sizeof(xm_esl_filter_config) */
  int32_t width, height;        /* of a map; width * height at most 2^30 */
  uint32_t flags;               /* XM_ESL_FILTER_* */
  int32_t d;                    /* 0 = the reference's 5; 1, 3 or 5 */
  int32_t niter_outer;          /* 0 = 20; at most 255 */
  int32_t niter_inner;          /* 0 = 10; at most 255 */
  int32_t iter_lim;             /* 0 = 5; at most 254 (a trip count is a u8, 0xFF = no call) */
  double sigma_color, sigma_space; /* 0 = 3, 3; positive */
  double mu, lambda0, lambda1;  /* 0 = 0.5, 0.1, 0.1; positive */
  double tol, tau, damp;        /* 0 = 1e-4, 1, 1e-4; non-negative */
} xm_esl_filter_config;
typedef struct xm_esl_filter_stats {
  double lo, hi;            /* extrema of the input map                                           */
  double final_norm;        /* norm(x - xold) behind the last outer iteration that ran            */
  uint32_t n_outer;         /* outer iterations run                                               */
  uint32_t n_lsqr;          /* lsqr calls                                                         */
  uint32_t sum_itn;         /* ... their iterations                                               */
  uint32_t reserved;
  uint32_t istop_count[8];  /* ... by scipy's istop                                               */
} xm_esl_filter_stats;
int xm_esl_filter_create(int device, const xm_esl_filter_config* cfg, xm_esl_filter** out);
void xm_esl_filter_destroy(xm_esl_filter* e);
/* depth_optim: f32 [n_maps][height][width].  filtered_out: f64, the same shape.  bilateral_out (may be NULL): f32, the same shape,
 * stage 1's result.  trips_out (may be NULL): u8 [n_maps][niter_outer * niter_inner], lsqr's itn of every inner call in order, 0xFF
 * where none ran.  stats_out (may be NULL): xm_esl_filter_stats[n_maps].  mem as for xm_esl_optim_time_surfaces: with
 * XM_MEM_DEVICE depth_optim may be the buffer xm_esl_optim_time_surfaces has just filled.  Synchronous.  Scratch (about 13
 * float64 per pixel of the group) is allocated by the first call and grown.  At most 65535 maps per call (XM_ERR_TOO_MANY). */
int xm_esl_filter_maps(xm_esl_filter* e, const float* depth_optim, int n_maps, int mem, double* filtered_out, float* bilateral_out,
                       uint8_t* trips_out, xm_esl_filter_stats* stats_out);
/* kernel launches of the object's last call */
int xm_esl_filter_last_launches(xm_esl_filter* e, uint64_t* out);

/* ---- MC3D: the other baseline of the reference's evaluation table, on the device -------------------------------------------------
 * What python/eval/mc3d_baseline.py:40-78,129-140 computes, for a GROUP of camera time surfaces in one device call.  With
 * (W, H) = (proj_width, proj_height), per surface (used as stored: no normalisation):
 *   1. v = median of the 3 x 3 neighbourhood, borders replicated, the exact median of nine (cv2.medianBlur(., 3): UNPINNED against
 *      a cv2 run), taken in the surface's own type; XM_MC3D_NO_BLUR: v = the pixel itself;
 *   2. for every pixel with v > 0: (xc, yc) = cam_map[i][j]; dropped unless 0 < xc < rect_x_limit and 0 < yc < rect_y_limit;
 *      id = (int)(W * H * v), the product a float32 multiply for XM_T_FLOAT32 and a float64 multiply for XM_T_FLOAT64; dropped if
 *      id >= W * H (v >= 1, +inf); proj_x = id / H, proj_y = id % H; over y in [max(proj_y - nc, 0), min(proj_y + nc, H)), with
 *      (xp, yp) = proj_map[y][proj_x], the FIRST minimum of |yc - yp| wins; it is accepted if <= max_row_diff; then
 *      disp = xp - xc, stored only if > 0.  Only that one candidate is ever examined;
 *   3. depth = (float)(p1_03 / (double)disp), 0 where the disparity is 0 (never inf).
 * The maps are int32 pairs, the reference's int(map[..]) -- truncation toward zero -- done by the table builder
 * (x_maps_amd/mc3d.py mc3d_int_maps).  XM_MC3D_POISON in either component marks a NaN / +-inf entry: in cam_map it drops the
 * pixel, in proj_map INSIDE a pixel's window it drops that pixel (the reference's swallowed exception), outside it has no effect.
 * Finite entries beyond +-2^30 saturate there (the builder's, and again at create).  That cannot change a result: the rect limits
 * and max_row_diff are at most 2^29, so xc and yc lie below 2^29; a camera entry at the bound fails the limits either way; a
 * projector yp at or beyond +-2^30 is more than 2^29 away from every admissible yc, so its cost is never <= max_row_diff; and an
 * xp there gives a disparity that is negative or beyond 2^29 either way, and
 * a disparity above 65535 cannot be stored as u16; it is DEFINED as 0 (depth 0) and counted in n_disp_overflow.
 * An all-zero surface gives zero maps and zero counts (the reference skips it); not an error.  NaN surfaces are out of contract;
 * they neither fault nor index outside a table.  No kernel has atomics or waits for another block.  No xm_handle is involved;
 * an object serves one thread at a time. */
#define XM_MC3D_POISON INT32_MIN
#define XM_MC3D_NO_BLUR 1
typedef struct xm_mc3d xm_mc3d;
typedef struct xm_mc3d_config {
  uint32_t struct_size; /* sizeof(xm_mc3d_config) */
  int32_t cam_width, cam_height;
  int32_t proj_width, proj_height;    /* the reference: 1080 x 1920; proj_width * proj_height <= 2^24 */
  int32_t nc;                         /* 0 = (int)(proj_height / 15); invalid: nc < 0, 2 * nc > proj_height */
  int32_t max_row_diff;               /* 0 = 50; invalid: < 0, > 2^29, or a search key beyond 32 bits (mc3d_key_fits) */
  int32_t rect_x_limit, rect_y_limit; /* 0, 0 = 3 * proj_height, 3 * proj_width: swapped, as the reference; each 1 .. 2^29 */
  int32_t reserved;
  double p1_03;                       /* P1[0, 3] of the rectification (either sign; 0 gives zero depth) */
  const int32_t* cam_map;             /* host, [cam_height][cam_width][2]   (x, y), truncated toward zero */
  const int32_t* proj_map;            /* host, [proj_height][proj_width][2] (x, y), the reference's orientation */
} xm_mc3d_config;                     /* both tables are copied to the device (the projector's by column); the caller keeps ownership */
typedef struct xm_mc3d_stats {
  uint64_t n_nonzero;       /* pixels != 0, before the blur                                            */
  uint64_t n_positive;      /* pixels with v > 0, after it                                             */
  uint64_t n_in_rect;       /* ... whose camera entry passes the rect limits                           */
  uint64_t n_out_of_range;  /* ... of which id >= W * H                                                */
  uint64_t n_poisoned;      /* searched pixels whose window holds a poisoned entry                     */
  uint64_t n_matched;       /* pixels with a stored disparity (1 .. 65535)                             */
  uint64_t n_disp_overflow; /* accepted winners whose disparity exceeds 65535: stored as 0             */
} xm_mc3d_stats;
int xm_mc3d_create(int device, const xm_mc3d_config* cfg, xm_mc3d** out);
void xm_mc3d_destroy(xm_mc3d* m);
/* surfaces: [n_surfaces][cam_height][cam_width], XM_T_FLOAT32 or XM_T_FLOAT64.  depth_out: f32, the same shape.  disp_out (may be
 * NULL): u16, the same shape.  stats_out (may be NULL): xm_mc3d_stats[n_surfaces].  flags: 0 or XM_MC3D_NO_BLUR.  mem ==
 * XM_MEM_HOST: every pointer is host memory; XM_MEM_DEVICE: every pointer is device memory of the object's device.  Synchronous
 * in both.  Scratch is allocated by the first call and grown when a larger group arrives.  XM_ERR_INVALID: a dtype other than the
 * two float types, n_surfaces <= 0, unknown flags. */
int xm_mc3d_time_surfaces(xm_mc3d* m, const void* surfaces, int dtype, int n_surfaces, int mem, int flags, float* depth_out,
                          uint16_t* disp_out, xm_mc3d_stats* stats_out);

/* ---- the evaluation table's scorer: a sequence's depth maps -> the cells of the reference's Table 1 ------------------------------
 * python/eval/create_evaluation_table.py:14-62,121-163 with esl_utilities.py:153-175 (combine_mc3d), in one device call.  All
 * maps are f32 [height][width]; min_depth / max_depth compare as float32 (the reference's 20 / 120).
 *
 *   combine(stack) : per pixel, maps in index order: d = v; if (d >= max_depth) d = 0; if (d <= min_depth) d = 0; acc += d (float32);
 *                    cnt += d > 0.  mean = cnt == 0 ? 0 : acc / cnt, the correctly rounded float32 quotient.  (A NaN follows
 *                    from these comparisons: acc turns NaN, cnt is untouched.)  combined = the 3 x 3 median of mean, borders
 *                    replicated, the exact rank-4 value of the nine -- cv2.medianBlur(., 3) for finite values; a NaN in the
 *                    window is unspecified.  avg_depth = sum(combined[combined > 0]) / #(combined > 0) in float64 (0 when no
 *                    pixel is positive).
 *   score          : mask = combine(gt stack).  Per scan s: g = load_and_filter(gt[s], mask) (:57-62: v >= max_depth -> 0,
 *                    v <= min_depth -> 0, mask == 0 -> 0).  A method's row: e = load_and_filter(est[m][s], mask); its "1 sec" row:
 *                    e = combine(est[m]), NOT filtered, the same map for every scan (:128,:151).  Then xm_eval_stats'
 *                    arithmetic on (e, g): float32 difference and square, (double)|d| < margin with margin = 0.01 * sum(g[g > 0])
 *                    / #(g > 0) in float64 (NaN when no g > 0), the thresholds 1 / 5 / 10, float64 sums.
 * Every sum is made of per-tile partial sums folded in one fixed order: no atomics, no block that waits for another, a fixed
 * schedule of launches with no readback.  A cell's bits therefore depend on the maps alone -- not on the run, on XM_MEM_HOST or
 * XM_MEM_DEVICE, on the alignment of a pointer or on which other methods are in the call.  (xm_eval_stats, which accumulates
 * with atomics, agrees to the last few bits of margin and RMSE and, where no pixel's error sits on the margin, in every count.)
 * No xm_handle is involved; an object serves one thread at a time.  Synchronous. */
typedef struct xm_eval_table_config { uint32_t struct_size; int32_t height, width; float min_depth, max_depth; uint32_t reserved; } xm_eval_table_config;
typedef struct xm_eval_sums { double sum_gt, sum_sq; uint64_t n_gt_pos, n_gt_zero, n_close, n_valid, n1, n5, n10; } xm_eval_sums;
typedef struct xm_eval_table xm_eval_table;
/* XM_ERR_INVALID: NULL, struct_size mismatch, a non-positive dimension, height beyond 65535 * 8 */
int xm_eval_table_create(int device, const xm_eval_table_config* cfg, xm_eval_table** out);
void xm_eval_table_destroy(xm_eval_table* e);
/* maps [n_maps][h][w] f32, host or device by `mem`; combined_out / mean_out (before the median; nullable) follow `mem`;
   avg_depth_out (nullable) is host memory */
int xm_eval_table_combine(xm_eval_table* e, const float* maps, int n_maps, int mem, float* combined_out, float* mean_out,
                          double* avg_depth_out);
/* gt [n_scans][h][w]; est: n_methods pointers (a host array) to [n_scans][h][w]; bit m of one_sec_mask adds a "1 sec" row for
   method m.  Rows: methods 0..M-1, then the 1-sec rows by ascending m.  results_out / sums_out (nullable) are host arrays
   [rows][n_scans]; mask_out (nullable, follows `mem`) is the combined ground truth; avg_depth_out (nullable, host) its mean depth.
   The six floats of a result come from its sums through the same expressions as xm_eval_stats'.  1 <= n_methods <= 8; the bits
   of one_sec_mask lie below n_methods; n_scans >= 1: otherwise, and for a NULL gt / est / est[m], XM_ERR_INVALID before any GPU
   work.  XM_ERR_TOO_MANY: more than 65535 scans, or n_scans * h * w >= 2^40. */
int xm_eval_table_score(xm_eval_table* e, const float* gt, const float* const* est, int n_methods, uint32_t one_sec_mask,
                        int n_scans, int mem, xm_eval_result* results_out, xm_eval_sums* sums_out, float* mask_out,
                        double* avg_depth_out);

/* ---- projector time-map calibration: a white-frame recording's camera time surfaces -> the projector-space time map --------------
 * The paper's recipe (section 3.3, "Time map calibration"): project a white image onto a plane, average several normalised camera
 * time maps per pixel, find the projected frame's corners in a binary map, warp the quadrilateral to the projector's width x
 * height with a projective transformation, interpolate missing values linearly between actual lines.  The reference ships no
 * code for it: the arithmetic is THIS BUILD'S DEFINITION, pinned bit for bit to the NumPy oracle of tests/time_cal_cases.py.
 * Float64 throughout, every expression in the order written, unfused; csrc/xmaps_timecal.hpp has the kernels.
 *
 *   accumulate : per surface lo / hi / nnz over its non-zero entries (as xm_process_time_surfaces takes them); a surface without
 *                two distinct non-zero values is skipped and counted.  Otherwise per pixel with v != 0:
 *                sum += max((f64(v) - lo) / (hi - lo), 0), cnt += 1.  Surfaces are taken in order -- inside a call by index, across
 *                calls in call order -- by the one thread that owns the pixel: the sums depend on the sequence of surfaces only.
 *   mean       : valid = cnt >= min_count (min_count >= 1); mean = valid ? sum / f64(cnt) : 0.
 *   corners    : core = valid on the whole 3 x 3 neighbourhood (an image-border pixel is never core).  Over the core pixels
 *                TL = argmin(x + y), TR = argmax(x - y), BR = argmax(x + y), BL = argmin(x - y), ties to the smallest raster index.
 *                XM_ERR_INVALID (xm_last_error names the reason): no core pixel; two corners coincide; TL -> TR -> BR -> BL is not
 *                strictly convex (the integer cross products of consecutive edges do not all have one sign).
 *   warp       : h maps a projector pixel (u, v) to a camera position: X = h0 u + h1 v + h2, Y = h3 u + h4 v + h5,
 *                D = h6 u + h7 v + h8, x = X / D, y = Y / D, x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0.  Taps (x0, y0),
 *                (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy; a tap outside the image
 *                or not valid has weight 0.  den = the weights, num = the products w * mean, both summed in tap order.  den > 0: the
 *                value is num / den and the pixel is present; otherwise 0 and missing (so is NaN, D = 0, a position beyond the image).
 *   fill       : along each projector row (a projector line is a column).  A missing pixel at u between the nearest present
 *                u_l < u < u_r gets m_l + (m_r - m_l) * ((u - u_l) / (u_r - u_l)); with a present pixel on one side only, that
 *                side's value; a row with no present pixel stays 0 and counts as one in n_unfilled.  One cast to float32.
 *
 * An object serves one thread at a time; every call is synchronous.  mem == XM_MEM_HOST: every array pointer is host memory,
 * XM_MEM_DEVICE: device memory of the object's device; stats and h are host memory always. */
typedef struct xm_timecal xm_timecal;
typedef struct xm_timecal_stats {
  uint64_t n_added;    /* surfaces handed in since create / reset, the skipped ones included */
  uint64_t n_skipped;  /* ... of which not normalisable                                      */
  uint32_t n_valid, n_core;      /* xm_timecal_mean / _set_mean                              */
  int32_t corners[4][2];         /* TL, TR, BR, BL as (x, y); -1 where there is no core pixel */
  uint32_t n_missing, n_unfilled; /* xm_timecal_warp: missing pixels before the fill; rows without a present pixel */
} xm_timecal_stats;
/* XM_ERR_INVALID: NULL, a non-positive side, cam_width * cam_height >= 2^31 */
int xm_timecal_create(int device, int cam_width, int cam_height, xm_timecal** out);
void xm_timecal_destroy(xm_timecal* tc);
/* the accumulators and counters back to zero; the state of xm_timecal_mean is forgotten */
int xm_timecal_reset(xm_timecal* tc);
/* surfaces: [n][cam_height][cam_width], XM_T_FLOAT32 or XM_T_FLOAT64, 0 = no event.  At most 65535 surfaces per call. */
int xm_timecal_add_surfaces(xm_timecal* tc, const void* surfaces, int dtype, int n, int mem);
/* the counters alone (either may be NULL) */
int xm_timecal_counts(xm_timecal* tc, uint64_t* n_added, uint64_t* n_skipped);
/* the device time of the kernels, from HIP events around each launch of the last call that ran it, in ms: k_surf_extrema,
 * k_tcal_accumulate (the last xm_timecal_add_surfaces), k_tcal_mean, k_tcal_corners, k_tcal_warp, k_tcal_fill */
int xm_timecal_kernel_ms(xm_timecal* tc, float ms[6]);
/* mean_out: f64 [cam_height][cam_width], valid_out: u8, the same shape; either may be NULL, and so may stats.  The corner errors
 * are reported here, after the outputs and stats have been written: the mean and the mask stay in the object, so that
 * xm_timecal_warp can follow with an h from corners of the caller's own.  XM_ERR_INVALID also for min_count == 0. */
int xm_timecal_mean(xm_timecal* tc, uint32_t min_count, double* mean_out, uint8_t* valid_out, int mem, xm_timecal_stats* stats);
/* the state xm_timecal_mean leaves, from the caller's arrays instead (mean must be 0 where valid is 0): the warp as a stage of its
 * own.  Corners, errors and stats as xm_timecal_mean. */
int xm_timecal_set_mean(xm_timecal* tc, const double* mean, const uint8_t* valid, int mem, xm_timecal_stats* stats);
/* warp and fill on the state left by the last xm_timecal_mean / _set_mean (XM_ERR_INVALID without one).  time_map_out: f32
 * [proj_height][proj_width]; present_out (may be NULL): u8, the mask before the fill.  Sides in 1 .. 2^24. */
int xm_timecal_warp(xm_timecal* tc, const double h[9], int proj_width, int proj_height, float* time_map_out, uint8_t* present_out,
                    int mem, xm_timecal_stats* stats);

/* ---- pinned host memory for XM_MEM_HOST_PINNED ------------------------------------------------------------- */
int xm_host_alloc(xm_handle* h, size_t bytes, void** out);
int xm_host_free(xm_handle* h, void* p);

/* ---- small device-memory helpers so that a host without torch can stage buffers ------------------- */
int xm_dev_alloc(xm_handle* h, size_t bytes, void** out);
int xm_dev_free(xm_handle* h, void* p);
int xm_dev_upload(xm_handle* h, void* dst_dev, const void* src_host, size_t bytes);
int xm_dev_download(xm_handle* h, void* dst_host, const void* src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* XMAPS_H */
