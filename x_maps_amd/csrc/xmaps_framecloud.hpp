// xmaps_framecloud.hpp -- gfx950 device code of the frame -> point cloud entry (xm_frames_to_point_clouds, and the same kernels as
// a stage of the device ingest: xm_ingest_set_cloud_output): a GROUP of frames of EventCD records -> one per-event point cloud per
// frame, the reference's construct_point_cloud(xr_f32[mask], yr_f32[mask], disparity) (cam_proj_calibration.py:319-331 as
// eval/compute_depth_x_maps.py:99-122 applies it) on the live frame's own int64 stamps and X-map columns.  include/xmaps.h states
// the definition; nothing in it is this build's own.
//
// Per launch sequence (at most FC_GROUP frames, grid = blocks x frames), every dependency between blocks a kernel boundary:
//   C0 k_fc_extrema  per event: does it exist (polarity)?  Extrema of t over ALL existing events (those left out later included)
//                    and their count: reduced per block, then ONE 64-bit integer atomic per value and block into the frame's
//                    accumulator (xmaps_frameacc.hpp: all-zero words are neutral for every field)
//   C1 k_fc_events   per existing event: A1 (packed int16 LUT) -> A2 (TimeNorm<long long> + event_disparity_col: the code K1 runs)
//                    -> a 2-byte code, disparity + 1 of an inlier, else 0; per 64 consecutive events (one wave instruction) the
//                    counts of inliers and of left-out events (off the sensor, or a column outside the X-map).  Every code and every
//                    count of the frame is written: nothing of an earlier call is ever read
//   C2 k_fc_scan     one block per frame: exclusive scan of the frame's 64-event counts (stream order) + the frame's statistics;
//                    leaves the accumulator ZERO
//   C3 k_fc_points   stable compaction in stream order = the order of xr_f[mask]: ballot + mbcnt inside the 64 events, the scanned
//                    offset in front; gather of the two float rectify maps; point_from_disparity (xmaps_stage.hpp, unchanged);
//                    three plain 4-byte stores per row.  Rows past the frame's inliers are not touched: no clear of the output
//   C4 k_fc_publish  (ingest only) the statistics and the ring entry's tag into pinned host memory, behind C3
// No floating-point atomic anywhere; no block waits for or spins on another block of its launch.  A frame longer than the grid
// covers (FC_CHUNK events per block, at most max_chunk_blocks blocks: "XM_FC_MAX_BLOCKS") takes further trips of a chunk loop; the
// mapping event -> (wave, lane) is the same in C1 and C3 on every trip, so the 64 events of one count are the 64 lanes of one wave
// instruction in both.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_frameacc.hpp"
#include "xmaps_stage.hpp"  // Mat4f, point_from_disparity

namespace xm {

constexpr int FC_THREADS = FRAME_THREADS;      // threads per block (C0, C1, C3)
constexpr int FC_EPT = FRAME_EPT;              // events per thread
constexpr int FC_CHUNK = FRAME_CHUNK;          // events per block and trip of its chunk loop
constexpr int FC_GROUP = FRAME_GROUP;          // frames per launch sequence
constexpr int FC_SCAN_BLOCK = 1024;            // C2

struct FcAcc {   // device, one per frame of a sequence; all zero between calls
  u64 min_enc;   // max over the existing events of ~(t ^ 2^63)
  u64 max_enc;   // max over the existing events of   t ^ 2^63
  u32 n_events;  // existing events (all of them, or those with p == 1)
  u32 pad[3];
};
static_assert(sizeof(FcAcc) == 32, "FcAcc layout");

struct FcStats {  // == xm_frame_cloud_stats (include/xmaps.h)
  u64 n_events, n_inliers, n_index_errors;
  long long t_min, t_max;
};

struct FcArgs {           // by value to the kernels
  const uint4* ev;        // the record array (group entry) ...
  u64 first[FC_GROUP];    // ... frame f = records [first[f], first[f] + n[f]); its codes and cloud rows start at first[f] too
  u32 n[FC_GROUP];
  u32 seg0[FC_GROUP];     // the frame's first 64-event count
  const FrameDesc* desc;  // ingest: ONE frame, described on the device (aos, n, valid); ev / first / n / seg0 unused
  u32 cap;                // ingest: the events the scratch holds (a cut frame never has more; the kernels clamp to it)
  u32 max_rows;           // rows a frame's cloud may hold (ingest: max_points; group entry: no limit)
  DevTables tb;
  const float *mapx, *mapy;  // float rectify maps [cam_h][cam_w]
  Mat4f Q;
  FcAcc* acc;             // [frames of the sequence]
  uint16_t* code;         // per event
  uint2* cnt;             // per 64 events: {inliers, left out}
  u32* off;               // per 64 events: rows of the frame in front of them (C2)
  FcStats* stats;         // [frames of the sequence]
  float* cloud;           // [events][3]; NULL: statistics only (C3 is not launched)
  u64* tag;               // ingest: the ring entry's tag in pinned host memory (C0 clears it, C4 sets it), else NULL
  u64 tag_value;
  FcStats* host_stats;    // ingest: the ring entry's statistics in pinned host memory (C4)
  int use_polarity;
  u32 max_chunk_blocks;   // grid.x of C0 / C1 / C3 is at most this
};

struct FcFrameRef {
  const uint4* ev;
  u64 n, base;  // events; index of the frame's first code / cloud row
  u32 seg0;
};
__device__ inline FcFrameRef fc_frame(const FcArgs& a, u32 f) {
  if (a.desc) {
    if (!a.desc->valid) return FcFrameRef{nullptr, 0, 0, 0};
    const u64 n = a.desc->n;
    return FcFrameRef{a.desc->aos, n < a.cap ? n : a.cap, 0, 0};
  }
  return FcFrameRef{a.ev + a.first[f], a.n[f], a.first[f], a.seg0[f]};
}

// C0 ------------------------------------------------------------------------------------------------------------------------
// (k_fs_events without the winner map; both written out: see xmaps_frameacc.hpp)
__global__ __launch_bounds__(FC_THREADS) void k_fc_extrema(FcArgs a) {
  __shared__ u64 s_min[FC_THREADS / 64], s_max[FC_THREADS / 64];
  __shared__ u32 s_n[FC_THREADS / 64];
  const u32 f = blockIdx.y, tid = threadIdx.x;
  frame_tag_clear(a.tag);  // (C3 of this frame rewrites the ring entry)
  const FcFrameRef fr = fc_frame(a, f);
  u64 mn = 0, mx = 0;
  u32 n_ev = 0;
  for (u64 c0 = (u64)blockIdx.x * FC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * FC_CHUNK) {  // (block-uniform)
    uint4 r[FC_EPT];
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 i = c0 + (u64)k * FC_THREADS + tid;
      r[k] = i < fr.n ? fr.ev[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 i = c0 + (u64)k * FC_THREADS + tid;
      if (i >= fr.n || !frame_exists(a.use_polarity, r[k])) continue;
      const u64 u = frame_enc(rec_t<long long>(r[k]));
      mn = ~u > mn ? ~u : mn;
      mx = u > mx ? u : mx;
      n_ev += 1;
    }
  }
  mn = wave_max_u64(mn);
  mx = wave_max_u64(mx);
  n_ev = wave_sum_u32(n_ev);
  const u32 wave = tid >> 6;
  if ((tid & 63) == 0) s_min[wave] = mn, s_max[wave] = mx, s_n[wave] = n_ev;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < FC_THREADS / 64; ++w) {
      mn = s_min[w] > mn ? s_min[w] : mn;
      mx = s_max[w] > mx ? s_max[w] : mx;
      n_ev += s_n[w];
    }
    if (n_ev) {
      FcAcc* acc = a.acc + f;
      __hip_atomic_fetch_max(&acc->min_enc, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(&acc->max_enc, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&acc->n_events, n_ev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// C1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_THREADS) void k_fc_events(FcArgs a) {
  const u32 f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const FcFrameRef fr = fc_frame(a, f);
  const FcAcc acc = a.acc[f];  // (C0 has finished: plain loads)
  const bool any = acc.n_events != 0;
  const TimeNorm<long long> tn(any ? frame_dec(~acc.min_enc) : 0, any ? frame_dec(acc.max_enc) : 0, a.tb.t_px_scale);
  uint16_t* code = a.code + fr.base;
  uint2* cnt = a.cnt + fr.seg0;
  for (u64 c0 = (u64)blockIdx.x * FC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * FC_CHUNK) {  // (block-uniform)
    uint4 r[FC_EPT];
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 i = c0 + (u64)k * FC_THREADS + tid;
      r[k] = i < fr.n ? fr.ev[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 w0 = c0 + (u64)k * FC_THREADS + (tid & ~63u), i = w0 + lane;  // w0: the wave's first event, a multiple of 64
      if (w0 >= fr.n) break;                                                    // (wave-uniform)
      bool inl = false, oob = false;
      int dsp = 0;
      if (i < fr.n && frame_exists(a.use_polarity, r[k])) {
        const EventResult e = event_disparity_col(a.tb, tn.column(rec_t<long long>(r[k])), rec_x(r[k]), rec_y(r[k]), oob);
        inl = e.inlier;
        dsp = e.disp;
      }
      const u64 b_in = __ballot(inl), b_oob = __ballot(oob);
      if (i < fr.n) code[i] = inl ? (uint16_t)(dsp + 1) : (uint16_t)0;
      if (lane == 0) cnt[w0 >> 6] = make_uint2((u32)__popcll(b_in), (u32)__popcll(b_oob));
    }
  }
}

// C2 ------------------------------------------------------------------------------------------------------------------------
// one block per frame: off = exclusive scan of the inlier counts of the frame's ceil(n / 64) segments, the frame's statistics
__global__ __launch_bounds__(FC_SCAN_BLOCK) void k_fc_scan(FcArgs a) {
  __shared__ u32 s_w[FC_SCAN_BLOCK / 64], s_oob[FC_SCAN_BLOCK / 64];
  const u32 f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FcFrameRef fr = fc_frame(a, f);
  const u32 n_seg = (u32)((fr.n + 63) >> 6);
  const uint2* cnt = a.cnt + fr.seg0;
  u32* off = a.off + fr.seg0;
  const u32 ipt = (n_seg + FC_SCAN_BLOCK - 1) / FC_SCAN_BLOCK;  // consecutive segments per thread
  const u32 first = tid * ipt < n_seg ? tid * ipt : n_seg, last = first + ipt < n_seg ? first + ipt : n_seg;
  u32 sum = 0, oob = 0;
  for (u32 i = first; i < last; ++i) {
    const uint2 c = cnt[i];
    sum += c.x;
    oob += c.y;
  }
  u32 incl = sum;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 up = __shfl_up(incl, o, 64);
    if (lane >= (u32)o) incl += up;
  }
  oob = wave_sum_u32(oob);
  if (lane == 63) s_w[wave] = incl;
  if (lane == 0) s_oob[wave] = oob;
  __syncthreads();
  u32 before = 0, total = 0, oob_total = 0;
#pragma unroll
  for (int w = 0; w < FC_SCAN_BLOCK / 64; ++w) {
    before += (u32)w < wave ? s_w[w] : 0u;
    total += s_w[w];
    oob_total += s_oob[w];
  }
  u32 run = before + incl - sum;
  for (u32 i = first; i < last; ++i) {
    off[i] = run;
    run += cnt[i].x;
  }
  if (tid == 0) {
    FcAcc* acc = a.acc + f;
    const FcAcc v = *acc;
    *acc = FcAcc{0, 0, 0, {0, 0, 0}};  // its last reader leaves it zero
    FcStats s{0, 0, 0, 0, 0};
    if (v.n_events) s = FcStats{v.n_events, total, oob_total, frame_dec(~v.min_enc), frame_dec(v.max_enc)};
    a.stats[f] = s;
  }
}

// C3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_THREADS) void k_fc_points(FcArgs a) {
  const u32 f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const FcFrameRef fr = fc_frame(a, f);
  const uint16_t* code = a.code + fr.base;
  const u32* off = a.off + fr.seg0;
  float* cloud = a.cloud + fr.base * 3;
  for (u64 c0 = (u64)blockIdx.x * FC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * FC_CHUNK) {  // (block-uniform)
    u32 c[FC_EPT];
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 i = c0 + (u64)k * FC_THREADS + tid;
      c[k] = i < fr.n ? (u32)code[i] : 0u;
    }
#pragma unroll
    for (int k = 0; k < FC_EPT; ++k) {
      const u64 w0 = c0 + (u64)k * FC_THREADS + (tid & ~63u), i = w0 + lane;
      if (w0 >= fr.n) break;  // (wave-uniform)
      const u64 bal = __ballot(c[k] != 0);
      if (c[k] == 0) continue;
      const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
      const u32 row = off[w0 >> 6] + rank;  // < n: at most one row per event
      if (row >= a.max_rows) continue;      // (ingest: the first max_points rows in stream order are kept)
      const u32 xy = *(const u32*)(fr.ev + i);  // the record's x | y << 16 alone; an inlier lies on the sensor (C1)
      const u32 px = (xy >> 16) * (u32)a.tb.cam_w + (xy & 0xffffu);
      float p[3];
      point_from_disparity(a.Q, a.mapx[px], a.mapy[px], (float)(int)(c[k] - 1u), p);
      float* out = cloud + (size_t)row * 3;
      out[0] = p[0];
      out[1] = p[1];
      out[2] = p[2];
    }
  }
}

// C4 ------------------------------------------------------------------------------------------------------------------------
// ingest: statistics, then the tag behind them, where xm_ingest_copy_cloud reads both without a copy
__global__ __launch_bounds__(64) void k_fc_publish(FcArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *a.host_stats = a.stats[0];
  __hip_atomic_store(a.tag, a.tag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace xm
