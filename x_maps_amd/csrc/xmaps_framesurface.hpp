// xmaps_framesurface.hpp -- gfx950 device code of the frame -> time surface entry (xm_frames_to_time_surfaces, and the same
// kernels as a stage of the device ingest: xm_ingest_set_surface_output): a GROUP of frames of EventCD records -> one camera time
// surface per frame, the image that holds per pixel the time of the event that fired there.  It is the inverse direction of
// xmaps_surface.hpp (surface -> events -> depth); this build's own definition (include/xmaps.h states it; the ESL dataset's own
// events-to-scan converter is not part of the reference: DESIGN.md section 5).
//
// Per group (grid = blocks x frames everywhere), three launches, every dependency between blocks a kernel boundary:
//   F0 k_fs_events  per event: does it exist (polarity), does it take part (x < cam_w, y < cam_h)?  Integer atomic max of
//                   (index + 1) -- XM_SURFACE_LAST -- or of ~index -- XM_SURFACE_FIRST -- into the frame's u32 winner map: stream
//                   order decides, never the time stamp, so the result is defined for any event order.  Frame extrema of t over
//                   ALL existing events, the counts of existing and left-out events: reduced per block, then ONE 64-bit integer
//                   atomic per value and block into the frame's accumulator
//   F1 k_fs_pixels  per cell: the winner's index -> its t out of the event array (an 8-byte gather) -> t - base + 1 in int64 -> ONE
//                   conversion to the output type (round to nearest even: a C++ integer -> floating conversion) -> one plain store;
//                   the same store writes the zeros of the cells without an event (no clear of the output).  It leaves every cell
//                   it read ZERO: the map is all zero between calls, as the frame filters' maps are.  Non-zero pixels per block ->
//                   one atomic add
//   F2 k_fs_finish  one thread per frame: accumulator -> statistics; leaves the accumulator ZERO
// Accumulator encoding (xmaps_frameacc.hpp, shared with xmaps_framecloud.hpp): all-zero words are neutral for every field, so
// nothing has to be initialised per call.
// No floating-point atomic anywhere: every result is a function of the frame alone.
//
// One winner map PER FRAME of the launch sequence (at most FS_GROUP frames, longer groups go out in several sequences that reuse the
// maps): the atomics of one frame spread over its own 1.2 MB (640 x 480), a sequence of 32 is 39 MB -- beyond one XCD's 4 MiB L2
// but inside the Infinity Cache, and the frames of a sequence run side by side instead of one after the other, which one map reused
// frame after frame would force (two dependent launches per frame).
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_frameacc.hpp"

namespace xm {

constexpr int FS_THREADS = FRAME_THREADS;           // threads per block (F0, F1)
constexpr int FS_EPT = FRAME_EPT;                   // F0: events per thread
constexpr int FS_CHUNK = FRAME_CHUNK;               // F0: events per block and trip of its chunk loop
constexpr int FS_CPT = 4;                           // F1: consecutive cells per thread (one 16-byte load of the map)
constexpr int FS_CELLS_PER_BLOCK = FS_THREADS * FS_CPT;
constexpr int FS_GROUP = FRAME_GROUP;               // frames per launch sequence
constexpr int FS_SELECT_LAST = 1, FS_SELECT_FIRST = 2;  // == XM_SURFACE_LAST / XM_SURFACE_FIRST

struct FsAcc {   // device, one per frame of a sequence; all zero between calls
  u64 min_enc;   // max over the existing events of ~(t ^ 2^63)
  u64 max_enc;   // max over the existing events of   t ^ 2^63
  u32 n_events;  // existing events (all of them, or those with p == 1)
  u32 n_left;    // ... of which x >= cam_w or y >= cam_h
  u32 n_pixels;  // non-zero pixels (F1)
  u32 pad;
};
static_assert(sizeof(FsAcc) == 32, "FsAcc layout");

struct FsStats {  // == xm_frame_surface_stats (include/xmaps.h)
  u64 n_events, n_pixels, n_index_errors;
  long long t_base, t_span;
};

struct FsArgs {                // by value to the three kernels
  const uint4* ev;             // the record array (group entry) ...
  u64 first[FS_GROUP];         // ... frame f = records [first[f], first[f] + n[f])
  u32 n[FS_GROUP];
  const FrameDesc* desc;       // ingest: ONE frame, described on the device (aos, n, valid); ev / first / n unused
  u32* map;                    // [frames][map_stride] winner maps
  FsAcc* acc;                  // [frames]
  FsStats* stats;              // [frames] (F2)
  void* out;                   // [frames][cam_h][cam_w] of the output type
  u64* tag;                    // ingest: the ring entry's tag in pinned host memory (F0 clears it, F2 sets it), else NULL
  u64 tag_value;
  FsStats* host_stats;         // ingest: the ring entry's statistics in pinned host memory (F2), else NULL
  u32 cells, map_stride;       // cam_w * cam_h; the same rounded up to FS_CPT
  int cam_w, cam_h;
  int use_polarity, select;
  u32 max_chunk_blocks;        // F0's grid.x is at most this: a frame longer than that many chunks takes further trips
};

struct FsFrameRef {
  const uint4* ev;
  u64 n;
};
__device__ inline FsFrameRef fs_frame(const FsArgs& a, u32 f) {
  if (a.desc) return a.desc->valid ? FsFrameRef{a.desc->aos, a.desc->n} : FsFrameRef{nullptr, 0};
  return FsFrameRef{a.ev + a.first[f], a.n[f]};
}

// F0 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FS_THREADS) void k_fs_events(FsArgs a) {
  __shared__ u64 s_min[FS_THREADS / 64], s_max[FS_THREADS / 64];
  __shared__ u32 s_n[FS_THREADS / 64], s_left[FS_THREADS / 64];
  const u32 f = blockIdx.y, tid = threadIdx.x;
  frame_tag_clear(a.tag);  // (F1 of this frame, the next launch, rewrites the ring entry)
  const FsFrameRef fr = fs_frame(a, f);
  u32* map = a.map + (size_t)f * a.map_stride;
  u64 mn = 0, mx = 0;
  u32 n_ev = 0, n_left = 0;
  for (u64 c0 = (u64)blockIdx.x * FS_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * FS_CHUNK) {  // (block-uniform)
    uint4 r[FS_EPT];
#pragma unroll
    for (int k = 0; k < FS_EPT; ++k) {
      const u64 i = c0 + (u64)k * FS_THREADS + tid;
      r[k] = i < fr.n ? fr.ev[i] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < FS_EPT; ++k) {
      const u64 i = c0 + (u64)k * FS_THREADS + tid;
      if (i >= fr.n) continue;
      if (!frame_exists(a.use_polarity, r[k])) continue;
      const u64 u = frame_enc(rec_t<long long>(r[k]));
      mn = ~u > mn ? ~u : mn;
      mx = u > mx ? u : mx;
      n_ev += 1;
      const u32 x = rec_x(r[k]), y = rec_y(r[k]);
      if (x >= (u32)a.cam_w || y >= (u32)a.cam_h) {
        n_left += 1;
        continue;
      }
      const u32 key = a.select == FS_SELECT_LAST ? (u32)i + 1u : ~(u32)i;  // (n < 2^32 - 1: never 0)
      __hip_atomic_fetch_max(&map[y * (u32)a.cam_w + x], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  mn = wave_max_u64(mn);
  mx = wave_max_u64(mx);
  n_ev = wave_sum_u32(n_ev);
  n_left = wave_sum_u32(n_left);
  const u32 wave = tid >> 6;
  if ((tid & 63) == 0) s_min[wave] = mn, s_max[wave] = mx, s_n[wave] = n_ev, s_left[wave] = n_left;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < FS_THREADS / 64; ++w) {
      mn = s_min[w] > mn ? s_min[w] : mn;
      mx = s_max[w] > mx ? s_max[w] : mx;
      n_ev += s_n[w];
      n_left += s_left[w];
    }
    if (n_ev) {
      FsAcc* acc = a.acc + f;
      __hip_atomic_fetch_max(&acc->min_enc, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(&acc->max_enc, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(&acc->n_events, n_ev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (n_left) __hip_atomic_fetch_add(&acc->n_left, n_left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// F1 ------------------------------------------------------------------------------------------------------------------------
// the winner's surface value: t - base + 1 in int64, converted once (0 = no event)
template <typename T>
__device__ inline T fs_value(const FsFrameRef& fr, u32 key, int select, long long base) {
  if (!key) return (T)0;
  const u32 idx = select == FS_SELECT_LAST ? key - 1u : ~key;
  const uint2 tw = *(const uint2*)((const char*)(fr.ev + idx) + 8);  // the record's t alone
  const long long t = (long long)(((u64)tw.y << 32) | tw.x);
  return (T)(long long)((u64)t - (u64)base + 1ull);  // (t >= base: the difference is exact; wraps only beyond a span of 2^63)
}

template <typename T>
__global__ __launch_bounds__(FS_THREADS) void k_fs_pixels(FsArgs a) {
  __shared__ u32 s_c[FS_THREADS / 64];
  const u32 f = blockIdx.y, tid = threadIdx.x;
  const FsFrameRef fr = fs_frame(a, f);
  u32* map = a.map + (size_t)f * a.map_stride;
  T* out = (T*)a.out + (size_t)f * a.cells;
  const long long base = frame_dec(~a.acc[f].min_enc);  // (F0 has finished: plain loads; unused when the frame has no event)
  const u32 c0 = (blockIdx.x * FS_THREADS + tid) * FS_CPT;
  u32 nz = 0;
  if (c0 < a.cells) {  // (map_stride is a multiple of FS_CPT: the 16-byte load stays inside the frame's map)
    const uint4 w = *(const uint4*)(map + c0);
    const u32 key[FS_CPT] = {w.x, w.y, w.z, w.w};
    T v[FS_CPT];
#pragma unroll
    for (int k = 0; k < FS_CPT; ++k) {
      v[k] = fs_value<T>(fr, key[k], a.select, base);
      nz += key[k] != 0;
    }
    if (nz) *(uint4*)(map + c0) = make_uint4(0, 0, 0, 0);  // the cells' last reader leaves them zero
    T* o = out + c0;
    if (c0 + FS_CPT <= a.cells && ((size_t)o & 15) == 0) {  // 16-byte stores where the frame's place in the output allows them
      if constexpr (sizeof(T) == 4) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        *(double2*)o = make_double2(v[0], v[1]);
        *(double2*)(o + 2) = make_double2(v[2], v[3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < FS_CPT; ++k)
        if (c0 + k < a.cells) o[k] = v[k];
    }
  }
  nz = wave_sum_u32(nz);
  if ((tid & 63) == 0) s_c[tid >> 6] = nz;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < FS_THREADS / 64; ++w) nz += s_c[w];
    if (nz) __hip_atomic_fetch_add(&a.acc[f].n_pixels, nz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// F2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_fs_finish(FsArgs a, u32 n_frames) {
  const u32 f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  FsAcc* acc = a.acc + f;
  const FsAcc v = *acc;
  *acc = FsAcc{0, 0, 0, 0, 0, 0};  // its last reader leaves it zero
  FsStats s{0, 0, 0, 0, 0};
  if (v.n_events) {
    const long long base = frame_dec(~v.min_enc), last = frame_dec(v.max_enc);
    s = FsStats{v.n_events, v.n_pixels, v.n_left, base, (long long)((u64)last - (u64)base)};
  }
  a.stats[f] = s;
  if (a.host_stats) {  // ingest: statistics, then the tag behind them, where xm_ingest_copy_surface reads both without a copy
    *a.host_stats = s;
    __hip_atomic_store(a.tag, a.tag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace xm
