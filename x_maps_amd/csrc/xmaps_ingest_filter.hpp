// xmaps_ingest_filter.hpp -- the frame event filters (N3) as a stage of the device ingest (N2): between the cut and K0, on the frame
// stream, without the host.
//
// What the reference does per cut frame while a filter is selected (python/frame_event_filter.py:19-151, applied at
// python/depth_reprojection_pipe.py:130-139): one output event per cell that fired -- cell = camera pixel (y, x) for the three XY
// filters, (y, rectified x) for FirstEventPerYT --, handed on in raster order of the cells.  The arithmetic of the record is
// filter_record (xmaps_filters.hpp), shared with the synchronous entry point xm_frame_event_filter.
// Here the cut frame is the FrameDesc k_ing_segment wrote (a pointer into the event ring + a count); the stage writes a SECOND
// descriptor for the same verdict entry whose events are the survivors in a scratch buffer, and K0 -> K1 -> K2 -> k_ing_publish run on
// that one unchanged:
//   k_ff_width    FirstEventPerYT on a rig whose rectify LUT has negative entries only: the frame's max(xr) -- the reference's map
//                 is max(xr) + 1 wide and a negative xr wraps like NumPy's negative index (col = xr + width), so the width must be
//                 known before the scatter.  Without negative entries no column wraps and the pass is not issued
//   k_ff_scatter  per event: its cell; atomic max of (index + 1) into the `last` map and, where the first event is asked for
//                 (`intended` semantics), of ~index into the `first` map.  An event whose cell lies outside the map -- x >= cam_w,
//                 y >= cam_h, a column still negative after the wrap: the reference raises IndexError -- is left out and counted
//                 (the frame's n_index_errors)
//   k_ff_count    per block of 1024 cells: how many are occupied
//   k_ff_emit     the same blocks: every block sums the counts in front of it itself (<= a few thousand words: no scan kernel),
//                 ranks its occupied cells by ballots and writes their records to the survivors buffer at raster rank; it leaves
//                 the cells it read ZERO (no memset per frame), and block 0 writes the second descriptor (n = the total)
// COMPACTION, not one record per cell with the polarity column honoured: K0 / K1 cost per event THREAD, and the cell count is
// 2 x (640 x 480, 153 K events per frame) to 5.5 x (FirstEventPerYT on the ESL rig: 845 K cells) the event count -- the frame
// kernels would run that many more threads to save one launch over a block per 1024 cells here.  (Reasoned from the thread
// counts; the two forms have not been timed against each other: tools/ingest_filter_probe.py gives the stage's share.)
// Every count is read from device memory; the grids come from the verdict's event count (an upper bound of the survivors) and the
// fixed cell count.  The cell maps use a FIXED row stride (cam_w, or the LUT's largest entry + 1): raster order does not depend on
// the reference's per-frame `max + 1` extents, only the wrap does.
// k_ff_emit is the last reader of the cut frame in the ring: the ingest stream waits for IT (not for K1) before appending more.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_filters.hpp"  // filter_record, FILTER_*
#include "xmaps_ingest.hpp"

namespace xm {

constexpr int FF_THREADS = 256;    // k_ff_width / k_ff_scatter: one event per thread
constexpr int FF_BLOCK = 1024;     // k_ff_count / k_ff_emit: one cell per thread
constexpr int FF_XR_BIAS = 32769;  // the width accumulator holds max(xr) + 32769: 0 = no event yet (xr is an int16)

struct FrameFilterCtl {   // device, one per ingest
  u32 xr_enc;             // k_ff_width: max over the frame's events of xr + FF_XR_BIAS; k_ff_emit (block 0) leaves it 0
  u32 pad;
};

struct FrameFilterInfo {  // device, one per verdict entry
  u32 n_dropped;          // events whose cell lies outside the map; k_ing_publish adds them to n_index_errors and leaves 0
  u32 pad;
};

struct FrameFilterDev {   // by value to the filter kernels
  const FrameDesc* cut;   // the verdict entry's descriptor as k_ing_segment wrote it
  FrameDesc* out;         // the entry's second descriptor (written by k_ff_emit)
  FrameFilterInfo* info;
  FrameFilterCtl* ctl;
  u32* last;              // [n_cells] largest (event index + 1) of the cell, 0 = empty.  All zero between frames
  u32* first;             // [n_cells] ~(smallest event index), 0 = empty (used with `use_first` only).  All zero between frames
  u32* sums;              // [blocks of FF_BLOCK cells] occupied cells of the block
  uint4* survivors;       // max(frame capacity, cells) records
  const u32* lut;         // the handle's rectify LUT, [cam_w][cam_h]: (u16(yr) << 16) | u16(xr)
  int cam_w, cam_h;
  int map_w;              // row stride of the maps: cam_w, or (FirstEventPerYT) the LUT's largest entry + 1
  u32 n_cells;            // cam_h * map_w
  int filter;             // FILTER_*
  int use_first;          // the cell's first event is needed too (`intended` semantics, any filter but LastEventPerXY)
  int wrap;               // FirstEventPerYT, LUT with negative entries: columns wrap at the frame's own width (ctl->xr_enc)
};

__device__ inline int ff_xr(const FrameFilterDev& f, int x, int y) { return (int)(short)(f.lut[(u32)x * (u32)f.cam_h + (u32)y] & 0xffffu); }

__global__ __launch_bounds__(FF_THREADS) void k_ff_width(FrameFilterDev f) {
  if (!f.cut->valid) return;
  const u64 n = f.cut->n;
  const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
  u32 enc = 0;
  if (i < n) {
    const uint4 r = f.cut->aos[i];
    const int x = (int)(r.x & 0xffff), y = (int)(r.x >> 16);
    if (x < f.cam_w && y < f.cam_h) enc = (u32)(ff_xr(f, x, y) + FF_XR_BIAS);
  }
  enc = wave_max_u32(enc);
  if ((threadIdx.x & 63) == 0 && enc) __hip_atomic_fetch_max(&f.ctl->xr_enc, enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FF_THREADS) void k_ff_scatter(FrameFilterDev f) {
  if (!f.cut->valid) return;
  const u64 n = f.cut->n;
  const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4 r = f.cut->aos[i];  // (every event in the ring has passed the polarity filter: p == 1)
  const int x = (int)(r.x & 0xffff), y = (int)(r.x >> 16);
  bool bad = x >= f.cam_w || y >= f.cam_h;
  int col = x;
  if (!bad && f.filter == FILTER_FIRST_PER_YT) {
    col = ff_xr(f, x, y);
    if (f.wrap && col < 0) col += (int)f.ctl->xr_enc - (FF_XR_BIAS - 1);  // NumPy negative index: + the frame's width, max(xr) + 1
    bad = col < 0 || col >= f.map_w;
  }
  if (bad) {
    atomicAdd(&f.info->n_dropped, 1u);
    return;
  }
  const u32 cell = (u32)y * (u32)f.map_w + (u32)col;
  __hip_atomic_fetch_max(&f.last[cell], (u32)i + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (f.use_first) __hip_atomic_fetch_max(&f.first[cell], ~(u32)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FF_BLOCK) void k_ff_count(FrameFilterDev f) {
  __shared__ u32 s_wave[FF_BLOCK / 64];
  if (!f.cut->valid) return;
  const u32 i = blockIdx.x * FF_BLOCK + threadIdx.x;
  const u64 b = __ballot(i < f.n_cells && f.last[i] != 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 c = 0;
#pragma unroll
    for (int w = 0; w < FF_BLOCK / 64; ++w) c += s_wave[w];
    f.sums[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(FF_BLOCK) void k_ff_emit(FrameFilterDev f, u32 n_blocks) {
  __shared__ u32 s_wave[FF_BLOCK / 64];
  __shared__ u32 s_red[2][FF_BLOCK / 64];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!f.cut->valid) {
    if (blockIdx.x == 0 && tid == 0) f.out->valid = 0;
    return;
  }
  const u32 mine = f.sums[blockIdx.x];
  if (!mine && blockIdx.x != 0) return;  // (an empty block has nothing to write or to clear; block 0 has the descriptor to write)
  // survivors in front of this block, and of the whole frame
  u32 before = 0, total = 0;
  for (u32 j = tid; j < n_blocks; j += FF_BLOCK) {
    const u32 v = f.sums[j];
    total += v;
    before += j < blockIdx.x ? v : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    total += __shfl_xor(total, o, 64);
  }
  const u32 i = blockIdx.x * FF_BLOCK + tid;
  const u32 li = i < f.n_cells ? f.last[i] : 0u;
  const u64 bal = __ballot(li != 0);
  if (lane == 0) {
    s_red[0][wave] = before;
    s_red[1][wave] = total;
    s_wave[wave] = __popcll(bal);
  }
  __syncthreads();
  before = 0, total = 0;
  u32 base = 0;
#pragma unroll
  for (int w = 0; w < FF_BLOCK / 64; ++w) {
    before += s_red[0][w];
    total += s_red[1][w];
    base += (u32)w < wave ? s_wave[w] : 0u;
  }
  if (li) {
    const uint4* aos = f.cut->aos;
    const uint4 last = aos[li - 1];
    uint4 first = last;
    if (f.use_first) {
      first = aos[~f.first[i]];
      f.first[i] = 0u;
    }
    f.last[i] = 0u;
    const u32 rank = before + base + (u32)__popcll(bal & ((1ull << lane) - 1ull));
    f.survivors[rank] = filter_record(f.filter, first, last, (int)(i % (u32)f.map_w), (int)(i / (u32)f.map_w));
  }
  if (blockIdx.x == 0 && tid == 0) {
    const FrameDesc c = *f.cut;
    FrameDesc* o = f.out;
    o->x = nullptr; o->y = nullptr; o->t = nullptr; o->p = nullptr;
    o->aos = f.survivors;
    o->n = total;
    o->key_frame = c.key_frame;
    o->st = c.st;
    o->depth = c.depth;
    o->bgr = c.bgr;
    o->pad = c.pad;
    o->valid = 1;
    f.ctl->xr_enc = 0u;  // (k_ff_scatter, its reader, has run)
  }
}

}  // namespace xm
