// xmaps_trigfilter.hpp -- the two filters of the triggered frames (xm_trigframes; the cut at EXT_TRIGGER words, xmaps_exttrigger.hpp):
// what the reference's pipe does to every packet in front of the cut (python/depth_reprojection_pipe.py:110-119: polarity filter,
// activity-noise filter) and to every cut frame while key E has a filter selected (:130-139), on the buffers of THAT chain -- a
// chunk of decoded records with trigger indices beside it, and runs of ready frames given by offsets --, not on the ingest's ring.
// (gfx950 / MI355X; included by xmaps_hip.hip behind xmaps_ingest.hpp, xmaps_ingest_filter.hpp and xmaps_exttrigger.hpp, whose
// pieces it joins and leaves as they are.)
//
// STAGE 1, the activity filter inside xm_trigframes_push (xm_trigframes_set_activity).  The rule is the ingest's, THIS BUILD'S
// DEFINITION (xmaps_ingest.hpp's header comment; oracle/ingest_oracle.py), on the positive on-sensor records of the stream in
// stream order; the state is an ActDev of the chain's own (history last_ts, the chunk's (bucket, pixel) cells, ctl), the chunk
// plays the packet's part.  With the stage on a push issues, in place of k_trig_keep_count / k_trig_keep_write:
//   k_act_first        (the ingest's, unchanged) the chunk's cells, and ctl[0] = 1 where the proviso fails
//   k_trigact_seq      one block: a chunk that failed the proviso is judged by act_sequential into the keep bytes (ctl[2] counts
//                      it); otherwise it returns at once.  A launch of its own because the host cannot know which way the chunk
//                      goes (the stamps never leave the device) and because no block may wait for another
//   k_trigact_count    the append's count kernel, 2048 records per block: every thread judges its 8 records with act_keep -- or, for
//                      a sequential chunk, reads what k_trigact_seq left --, stores the 8 keep bytes as ONE 8-byte store and the
//                      block stores its kept count
//   k_trigact_write    k_trig_keep_write driven by the keep bytes (fold of the counts in front, block scan, stable write, trigger
//                      remap), then the same threads retire their records (act_retire: history maximum, cells emptied) and
//                      record 0's thread resets ctl[0]
// THE FLAGS ARE COMPUTED INSIDE THE COUNT KERNEL, not by a k_act_mark launch in front of it: the count kernel has the records in
// registers anyway, the bytes it would read back are the bytes it has just made, and a launch on this chain is ~5 us of a push
// that is synchronous.  What that costs: a thread's 8 records are 8 consecutive ones, so a wave's gathers from the cell maps are
// 8 rounds of 64 scattered reads instead of k_act_mark's coalesced-by-index form; the maps are L2-resident either way.
// Measured (profiles/ext_trigger_filters.md, period chunks of ~170 K records): k_trigact_count 31 us, where the ingest's
// k_act_mark takes 6.7 us on the same chunk's positive events -- so the other form (k_act_mark in front, a count kernel that
// only reads bytes) would probably win ~15 us of kernel time per chunk against the launch it adds.  The two forms have not
// been timed against each other as whole pushes; the stage costs +0.049 ms per chunk as it is.
// k_trigact_write reads no cell and no history: retiring in the same launch races with nothing.  Integer atomics only (the
// history's 64-bit maximum, a counter per block for the statistics); plain stores for the records.
//
// STAGE 2, the frame event filters on a run of ready frames (xm_trigframes_set_frame_filter / xm_trigframes_ready_filtered):
// xmaps_ingest_filter.hpp's four kernels restated for a GROUP -- blockIdx.y is the frame, frame f's events are
// buf + offsets[f] .. offsets[f + 1] (offsets uploaded per call), the `last` / `first` maps, the width accumulator and the
// drop counter are per frame, and event indices are relative to the frame.  The arithmetic stays filter_record.
//   k_tff_width    FirstEventPerYT on a LUT with negative entries only: frame f's max(xr), for the wrap
//   k_tff_scatter  per event: its cell; atomic max of index + 1 into `last`, of ~index into `first` where the first event is needed
//   k_tff_count    per (frame, 1024 cells): occupied cells
//   k_tff_emit     the same blocks: every block folds the counts of the blocks in front of it -- its own frame's and the frames' in
//                  front of its frame -- ranks by ballots, writes the survivor at its rank and leaves the cells it read ZERO; the
//                  last block of each frame stores the frame's total and drop count for the host and clears the frame's
//                  accumulators (no memset per call)
// PACKED, not a fixed stride per frame: the frame entries take ONE buffer and n + 1 offsets, frame f = [offsets[f], offsets[f + 1])
// -- frames with gaps between them cannot be said that way.  Frame f's survivors start at the sum of the totals in front, which
// is the fold every block does anyway.  No block waits for another.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_exttrigger.hpp"      // KeepScan, ext_trig_offset, trig_lower_bound
#include "xmaps_filters.hpp"         // filter_record, FILTER_*
#include "xmaps_ingest.hpp"          // ActDev, act_event, act_keep, act_retire, act_sequential
#include "xmaps_ingest_filter.hpp"   // FF_THREADS, FF_BLOCK, FF_XR_BIAS

namespace xm {

// ---- stage 1 ------------------------------------------------------------------------------------------------------------------
// (a.keep: room for gridDim.x * EVT_PER_BLOCK bytes, 8-byte aligned: a thread's 8 flags are one word, the chunk's tail included)
__global__ __launch_bounds__(ACT_GROUP) void k_trigact_seq(ActDev a, const uint4* __restrict__ ev, u32 n) {
  if (!a.ctl[0]) return;
  if (threadIdx.x == 0) a.ctl[2] += 1u;
  act_sequential(a, ev, 0, n, true);
}

// stats[0] += the chunk's p == 1 records (on the sensor or not)
__global__ __launch_bounds__(EVT_THREADS) void k_trigact_count(ActDev a, const uint4* __restrict__ ev, u32 n, u32* __restrict__ counts,
                                                               unsigned long long* __restrict__ stats) {
  __shared__ KeepScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  unsigned long long* kw = reinterpret_cast<unsigned long long*>(a.keep) + (i0 >> 3);
  static_assert(EVT_IPT == 8, "a thread's keep flags are one 8-byte word");
  const bool sequential = a.ctl[0] != 0u;
  const long long t0 = n ? rec_t(ev[0]) : 0;
  unsigned long long word = sequential ? *kw : 0ull;
  KeepScan acc{0}, pos{0};
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n) {
      word &= ~(0xffull << (8 * k));
      continue;
    }
    const uint4 r = ev[i0 + k];
    pos.n += trig_keeps(r);
    if (!sequential) {
      const bool keep = act_keep(a, act_event(r, true, true, a.cam_w, a.cam_h), i0 + k, t0);
      word |= (unsigned long long)(keep ? 1u : 0u) << (8 * k);
    }
    acc.n += (u32)((word >> (8 * k)) & 1ull);
  }
  if (!sequential) *kw = word;
  KeepScan total, ptotal;
  (void)evt_block_scan(acc, buf, &total);
  (void)evt_block_scan(pos, buf, &ptotal);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = total.n;
    if (ptotal.n) atomicAdd(stats, (unsigned long long)ptotal.n);
  }
}

// out / remap / counts[gridDim.x]: as k_trig_keep_write
__global__ __launch_bounds__(EVT_THREADS) void k_trigact_write(ActDev a, const uint4* __restrict__ ev, u32 n, u32* __restrict__ counts,
                                                               uint4* __restrict__ out, u32 out_cap, const uint4* __restrict__ trig,
                                                               u32 n_trig, u32* __restrict__ remap) {
  __shared__ KeepScan buf[2][EVT_THREADS];
  __shared__ KeepScan s_incl[EVT_THREADS];
  __shared__ u32 s_sum[EVT_THREADS];
  const u32 offset = ext_trig_offset(counts, s_sum);
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  const unsigned long long word = reinterpret_cast<const unsigned long long*>(a.keep)[i0 >> 3];
  const long long t0 = n ? rec_t(ev[0]) : 0;
  uint4 r[EVT_IPT];
  KeepScan acc{0};
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    r[k] = i0 + k < n ? ev[i0 + k] : make_uint4(0, 0, 0, 0);
    if (i0 + k < n) acc.n += (u32)((word >> (8 * k)) & 1ull);
  }
  KeepScan total;
  const KeepScan incl = evt_block_scan(acc, buf, &total);
  s_incl[threadIdx.x] = incl;
  __syncthreads();
  u32 at = offset + (threadIdx.x ? s_incl[threadIdx.x - 1].n : 0u);
  u32 j = i0 < n ? trig_lower_bound(trig, n_trig, i0) : n_trig;
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n) break;
    for (; j < n_trig && trig[j].z == i0 + k; ++j) remap[j] = at;  // the triggers in front of record i0 + k
    if ((word >> (8 * k)) & 1ull) {
      if (at < out_cap) out[at] = r[k];
      at += 1;
    }
  }
  if (blockIdx.x == gridDim.x - 1) {
    const u32 kept = offset + total.n;
    if (threadIdx.x == 0) counts[gridDim.x] = kept;
    for (u32 q = trig_lower_bound(trig, n_trig, n) + threadIdx.x; q < n_trig; q += EVT_THREADS) remap[q] = kept;  // behind the chunk's last record
  }
  // behind the flags: the positive records join their pixels' history, their cells of this chunk are emptied for the next one
  if (i0 == 0) a.ctl[0] = 0u;  // (read by k_trigact_seq and k_trigact_count, in front of this kernel)
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) act_retire(a, act_event(r[k], true, true, a.cam_w, a.cam_h), t0);
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------------
struct TrigFilterDev {    // by value to the four kernels
  const uint4* buf;       // the triggered frames' buffer
  const u64* offsets;     // [n_frames + 1] record offsets into buf (device; uploaded per call)
  u32* last;              // [max_frames][n_cells] largest (frame-relative index + 1) of the cell, 0 = empty.  All zero between calls
  u32* first;             // [max_frames][n_cells] ~(smallest index), 0 = empty (use_first only).  All zero between calls
  u32* sums;              // [n_frames][blocks of FF_BLOCK cells]
  u32* xr_enc;            // [max_frames] k_tff_width: max(xr) + FF_XR_BIAS of the frame; 0 between calls
  u32* dropped;           // [max_frames] events whose cell lies outside the map; 0 between calls
  u32* result;            // [2][max_frames] per frame: survivors, dropped -- what the host copies back
  uint4* survivors;       // surv_cap records
  const u32* lut;         // the handle's rectify LUT, [cam_w][cam_h]: (u16(yr) << 16) | u16(xr)
  u32 surv_cap, max_frames;
  int cam_w, cam_h;
  int map_w;              // row stride of the maps
  u32 n_cells;            // cam_h * map_w
  int filter, use_first, wrap;  // as FrameFilterDev's
};

__device__ inline int tff_xr(const TrigFilterDev& f, int x, int y) { return (int)(short)(f.lut[(u32)x * (u32)f.cam_h + (u32)y] & 0xffffu); }

__global__ __launch_bounds__(FF_THREADS) void k_tff_width(TrigFilterDev f) {
  const u32 fr = blockIdx.y;
  const u64 a = f.offsets[fr], n = f.offsets[fr + 1] - a;
  const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
  u32 enc = 0;
  if (i < n) {
    const uint4 r = f.buf[a + i];
    const int x = (int)(r.x & 0xffff), y = (int)(r.x >> 16);
    if (x < f.cam_w && y < f.cam_h) enc = (u32)(tff_xr(f, x, y) + FF_XR_BIAS);
  }
  enc = wave_max_u32(enc);
  if ((threadIdx.x & 63) == 0 && enc) __hip_atomic_fetch_max(&f.xr_enc[fr], enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FF_THREADS) void k_tff_scatter(TrigFilterDev f) {
  const u32 fr = blockIdx.y;
  const u64 a = f.offsets[fr], n = f.offsets[fr + 1] - a;
  const u64 i = (u64)blockIdx.x * FF_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint4 r = f.buf[a + i];  // (every record of the buffer is what the chain's filters kept)
  const int x = (int)(r.x & 0xffff), y = (int)(r.x >> 16);
  bool bad = x >= f.cam_w || y >= f.cam_h;
  int col = x;
  if (!bad && f.filter == FILTER_FIRST_PER_YT) {
    col = tff_xr(f, x, y);
    if (f.wrap && col < 0) col += (int)f.xr_enc[fr] - (FF_XR_BIAS - 1);  // NumPy negative index: + the frame's width, max(xr) + 1
    bad = col < 0 || col >= f.map_w;
  }
  if (bad) {
    atomicAdd(&f.dropped[fr], 1u);
    return;
  }
  const size_t cell = (size_t)fr * f.n_cells + (u32)y * (u32)f.map_w + (u32)col;
  __hip_atomic_fetch_max(&f.last[cell], (u32)i + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (f.use_first) __hip_atomic_fetch_max(&f.first[cell], ~(u32)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FF_BLOCK) void k_tff_count(TrigFilterDev f) {
  __shared__ u32 s_wave[FF_BLOCK / 64];
  const u32 i = blockIdx.x * FF_BLOCK + threadIdx.x;
  const u64 b = __ballot(i < f.n_cells && f.last[(size_t)blockIdx.y * f.n_cells + i] != 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 c = 0;
#pragma unroll
    for (int w = 0; w < FF_BLOCK / 64; ++w) c += s_wave[w];
    f.sums[blockIdx.y * gridDim.x + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(FF_BLOCK) void k_tff_emit(TrigFilterDev f) {
  __shared__ u32 s_wave[FF_BLOCK / 64];
  __shared__ u32 s_red[2][FF_BLOCK / 64];
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 fr = blockIdx.y, nb = gridDim.x, lin = fr * nb + blockIdx.x;
  const bool closes = blockIdx.x == nb - 1;  // the frame's last block (in block order: nobody waits) reports the frame
  const u32 mine = f.sums[lin];
  if (!mine && !closes) return;  // (an empty block has nothing to write or to clear)
  // survivors in front of this block -- of the frames in front and of this frame's earlier blocks --, and this frame's total
  u32 before = 0, total = 0;
  for (u32 j = tid; j < (fr + 1) * nb; j += FF_BLOCK) {
    const u32 v = f.sums[j];
    before += j < lin ? v : 0u;
    total += j >= fr * nb ? v : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    total += __shfl_xor(total, o, 64);
  }
  const u32 i = blockIdx.x * FF_BLOCK + tid;
  const size_t cell = (size_t)fr * f.n_cells + i;
  const u32 li = i < f.n_cells ? f.last[cell] : 0u;
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
    const uint4* aos = f.buf + f.offsets[fr];
    const uint4 last = aos[li - 1];
    uint4 first = last;
    if (f.use_first) {
      first = aos[~f.first[cell]];
      f.first[cell] = 0u;
    }
    f.last[cell] = 0u;
    const u32 rank = before + base + (u32)__popcll(bal & ((1ull << lane) - 1ull));
    if (rank < f.surv_cap) f.survivors[rank] = filter_record(f.filter, first, last, (int)(i % (u32)f.map_w), (int)(i / (u32)f.map_w));
  }
  if (closes && tid == 0) {
    f.result[fr] = total;
    f.result[f.max_frames + fr] = f.dropped[fr];
    f.dropped[fr] = 0u;  // (k_tff_scatter, their writer and reader, has run)
    f.xr_enc[fr] = 0u;
  }
}

}  // namespace xm
