// xmaps_evt21.hpp -- Prophesee EVT 2.1 words -> EventCD records on the device: the 64-bit vectorised RAW
// encoding of Gen4 / IMX636 cameras, one CD word = a row, a base column and a 32-bit validity mask.  (gfx950 / MI355X; included
// by xmaps_hip.hip.)  x_maps_amd/evt21.py restates the format on the host, tests/evt21_ref.py is the independent word-by-word checker.
//
//   [63:60] type   0x0 EVT_NEG / 0x1 EVT_POS   [59:54] t[5:0]   [53:43] x_base   [42:32] y   [31:0] valid
//                                              bit n of valid set -> one event at (x_base + n, y), p = type, ascending n
//                  0x8 EVT_TIME_HIGH           [59:32] t[33:6]; [31:0] ignored                 the time base of the words behind it
//                  0xA EXT_TRIGGER, 0xE OTHERS, 0xF CONTINUED, anything else                   skipped
//   t = (loops << 34) | (time_high << 6) | t[5:0]; a loop: the 28-bit field falls back by more than 2^27, as in EVT 2.0.
//   legacy halves: the file stores each word as two 32-bit little-endian halves, HIGH half first; undone where a word is loaded.
//
// The scan is EVT 2.0's with one difference: a word is 0..32 events, so n_ev and n_pre count EVENTS (popcounts).  A block of
// EVT_PER_BLOCK words can therefore emit 65 536 records, and there are two emit kernels.  k_evt21_emit writes BY OUTPUT SLOT: the
// block's events are one contiguous range of the output, the block scan leaves every word's inclusive event count (and time base)
// in LDS, a lane takes slot trip * EVT_THREADS + lane, finds its word by binary search over the counts and picks the k-th set bit
// of its mask, so a wave's 16-byte stores go to 64 consecutive records whatever the masks are.  k_evt21_emit_words is the plain
// per-word loop (a lane walks the set bits of its own words).  Measured (profiles/evt21.md), the per-word loop is the faster one
// -- 0.21 against 0.37 ms on 2^18 words of 27 events each: the slot kernel pays eleven dependent LDS reads per record and its
// 61 KB of LDS leave two blocks per CU -- so IT is what the decoder launches; the slot kernel stays behind the debug option
// "XM_EVT21_EMIT_BY_WORD" = 0 so that the table can be measured again, and both are pinned by tests/test_gpu_evt21.py.  The block
// geometry, the state record (t_high, t_loops, have_high, n_events), the start-of-stream rule and the block scan are xmaps_evt.hpp's.
#pragma once
#include "xmaps_evt.hpp"

namespace xm {

struct Evt21Scan {
  u32 hi_has, hi_first, hi_last, hi_wraps;  // TIME_HIGH words of the range
  u32 n_ev;                                 // EVENTS of the range: the popcounts of its CD words' masks
  u32 hi_word, n_pre;                       // a TIME_HIGH WORD lies in the range (the seed is not one); events in front of its first one
};

__device__ __forceinline__ Evt21Scan evt21_identity() {
  Evt21Scan e;
  e.hi_has = e.hi_first = e.hi_last = e.hi_wraps = 0;
  e.n_ev = 0;
  e.hi_word = e.n_pre = 0;
  return e;
}

// a = the earlier range, b = the later one
__device__ __forceinline__ Evt21Scan evt_combine(const Evt21Scan& a, const Evt21Scan& b) {
  Evt21Scan r;
  if (!b.hi_has) {
    r.hi_has = a.hi_has; r.hi_first = a.hi_first; r.hi_last = a.hi_last; r.hi_wraps = a.hi_wraps;
  } else if (!a.hi_has) {
    r.hi_has = 1; r.hi_first = b.hi_first; r.hi_last = b.hi_last; r.hi_wraps = b.hi_wraps;
  } else {
    const bool wrap = (long long)a.hi_last - (long long)b.hi_first > (1ll << 27);
    r.hi_has = 1; r.hi_first = a.hi_first; r.hi_last = b.hi_last;
    r.hi_wraps = a.hi_wraps + b.hi_wraps + (wrap ? 1u : 0u);
  }
  r.n_ev = a.n_ev + b.n_ev;
  r.hi_word = a.hi_word | b.hi_word;
  r.n_pre = a.hi_word ? a.n_pre : a.n_ev + b.n_pre;
  return r;
}

constexpr unsigned long long EVT21_SKIPPED = 0xE000000000000000ull;  // (OTHERS: what the words behind the chunk's end count as)

// word i of the chunk as the format defines it (legacy: the two halves swapped back)
__device__ __forceinline__ unsigned long long evt21_load(const unsigned long long* __restrict__ words, u32 i, int legacy) {
  const unsigned long long w = words[i];
  return legacy ? (w << 32) | (w >> 32) : w;
}

__device__ __forceinline__ Evt21Scan evt21_element(unsigned long long w) {
  Evt21Scan e = evt21_identity();
  const u32 typ = (u32)(w >> 60);
  if (typ <= 1u) e.n_ev = e.n_pre = (u32)__popc((u32)w);
  else if (typ == 0x8u) { e.hi_has = 1; e.hi_first = e.hi_last = (u32)(w >> 32) & 0x0fffffffu; e.hi_word = 1; }
  return e;
}

__device__ __forceinline__ Evt21Scan evt21_seed(const Evt3State& s) {  // the state in front of the chunk as a range of its own
  Evt21Scan e = evt21_identity();
  e.hi_has = 1;
  e.hi_first = e.hi_last = s.t_high;
  return e;
}

// column offset of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ u32 evt21_kth_bit(u32 m, u32 k) {
  u32 pos = 0;
#pragma unroll
  for (u32 width = 16; width; width >>= 1) {
    const u32 c = (u32)__popc(m & ((1u << width) - 1u));
    if (k >= c) { k -= c; m >>= width; pos += width; }
  }
  return pos;
}

__device__ __forceinline__ uint4 evt21_record(unsigned long long w, u32 bit, unsigned long long loops, u32 t_high) {
  const unsigned long long t = (loops << 34) | ((unsigned long long)t_high << 6) | ((w >> 54) & 0x3full);
  const u32 x = ((u32)(w >> 43) & 0x7ffu) + bit, y = (u32)(w >> 32) & 0x7ffu;
  return make_uint4(x | (y << 16), (u32)(w >> 60), (u32)t, (u32)(t >> 32));
}

// 1. the aggregate of every block of EVT_PER_BLOCK words
__global__ __launch_bounds__(EVT_THREADS) void k_evt21_aggregate(const unsigned long long* __restrict__ words, u32 n, Evt21Scan* __restrict__ agg,
                                                                 int legacy) {
  __shared__ Evt21Scan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  Evt21Scan acc = evt21_identity();
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc = evt_combine(acc, evt21_element(evt21_load(words, i0 + k, legacy)));
  Evt21Scan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// 2. one block: exclusive scan of the aggregates, seeded with the previous chunk's state; the chunk's event count and the state
//    for the next chunk (the EVT 3.0 record: only t_high, t_loops, have_high and n_events are used)
__global__ __launch_bounds__(EVT_THREADS) void k_evt21_prefix(u32 n_blocks, Evt21Scan* __restrict__ agg, const Evt3State* __restrict__ st_in,
                                                              Evt3State* __restrict__ st_out, u32* __restrict__ count_out, int wait) {
  __shared__ Evt21Scan buf[2][EVT_THREADS];
  __shared__ Evt21Scan s_incl[EVT_THREADS];
  const Evt3State s = *st_in;
  Evt21Scan carry = evt21_seed(s);
  for (u32 b0 = 0; b0 < n_blocks; b0 += EVT_THREADS) {
    const u32 b = b0 + threadIdx.x;
    const Evt21Scan mine = b < n_blocks ? agg[b] : evt21_identity();
    Evt21Scan total;
    const Evt21Scan incl = evt_block_scan(mine, buf, &total);
    s_incl[threadIdx.x] = incl;
    __syncthreads();
    if (b < n_blocks) agg[b] = threadIdx.x ? evt_combine(carry, s_incl[threadIdx.x - 1]) : carry;
    carry = evt_combine(carry, total);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Evt3State o;
    o.y = o.base_x = o.base_p = o.t_low = 0;
    o.have_high = s.have_high | carry.hi_word;
    o.t_high = carry.hi_last;
    o.t_loops = s.t_loops + carry.hi_wraps;
    o.n_events = carry.n_ev - evt_dropped(carry.n_pre, s.have_high, wait);
    *st_out = o;
    if (count_out) *count_out = (u32)o.n_events;  // (a cell of the consumer's: this record is rewritten two chunks from now)
  }
}

// 3. the records, by output slot: every block re-scans its words from its exclusive prefix, leaves per word {events emitted in
//    the block up to and including it, time base, loops, the word} in LDS and then walks its range of the output
__global__ __launch_bounds__(EVT_THREADS) void k_evt21_emit(const unsigned long long* __restrict__ words, u32 n, const Evt21Scan* __restrict__ prefix,
                                                            const Evt3State* __restrict__ st_in, uint4* __restrict__ out, u32 out_cap, int wait,
                                                            int legacy) {
  __shared__ Evt21Scan buf[2][EVT_THREADS];
  __shared__ Evt21Scan s_incl[EVT_THREADS];
  __shared__ unsigned long long s_word[EVT_PER_BLOCK];
  __shared__ u32 s_cnt[EVT_PER_BLOCK], s_high[EVT_PER_BLOCK], s_wraps[EVT_PER_BLOCK];
  const unsigned long long loops0 = st_in->t_loops;
  const u32 have_high = st_in->have_high;
  const u32 l0 = threadIdx.x * EVT_IPT, i0 = blockIdx.x * EVT_PER_BLOCK + l0;
  unsigned long long w[EVT_IPT];
  Evt21Scan acc = evt21_identity();
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    w[k] = i0 + k < n ? evt21_load(words, i0 + k, legacy) : EVT21_SKIPPED;
    acc = evt_combine(acc, evt21_element(w[k]));
  }
  Evt21Scan total;
  const Evt21Scan incl = evt_block_scan(acc, buf, &total);
  s_incl[threadIdx.x] = incl;
  __syncthreads();
  const Evt21Scan pre = prefix[blockIdx.x];
  const u32 base = pre.n_ev - evt_dropped(pre.n_pre, have_high, wait);  // the block's first slot of the output
  Evt21Scan run = pre;
  if (threadIdx.x) run = evt_combine(run, s_incl[threadIdx.x - 1]);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    run = evt_combine(run, evt21_element(w[k]));
    s_word[l0 + k] = w[k];
    s_cnt[l0 + k] = run.n_ev - evt_dropped(run.n_pre, have_high, wait) - base;  // (a word in front of the first time base adds nothing)
    s_high[l0 + k] = run.hi_last;
    s_wraps[l0 + k] = run.hi_wraps;
  }
  __syncthreads();
  if (base >= out_cap) return;
  const u32 n_slots = min(s_cnt[EVT_PER_BLOCK - 1], out_cap - base);  // (a word whose events straddle out_cap: the slots below it)
  for (u32 s = threadIdx.x; s < n_slots; s += EVT_THREADS) {
    u32 lo = 0, hi = EVT_PER_BLOCK - 1;  // the first word whose inclusive count exceeds s
    while (lo < hi) {
      const u32 mid = (lo + hi) >> 1;
      if (s_cnt[mid] > s) hi = mid; else lo = mid + 1;
    }
    const u32 k = s - (lo ? s_cnt[lo - 1] : 0u);
    const unsigned long long wd = s_word[lo];
    out[base + s] = evt21_record(wd, evt21_kth_bit((u32)wd, k), loops0 + s_wraps[lo], s_high[lo]);
  }
}

// 3'. the records, by word: a lane walks the set bits of its own EVT_IPT words (EVT 2.0's emit with an inner loop)
__global__ __launch_bounds__(EVT_THREADS) void k_evt21_emit_words(const unsigned long long* __restrict__ words, u32 n, const Evt21Scan* __restrict__ prefix,
                                                                  const Evt3State* __restrict__ st_in, uint4* __restrict__ out, u32 out_cap,
                                                                  int wait, int legacy) {
  __shared__ Evt21Scan buf[2][EVT_THREADS];
  __shared__ Evt21Scan s_incl[EVT_THREADS];
  const unsigned long long loops0 = st_in->t_loops;
  const u32 have_high = st_in->have_high;
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  unsigned long long w[EVT_IPT];
  Evt21Scan acc = evt21_identity();
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    w[k] = i0 + k < n ? evt21_load(words, i0 + k, legacy) : EVT21_SKIPPED;
    acc = evt_combine(acc, evt21_element(w[k]));
  }
  Evt21Scan total;
  const Evt21Scan incl = evt_block_scan(acc, buf, &total);
  s_incl[threadIdx.x] = incl;
  __syncthreads();
  Evt21Scan run = prefix[blockIdx.x];
  if (threadIdx.x) run = evt_combine(run, s_incl[threadIdx.x - 1]);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    u32 at = run.n_ev - evt_dropped(run.n_pre, have_high, wait);
    const Evt21Scan e = evt21_element(w[k]);
    run = evt_combine(run, e);
    if (!e.n_ev) continue;
    if (wait && !have_high && !run.hi_word) continue;  // in front of the stream's first EVT_TIME_HIGH: not emitted
    for (u32 m = (u32)w[k]; m && at < out_cap; m &= m - 1u, ++at)
      out[at] = evt21_record(w[k], (u32)__ffs(m) - 1u, loops0 + run.hi_wraps, run.hi_last);
  }
}

}  // namespace xm
