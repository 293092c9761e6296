// xmaps_exttrigger.hpp -- the EXT_TRIGGER words of a Prophesee recording (the pulses of the camera's sync jack) -> trigger records
// on the device, beside the decoders' EventCD records.  (gfx950 / MI355X; included by xmaps_hip.hip behind the decoders.)
// Host form x_maps_amd/ext_trigger.py (ExtTriggerExtractor), independent word-by-word checker tests/ext_trigger_ref.py.
//
// The word, per format (the vendor's published format description; unpinned against Metavision, like the decoders):
//   EVT 3.0 (16 bit)  [15:12] = 0xA   [11:8] id    [0] value     t = the state machine's current TIME_HIGH / TIME_LOW, exactly as for a
//                                                                CD event at that word (a TIME_HIGH that changed the field restarts the
//                                                                low field at 0; the 24-bit wrap count applies)
//   EVT 2.0 (32 bit)  [31:28] = 0xA   [27:22] t[5:0]   [12:8] id    [0] value    t = (loops << 34) | (time_high << 6) | t[5:0], as CD words
//   EVT 2.1 (64 bit)  [63:60] = 0xA   [59:54] t[5:0]   [44:40] id   [32] value   composed as in EVT 2.0; legacy halves swapped back first
// A trigger word changes no decoder state (row, vector base and time stay as they were): it is the identity of every format's scan.
//
// The record (xm_ext_trigger, include/xmaps.h; 16 bytes, stored here as one uint4): {t, event_index, id, value, reserved = 0}.
// event_index = the number of records the decoder writes for this chunk IN FRONT of the word -- the `before` of the k_*_emit
// kernels, n_ev - evt_dropped(...) of the range in front of the word (never more than the chunk's event count: evt_dropped is
// constant once the range holds a TIME_HIGH word and equals n_ev before) -- so the boundary is exact in stream order whatever
// the time stamps are.  Start-of-stream rule as for the events: in front of the stream's first TIME_HIGH a trigger carries the
// time base 0 (wait_for_time_base off) or is not emitted (on).
//
// Two launches per chunk behind the format's emit kernel, over what that left: the words (d_words), the per-block exclusive
// prefixes with the seed (d_agg) and the chunk's input state.  (a) k_*_trig_count: every block counts the trigger words it will
// emit.  (b) k_*_trig_emit: every block sums the counts of the blocks in front of it, in block order, re-scans its words from
// its prefix exactly as the emit kernel does and stores its triggers' records at offset + rank.  No atomics, no block waits for
// another, plain stores; the last block leaves the chunk's total behind the counts.  The bodies are spelled out per format
// (xmaps_evt.hpp says why); evt_block_scan, the formats' scan records and their evt_combine overloads are the decoders'.
#pragma once
#include "xmaps_evt.hpp"
#include "xmaps_evt2.hpp"
#include "xmaps_evt21.hpp"
#include "xmaps_evt3.hpp"

namespace xm {

// trigger words of a range: all of them, and those behind the range's first TIME_HIGH word (what a block in front of the
// stream's first time base emits when the decoder waits for it)
struct ExtTrigScan {
  u32 n_all, n_behind, has_hi;
};

__device__ __forceinline__ ExtTrigScan evt_combine(const ExtTrigScan& a, const ExtTrigScan& b) {
  ExtTrigScan r;
  r.n_all = a.n_all + b.n_all;
  r.n_behind = a.has_hi ? a.n_behind + b.n_all : b.n_behind;
  r.has_hi = a.has_hi | b.has_hi;
  return r;
}

__device__ __forceinline__ ExtTrigScan ext_trig_element(u32 typ) {  // a word of type `typ` (0x8 is TIME_HIGH in all three formats)
  ExtTrigScan e;
  e.n_all = typ == 0xAu ? 1u : 0u;
  e.n_behind = 0;
  e.has_hi = typ == 0x8u ? 1u : 0u;
  return e;
}

// the triggers of range `r` that are emitted; drop_pre: those in front of the range's first TIME_HIGH word are not
__device__ __forceinline__ u32 ext_trig_emitted(const ExtTrigScan& r, const bool drop_pre) { return drop_pre ? r.n_behind : r.n_all; }

__device__ __forceinline__ uint4 ext_trig_record(unsigned long long t, u32 event_index, u32 id, u32 value) {
  return make_uint4((u32)t, (u32)(t >> 32), event_index, id | (value << 8));  // (xm_ext_trigger: t, event_index, id, value, reserved 0)
}

// sum of counts[0 .. blockIdx.x): the records the blocks in front of this one store (EVT_THREADS counts per trip, in block order)
__device__ __forceinline__ u32 ext_trig_offset(const u32* __restrict__ counts, u32* s_sum) {
  u32 part = 0;
  for (u32 b0 = 0; b0 < blockIdx.x; b0 += EVT_THREADS) {
    const u32 b = b0 + threadIdx.x;
    if (b < blockIdx.x) part += counts[b];
  }
  s_sum[threadIdx.x] = part;
  __syncthreads();
  for (int o = EVT_THREADS / 2; o; o >>= 1) {
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  const u32 r = s_sum[0];
  __syncthreads();
  return r;
}

// ---- EVT 3.0 ----
__global__ __launch_bounds__(EVT_THREADS) void k_evt3_trig_count(const uint16_t* __restrict__ words, u32 n, const Evt3Scan* __restrict__ prefix,
                                                                 const Evt3State* __restrict__ st_in, u32* __restrict__ counts, int wait) {
  __shared__ ExtTrigScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  ExtTrigScan acc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc = evt_combine(acc, ext_trig_element((u32)words[i0 + k] >> 12));
  ExtTrigScan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = ext_trig_emitted(total, wait && !st_in->have_high && !prefix[blockIdx.x].hi_word);
}

__global__ __launch_bounds__(EVT_THREADS) void k_evt3_trig_emit(const uint16_t* __restrict__ words, u32 n, const Evt3Scan* __restrict__ prefix,
                                                                const Evt3State* __restrict__ st_in, u32* __restrict__ counts,
                                                                uint4* __restrict__ out, u32 out_cap, int wait) {
  __shared__ Evt3Scan buf[2][EVT_THREADS];
  __shared__ Evt3Scan s_incl[EVT_THREADS];
  __shared__ ExtTrigScan tbuf[2][EVT_THREADS];
  __shared__ ExtTrigScan s_tincl[EVT_THREADS];
  __shared__ u32 s_sum[EVT_THREADS];
  const Evt3State s = *st_in;
  const u32 offset = ext_trig_offset(counts, s_sum);
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  u32 w[EVT_IPT];
  Evt3Scan acc = evt3_identity();
  ExtTrigScan tacc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    w[k] = i0 + k < n ? (u32)words[i0 + k] : 0xE000u;  // (OTHERS: skipped)
    if (i0 + k < n) acc = evt_combine(acc, evt3_element(w[k], i0 + k));
    tacc = evt_combine(tacc, ext_trig_element(w[k] >> 12));
  }
  Evt3Scan total;
  const Evt3Scan incl = evt_block_scan(acc, buf, &total);
  ExtTrigScan ttotal;
  const ExtTrigScan tincl = evt_block_scan(tacc, tbuf, &ttotal);
  s_incl[threadIdx.x] = incl;
  s_tincl[threadIdx.x] = tincl;
  __syncthreads();
  Evt3Scan run = prefix[blockIdx.x];
  const bool drop_pre = wait && !s.have_high && !run.hi_word;  // the block starts in front of the stream's first TIME_HIGH word
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) counts[gridDim.x] = offset + ext_trig_emitted(ttotal, drop_pre);  // the chunk's total
  ExtTrigScan trun = ext_trig_element(0xEu);
  if (threadIdx.x) { run = evt_combine(run, s_incl[threadIdx.x - 1]); trun = s_tincl[threadIdx.x - 1]; }
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n) break;
    const u32 before = run.n_ev - evt_dropped(run.n_pre, s.have_high, wait);
    const u32 rank = ext_trig_emitted(trun, drop_pre);
    run = evt_combine(run, evt3_element(w[k], i0 + k));
    trun = evt_combine(trun, ext_trig_element(w[k] >> 12));
    if ((w[k] >> 12) != 0xAu) continue;
    if (wait && !s.have_high && !run.hi_word) continue;  // in front of the stream's first TIME_HIGH word: not emitted
    u32 y, th, tl, base, pol;
    unsigned long long loops;
    evt3_resolve(run, s, words, y, th, tl, loops, base, pol);
    const unsigned long long t = (loops << 24) | ((unsigned long long)th << 12) | (unsigned long long)tl;
    if (offset + rank < out_cap) out[offset + rank] = ext_trig_record(t, before, (w[k] >> 8) & 0xfu, w[k] & 1u);
  }
}

// ---- EVT 2.0 ----
__global__ __launch_bounds__(EVT_THREADS) void k_evt2_trig_count(const u32* __restrict__ words, u32 n, const Evt2Scan* __restrict__ prefix,
                                                                 const Evt3State* __restrict__ st_in, u32* __restrict__ counts, int wait) {
  __shared__ ExtTrigScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  ExtTrigScan acc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc = evt_combine(acc, ext_trig_element(words[i0 + k] >> 28));
  ExtTrigScan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = ext_trig_emitted(total, wait && !st_in->have_high && !prefix[blockIdx.x].hi_word);
}

__global__ __launch_bounds__(EVT_THREADS) void k_evt2_trig_emit(const u32* __restrict__ words, u32 n, const Evt2Scan* __restrict__ prefix,
                                                                const Evt3State* __restrict__ st_in, u32* __restrict__ counts,
                                                                uint4* __restrict__ out, u32 out_cap, int wait) {
  __shared__ Evt2Scan buf[2][EVT_THREADS];
  __shared__ Evt2Scan s_incl[EVT_THREADS];
  __shared__ ExtTrigScan tbuf[2][EVT_THREADS];
  __shared__ ExtTrigScan s_tincl[EVT_THREADS];
  __shared__ u32 s_sum[EVT_THREADS];
  const unsigned long long loops0 = st_in->t_loops;
  const u32 have_high = st_in->have_high;
  const u32 offset = ext_trig_offset(counts, s_sum);
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  u32 w[EVT_IPT];
  Evt2Scan acc = evt2_identity();
  ExtTrigScan tacc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    w[k] = i0 + k < n ? words[i0 + k] : 0xE0000000u;  // (OTHERS: skipped)
    if (i0 + k < n) acc = evt_combine(acc, evt2_element(w[k]));
    tacc = evt_combine(tacc, ext_trig_element(w[k] >> 28));
  }
  Evt2Scan total;
  const Evt2Scan incl = evt_block_scan(acc, buf, &total);
  ExtTrigScan ttotal;
  const ExtTrigScan tincl = evt_block_scan(tacc, tbuf, &ttotal);
  s_incl[threadIdx.x] = incl;
  s_tincl[threadIdx.x] = tincl;
  __syncthreads();
  Evt2Scan run = prefix[blockIdx.x];
  const bool drop_pre = wait && !have_high && !run.hi_word;  // the block starts in front of the stream's first EVT_TIME_HIGH
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) counts[gridDim.x] = offset + ext_trig_emitted(ttotal, drop_pre);  // the chunk's total
  ExtTrigScan trun = ext_trig_element(0xEu);
  if (threadIdx.x) { run = evt_combine(run, s_incl[threadIdx.x - 1]); trun = s_tincl[threadIdx.x - 1]; }
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n) break;
    const u32 before = run.n_ev - evt_dropped(run.n_pre, have_high, wait);
    const u32 rank = ext_trig_emitted(trun, drop_pre);
    run = evt_combine(run, evt2_element(w[k]));
    trun = evt_combine(trun, ext_trig_element(w[k] >> 28));
    if ((w[k] >> 28) != 0xAu) continue;
    if (wait && !have_high && !run.hi_word) continue;  // in front of the stream's first EVT_TIME_HIGH: not emitted
    const unsigned long long t = ((loops0 + run.hi_wraps) << 34) | ((unsigned long long)run.hi_last << 6) | (unsigned long long)((w[k] >> 22) & 0x3fu);
    if (offset + rank < out_cap) out[offset + rank] = ext_trig_record(t, before, (w[k] >> 8) & 0x1fu, w[k] & 1u);
  }
}

// ---- EVT 2.1 ----
__global__ __launch_bounds__(EVT_THREADS) void k_evt21_trig_count(const unsigned long long* __restrict__ words, u32 n, const Evt21Scan* __restrict__ prefix,
                                                                  const Evt3State* __restrict__ st_in, u32* __restrict__ counts, int wait, int legacy) {
  __shared__ ExtTrigScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  ExtTrigScan acc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc = evt_combine(acc, ext_trig_element((u32)(evt21_load(words, i0 + k, legacy) >> 60)));
  ExtTrigScan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = ext_trig_emitted(total, wait && !st_in->have_high && !prefix[blockIdx.x].hi_word);
}

__global__ __launch_bounds__(EVT_THREADS) void k_evt21_trig_emit(const unsigned long long* __restrict__ words, u32 n, const Evt21Scan* __restrict__ prefix,
                                                                 const Evt3State* __restrict__ st_in, u32* __restrict__ counts,
                                                                 uint4* __restrict__ out, u32 out_cap, int wait, int legacy) {
  __shared__ Evt21Scan buf[2][EVT_THREADS];
  __shared__ Evt21Scan s_incl[EVT_THREADS];
  __shared__ ExtTrigScan tbuf[2][EVT_THREADS];
  __shared__ ExtTrigScan s_tincl[EVT_THREADS];
  __shared__ u32 s_sum[EVT_THREADS];
  const unsigned long long loops0 = st_in->t_loops;
  const u32 have_high = st_in->have_high;
  const u32 offset = ext_trig_offset(counts, s_sum);
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  unsigned long long w[EVT_IPT];
  Evt21Scan acc = evt21_identity();
  ExtTrigScan tacc = ext_trig_element(0xEu);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    w[k] = i0 + k < n ? evt21_load(words, i0 + k, legacy) : EVT21_SKIPPED;
    acc = evt_combine(acc, evt21_element(w[k]));
    tacc = evt_combine(tacc, ext_trig_element((u32)(w[k] >> 60)));
  }
  Evt21Scan total;
  const Evt21Scan incl = evt_block_scan(acc, buf, &total);
  ExtTrigScan ttotal;
  const ExtTrigScan tincl = evt_block_scan(tacc, tbuf, &ttotal);
  s_incl[threadIdx.x] = incl;
  s_tincl[threadIdx.x] = tincl;
  __syncthreads();
  Evt21Scan run = prefix[blockIdx.x];
  const bool drop_pre = wait && !have_high && !run.hi_word;  // the block starts in front of the stream's first EVT_TIME_HIGH
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) counts[gridDim.x] = offset + ext_trig_emitted(ttotal, drop_pre);  // the chunk's total
  ExtTrigScan trun = ext_trig_element(0xEu);
  if (threadIdx.x) { run = evt_combine(run, s_incl[threadIdx.x - 1]); trun = s_tincl[threadIdx.x - 1]; }
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n) break;
    const u32 before = run.n_ev - evt_dropped(run.n_pre, have_high, wait);
    const u32 rank = ext_trig_emitted(trun, drop_pre);
    run = evt_combine(run, evt21_element(w[k]));
    trun = evt_combine(trun, ext_trig_element((u32)(w[k] >> 60)));
    if ((u32)(w[k] >> 60) != 0xAu) continue;
    if (wait && !have_high && !run.hi_word) continue;  // in front of the stream's first EVT_TIME_HIGH: not emitted
    const unsigned long long t = ((loops0 + run.hi_wraps) << 34) | ((unsigned long long)run.hi_last << 6) | ((w[k] >> 54) & 0x3full);
    if (offset + rank < out_cap) out[offset + rank] = ext_trig_record(t, before, (u32)(w[k] >> 40) & 0x1fu, (u32)(w[k] >> 32) & 1u);
  }
}

// ---- the triggered frames' append (xm_trigframes_push with positive_only): a stable compaction of the chunk's EventCD records
// that keeps p == 1, and in the same pass the chunk's trigger indices remapped to "kept records with chunk index < event_index".
// Count per block of EVT_PER_BLOCK records -> every block folds the counts in front of it (ext_trig_offset), scans its keep flags
// and writes.  No atomics, no block waits for another.
struct KeepScan {
  u32 n;
};
__device__ __forceinline__ KeepScan evt_combine(const KeepScan& a, const KeepScan& b) { return KeepScan{a.n + b.n}; }

__device__ __forceinline__ u32 trig_keeps(const uint4 ev) { return (ev.y & 0xffffu) == 1u ? 1u : 0u; }  // (p: the int16 at byte 4)

__global__ __launch_bounds__(EVT_THREADS) void k_trig_keep_count(const uint4* __restrict__ ev, u32 n, u32* __restrict__ counts) {
  __shared__ KeepScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  KeepScan acc{0};
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc.n += trig_keeps(ev[i0 + k]);
  KeepScan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total.n;
}

// the first trigger whose event_index is >= e (triggers are in word order: their indices never fall)
__device__ __forceinline__ u32 trig_lower_bound(const uint4* __restrict__ trig, u32 n_trig, u32 e) {
  u32 lo = 0, hi = n_trig;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (trig[mid].z < e) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// out: room for out_cap records; remap[j] = trigger j's index among the kept records; counts[gridDim.x] = the kept total
__global__ __launch_bounds__(EVT_THREADS) void k_trig_keep_write(const uint4* __restrict__ ev, u32 n, u32* __restrict__ counts,
                                                                 uint4* __restrict__ out, u32 out_cap, const uint4* __restrict__ trig,
                                                                 u32 n_trig, u32* __restrict__ remap) {
  __shared__ KeepScan buf[2][EVT_THREADS];
  __shared__ KeepScan s_incl[EVT_THREADS];
  __shared__ u32 s_sum[EVT_THREADS];
  const u32 offset = ext_trig_offset(counts, s_sum);
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  uint4 r[EVT_IPT];
  KeepScan acc{0};
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    r[k] = i0 + k < n ? ev[i0 + k] : make_uint4(0, 0, 0, 0);
    if (i0 + k < n) acc.n += trig_keeps(r[k]);
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
    if (trig_keeps(r[k])) {
      if (at < out_cap) out[at] = r[k];
      at += 1;
    }
  }
  if (blockIdx.x == gridDim.x - 1) {
    const u32 kept = offset + total.n;
    if (threadIdx.x == 0) counts[gridDim.x] = kept;
    for (u32 q = trig_lower_bound(trig, n_trig, n) + threadIdx.x; q < n_trig; q += EVT_THREADS) remap[q] = kept;  // behind the chunk's last record
  }
}

}  // namespace xm
