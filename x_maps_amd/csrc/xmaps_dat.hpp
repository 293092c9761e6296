// xmaps_dat.hpp -- Prophesee DAT (version 2, CD events) records -> EventCD records on the device: the other
// container the reference's --input takes.  (gfx950 / MI355X; included by xmaps_hip.hip.)  x_maps_amd/dat.py restates the format
// on the host (and reads the header: '%' lines, then the event type 0x0C and the event size 8), tests/dat_ref.py is the
// independent record-by-record checker.
//
//   8-byte records, little-endian:  u32 ts (us)   u32 data: [13:0] x   [27:14] y   [31:28] p        every record is one event
//   t = (loops << 32) | ts; a loop: ts falls back by more than 2^31 against the record before it (smaller steps back are kept).
//
// The state at record i is the number of loops so far: a scan over {n_ev, first ts, last ts, wraps} in the three launches every
// decoder here has (xmaps_evt.hpp); the emit is elementwise from the prefix, record i of the chunk is event i.  The state record is
// EVT 3.0's: t_high = the last ts, t_loops, n_events.  The seed -- the record in front of the chunk -- counts as one record of
// the scan (a range is empty where n_ev == 0), which the prefix kernel takes off again; a stream starts with ts = 0 in front of
// it, which no first record can fall back from.  The "wait for the time base" option has nothing to wait for here.
#pragma once
#include "xmaps_evt.hpp"

namespace xm {

struct DatScan {
  u32 n_ev, ts_first, ts_last, wraps;
};

__device__ __forceinline__ DatScan dat_identity() {
  DatScan e;
  e.n_ev = e.ts_first = e.ts_last = e.wraps = 0;
  return e;
}

// a = the earlier range, b = the later one
__device__ __forceinline__ DatScan evt_combine(const DatScan& a, const DatScan& b) {
  if (!b.n_ev) return a;
  if (!a.n_ev) return b;
  DatScan r;
  r.n_ev = a.n_ev + b.n_ev;
  r.ts_first = a.ts_first;
  r.ts_last = b.ts_last;
  r.wraps = a.wraps + b.wraps + ((long long)a.ts_last - (long long)b.ts_first > (1ll << 31) ? 1u : 0u);
  return r;
}

__device__ __forceinline__ DatScan dat_element(unsigned long long rec) {
  DatScan e;
  e.n_ev = 1;
  e.ts_first = e.ts_last = (u32)rec;
  e.wraps = 0;
  return e;
}

// 1. the aggregate of every block of EVT_PER_BLOCK records
__global__ __launch_bounds__(EVT_THREADS) void k_dat_aggregate(const unsigned long long* __restrict__ recs, u32 n, DatScan* __restrict__ agg) {
  __shared__ DatScan buf[2][EVT_THREADS];
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  DatScan acc = dat_identity();
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k)
    if (i0 + k < n) acc = evt_combine(acc, dat_element(recs[i0 + k]));
  DatScan total;
  (void)evt_block_scan(acc, buf, &total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// 2. one block: exclusive scan of the aggregates, seeded with the record in front of the chunk (n_ev counts it: + 1 in every
//    prefix); the chunk's event count and the state for the next chunk
__global__ __launch_bounds__(EVT_THREADS) void k_dat_prefix(u32 n_blocks, DatScan* __restrict__ agg, const Evt3State* __restrict__ st_in,
                                                            Evt3State* __restrict__ st_out, u32* __restrict__ count_out) {
  __shared__ DatScan buf[2][EVT_THREADS];
  __shared__ DatScan s_incl[EVT_THREADS];
  const Evt3State s = *st_in;
  DatScan carry;
  carry.n_ev = 1;
  carry.ts_first = carry.ts_last = s.t_high;
  carry.wraps = 0;
  for (u32 b0 = 0; b0 < n_blocks; b0 += EVT_THREADS) {
    const u32 b = b0 + threadIdx.x;
    const DatScan mine = b < n_blocks ? agg[b] : dat_identity();
    DatScan total;
    const DatScan incl = evt_block_scan(mine, buf, &total);
    s_incl[threadIdx.x] = incl;
    __syncthreads();
    if (b < n_blocks) agg[b] = threadIdx.x ? evt_combine(carry, s_incl[threadIdx.x - 1]) : carry;
    carry = evt_combine(carry, total);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Evt3State o;
    o.y = o.base_x = o.base_p = o.t_low = 0;
    o.have_high = s.have_high;
    o.t_high = carry.ts_last;
    o.t_loops = s.t_loops + carry.wraps;
    o.n_events = carry.n_ev - 1u;
    *st_out = o;
    if (count_out) *count_out = (u32)o.n_events;  // (a cell of the consumer's: this record is rewritten two chunks from now)
  }
}

// 3. the records: every block re-scans its records from its exclusive prefix; record i of the chunk is event i
__global__ __launch_bounds__(EVT_THREADS) void k_dat_emit(const unsigned long long* __restrict__ recs, u32 n, const DatScan* __restrict__ prefix,
                                                          const Evt3State* __restrict__ st_in, uint4* __restrict__ out, u32 out_cap) {
  __shared__ DatScan buf[2][EVT_THREADS];
  __shared__ DatScan s_incl[EVT_THREADS];
  const unsigned long long loops0 = st_in->t_loops;
  const u32 i0 = blockIdx.x * EVT_PER_BLOCK + threadIdx.x * EVT_IPT;
  unsigned long long r[EVT_IPT];
  DatScan acc = dat_identity();
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    r[k] = i0 + k < n ? recs[i0 + k] : 0ull;
    if (i0 + k < n) acc = evt_combine(acc, dat_element(r[k]));
  }
  DatScan total;
  const DatScan incl = evt_block_scan(acc, buf, &total);
  s_incl[threadIdx.x] = incl;
  __syncthreads();
  DatScan run = prefix[blockIdx.x];
  if (threadIdx.x) run = evt_combine(run, s_incl[threadIdx.x - 1]);
#pragma unroll
  for (int k = 0; k < EVT_IPT; ++k) {
    if (i0 + k >= n || i0 + k >= out_cap) break;
    run = evt_combine(run, dat_element(r[k]));
    const unsigned long long t = ((loops0 + run.wraps) << 32) | (unsigned long long)(u32)r[k];
    const u32 data = (u32)(r[k] >> 32);
    out[i0 + k] = make_uint4((data & 0x3fffu) | (((data >> 14) & 0x3fffu) << 16), data >> 28, (u32)t, (u32)(t >> 32));
  }
}

}  // namespace xm
