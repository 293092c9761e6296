// xmaps_evt.hpp -- what the device decoders of Prophesee's four recording formats share (xmaps_evt3.hpp: EVT 3.0, xmaps_evt2.hpp:
// EVT 2.0, xmaps_evt21.hpp: EVT 2.1, xmaps_dat.hpp: DAT; each includes this file, none includes another).  (gfx950 / MI355X)
//
// Every format is a state machine over its words, and every piece of that state at word i is "the value of the last word of type T
// at or before i" or a sum over the words before i: an inclusive scan with an associative combine, evaluated in three launches
// per chunk of EVT_PER_BLOCK-word blocks: block aggregates -> their exclusive scan in one block, EVT_THREADS of them per trip with
// the range read so far carried from trip to trip, seeded with the state the previous chunk left (which also writes the next state
// and the chunk's event count) -> every block re-scans its words from its prefix and writes its records in word order (EVT 2.1,
// whose words are up to 32 events each, has a second emit kernel that writes by output slot: xmaps_evt21.hpp).
// Here: the block geometry, the state record a chunk hands to the next one, the start-of-stream rule and the block scan (over a
// format's scan record and its evt_combine overload).  The three kernel bodies stay spelled out per format: shared as inlined
// templates they compile to different device code (profiles/evt_skeleton_identity.md lists the shapes that were tried).
#pragma once
#include "xmaps_common.hpp"

namespace xm {

constexpr int EVT_THREADS = 256, EVT_IPT = 8, EVT_PER_BLOCK = EVT_THREADS * EVT_IPT;

// What a chunk hands to the next one (Evt3Decoder's fields in x_maps_amd/evt3.py; EVT 2.0 and EVT 2.1 use t_high, t_loops,
// have_high and n_events, DAT t_high -- its last stamp --, t_loops and n_events; they leave the rest 0).  The name is EVT 3.0's because the kernels' mangled names carry it.
struct Evt3State {
  u32 y, base_x, base_p, t_high, t_low;
  u32 have_high;  // a TIME_HIGH word has been seen since the stream started (the "wait for the time base" option drops events before it)
  unsigned long long t_loops;
  unsigned long long n_events;  // of the chunk that wrote this state
};

// Start-of-stream rule (an option of the decoder, xm_evt3_wait_for_time_base): events in front of the stream's FIRST TIME_HIGH word
// carry a time of which only the low bits are known.  Off (default): they are emitted with the high field at its initial 0,
// like everything else the initial state defines.  On: they are not emitted (a reader that waits for the first time base).
// A scan record counts them: hi_word = a TIME_HIGH WORD lies in the range (the seed is not one), n_pre = the events in front of
// the range's first one.
__device__ __forceinline__ u32 evt_dropped(const u32 n_pre, const u32 have_high, const int wait) { return wait && !have_high ? n_pre : 0u; }

// inclusive scan of one element per thread over the block (Hillis-Steele on two LDS buffers); returns the thread's inclusive
// result, *block_total = the block's aggregate
template <class Scan>
__device__ __forceinline__ Scan evt_block_scan(const Scan mine, Scan (*buf)[EVT_THREADS], Scan* block_total) {
  const int tid = threadIdx.x;
  int cur = 0;
  buf[0][tid] = mine;
  __syncthreads();
  for (int o = 1; o < EVT_THREADS; o <<= 1) {
    Scan v = buf[cur][tid];
    if (tid >= o) v = evt_combine(buf[cur][tid - o], v);
    buf[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  const Scan r = buf[cur][tid];
  *block_total = buf[cur][EVT_THREADS - 1];
  __syncthreads();
  return r;
}

}  // namespace xm
