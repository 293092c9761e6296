// xmaps_evt3enc.hpp -- gfx950 device code of the frame -> EVT 3.0 entry (xm_frames_to_evt3_words, and the same kernels as a stage of
// the device ingest: xm_ingest_set_record_output): a GROUP of frames of EventCD records -> per frame the words
// x_maps_amd.evt3.encode_evt3(frame, use_vectors) writes, the encoder's state fresh for every frame.  include/xmaps.h states the
// rule in the parallel form evaluated here (links, chains, run starts, the words in front of a run start).
//
// Per launch sequence (at most ENC_GROUP frames, grid = blocks x frames), every dependency between blocks a kernel boundary:
//   R0 k_enc_runs    per event: is it linked to its predecessor?  The lane of an event that is NOT (a chain head) walks its chain:
//                    run start -> next(run start), at most 12 events further each time, and writes the 2-byte code of EVERY event of
//                    the chain -- ENC_START | the time / row words in front (only a head can have any: a linked event shares t and
//                    y with its predecessor) | the run's VECT_12 bits 1 .. 11 for a run start, 0 for the other events of a run;
//                    bit 0 of either: the event is out of the format's range.  Every event lies in exactly one chain, so every code
//                    of the frame is written once, by a plain store of the head's lane, whichever segment or block the chain
//                    reaches into; a chain holds at most 65 536 events (strictly increasing u16 columns), which bounds the walk
//   R1 k_enc_count   per 64 consecutive events (one wave instruction): words, vector runs, events out of range, from the codes
//   R2 k_enc_scan    one block per frame: exclusive scan of the frame's 64-event word counts (stream order) + the frame's statistics
//   R3 k_enc_emit    stable emit in stream order: ballot + mbcnt of the five kinds of word inside the 64 events, the scanned offset
//                    in front; every word one plain 2-byte store of the run start's lane.  Words past the frame's n_words are not
//                    touched; a frame with more than max_words words (ingest) writes none
//   R4 k_enc_publish (ingest only) the statistics and the ring entry's tag into pinned host memory, behind R3
// No atomic anywhere; no block waits for or spins on another block of its launch.  A frame longer than the grid covers (ENC_CHUNK
// events per block, at most max_chunk_blocks blocks: "XM_ENC_MAX_BLOCKS") takes further trips of a chunk loop; the mapping event ->
// (wave, lane) is the same in R1 and R3 on every trip, so the 64 events of one count are the 64 lanes of one wave instruction in both.
// From xmaps_frameacc.hpp: the block geometry of a per-event pass, the frames per launch sequence, frame_tag_clear.
#pragma once
#include "xmaps_common.hpp"
#include "xmaps_frameacc.hpp"

namespace xm {

constexpr int ENC_THREADS = FRAME_THREADS;  // threads per block (R0, R1, R3)
constexpr int ENC_EPT = FRAME_EPT;          // events per thread and trip
constexpr int ENC_CHUNK = FRAME_CHUNK;      // events per block and trip of its chunk loop
constexpr int ENC_GROUP = FRAME_GROUP;      // frames per launch sequence
constexpr int ENC_SCAN_BLOCK = 1024;        // R2
constexpr u32 ENC_RUN_COLS = 12;            // columns a run may span (one VECT_12)

// an event's code (R0)
constexpr u32 ENC_START = 0x8000u, ENC_HI = 0x4000u, ENC_LO = 0x2000u, ENC_Y = 0x1000u;  // a run start; TIME_HIGH / TIME_LOW / ADDR_Y in front
constexpr u32 ENC_VECT = 0x0ffeu;  // a run start's VECT_12 bits 1 .. 11 (bit 0 is the start itself): non-zero = a run of >= 2 events
constexpr u32 ENC_OOR = 0x0001u;   // the event's fields do not fit the format (counted, not refused)

struct EncStats {  // == xm_evt3_record_stats (include/xmaps.h)
  u64 n_events, n_words, n_vector_runs, n_out_of_range;
  long long t_first, t_last;
};

struct EncArgs {          // by value to the kernels
  const uint4* ev;        // the record array (group entry) ...
  u64 first[ENC_GROUP];   // ... frame f = records [first[f], first[f] + n[f]); its codes start at first[f], its words at 4 * first[f]
  u32 n[ENC_GROUP];
  u32 seg0[ENC_GROUP];    // the frame's first 64-event count
  const FrameDesc* desc;  // ingest: ONE frame, described on the device (aos, n, valid); ev / first / n / seg0 unused
  u32 cap;                // ingest: the events the scratch holds (a cut frame never has more; the kernels clamp to it)
  u32 max_words;          // words a frame may write (ingest: the ring entry's room, all or nothing; group entry: no limit)
  uint16_t* code;         // per event
  uint2* cnt;             // per 64 events: {words, vector runs | events out of range << 16}
  u32* off;               // per 64 events: words of the frame in front of them (R2)
  EncStats* stats;        // [frames of the sequence]
  uint16_t* words;        // [4 * events]
  u64* tag;               // ingest: the ring entry's tag in pinned host memory (R0 clears it, R4 sets it), else NULL
  u64 tag_value;
  EncStats* host_stats;   // ingest: the ring entry's statistics in pinned host memory (R4)
  int use_vectors;
  u32 max_chunk_blocks;   // grid.x of R0 / R1 / R3 is at most this
};

struct EncFrameRef {
  const uint4* ev;
  u64 n, base;  // events; index of the frame's first code (its first word: 4 * base)
  u32 seg0;
};
__device__ inline EncFrameRef enc_frame(const EncArgs& a, u32 f) {
  if (a.desc) {
    if (!a.desc->valid) return EncFrameRef{nullptr, 0, 0, 0};
    const u64 n = a.desc->n;
    return EncFrameRef{a.desc->aos, n < a.cap ? n : a.cap, 0, 0};
  }
  return EncFrameRef{a.ev + a.first[f], a.n[f], a.first[f], a.seg0[f]};
}

// record fields as the host encoder reads them: x, y raw u16; p the raw int16 (the record's bytes 4, 5); t the int64
__device__ inline u32 enc_p(const uint4& r) { return r.y & 0xffffu; }
// event b directly behind event a: linked iff t, y and the raw p are equal and the raw column grows
__device__ inline bool enc_linked(const uint4& a, const uint4& b) {
  return a.z == b.z && a.w == b.w && rec_y(a) == rec_y(b) && enc_p(a) == enc_p(b) && rec_x(b) > rec_x(a);
}
__device__ inline u32 enc_oor(const uint4& r) {  // x > 2047, y > 2047, p not in {0, 1} or t < 0
  return (rec_x(r) > 2047u || rec_y(r) > 2047u || enc_p(r) > 1u || (int)r.w < 0) ? ENC_OOR : 0u;
}
__device__ inline u32 enc_hi(const uint4& r) { return (r.z >> 12) & 0xfffu; }
__device__ inline u32 enc_lo(const uint4& r) { return r.z & 0xfffu; }

// what the five ballots of a segment's codes say to one lane: words of the lanes below it / of the whole segment
struct EncBallots {
  u64 hi, lo, y, start, vect;
  __device__ u32 below() const {
    return enc_mbcnt(hi) + enc_mbcnt(lo) + enc_mbcnt(y) + enc_mbcnt(start) + enc_mbcnt(vect);
  }
  __device__ u32 total() const { return (u32)(__popcll(hi) + __popcll(lo) + __popcll(y) + __popcll(start) + __popcll(vect)); }
  __device__ static u32 enc_mbcnt(u64 b) { return __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u)); }
};
__device__ inline EncBallots enc_ballots(u32 c) {  // (every lane of the wave calls it; c == 0: no event)
  const bool st = (c & ENC_START) != 0;
  return EncBallots{__ballot(st && (c & ENC_HI)), __ballot(st && (c & ENC_LO)), __ballot(st && (c & ENC_Y)), __ballot(st),
                    __ballot(st && (c & ENC_VECT))};
}

// R0 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ENC_THREADS) void k_enc_runs(EncArgs a) {
  const u32 f = blockIdx.y, tid = threadIdx.x;
  frame_tag_clear(a.tag);  // (R3 of this frame rewrites the ring entry)
  const EncFrameRef fr = enc_frame(a, f);
  uint16_t* code = a.code + fr.base;
  const bool vectors = a.use_vectors != 0;
  for (u64 c0 = (u64)blockIdx.x * ENC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * ENC_CHUNK) {  // (block-uniform)
#pragma unroll 1
    for (int k = 0; k < ENC_EPT; ++k) {
      const u64 i = c0 + (u64)k * ENC_THREADS + tid;
      if (i >= fr.n) break;
      uint4 rc = fr.ev[i];
      u32 hdr = ENC_HI | ENC_LO | ENC_Y;  // the frame's first event
      if (i > 0) {
        const uint4 rp = fr.ev[i - 1];
        if (vectors && enc_linked(rp, rc)) continue;  // not a chain head: its code is the head's lane's to write
        const bool hi = enc_hi(rp) != enc_hi(rc);
        hdr = (hi ? ENC_HI | ENC_LO : 0u) | (enc_lo(rp) != enc_lo(rc) ? ENC_LO : 0u) | (rec_y(rp) != rec_y(rc) ? ENC_Y : 0u);
      }
      // the chain from its head: cur = the run start, j = the event under test (cur < j <= cur + 12, j < n before every access)
      u64 cur = i;
      for (;;) {
        u32 bits = 0;
        bool more = false;
        uint4 rl = rc, rj = rc;  // the event in front of j; event j
        u64 j = cur + 1;
        while (vectors && j < fr.n) {
          rj = fr.ev[j];
          if (!enc_linked(rl, rj)) break;  // the chain ends in front of j
          const u32 d = rec_x(rj) - rec_x(rc);
          if (d >= ENC_RUN_COLS) {  // j = next(cur): the next run start
            more = true;
            break;
          }
          bits |= 1u << d;
          code[j] = (uint16_t)enc_oor(rj);
          rl = rj;
          j += 1;
        }
        code[cur] = (uint16_t)(ENC_START | hdr | bits | enc_oor(rc));
        if (!more) break;
        cur = j;
        rc = rj;
        hdr = 0;  // (linked to its predecessor: same t, same y)
      }
    }
  }
}

// R1 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ENC_THREADS) void k_enc_count(EncArgs a) {
  const u32 f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const EncFrameRef fr = enc_frame(a, f);
  const uint16_t* code = a.code + fr.base;
  uint2* cnt = a.cnt + fr.seg0;
  for (u64 c0 = (u64)blockIdx.x * ENC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * ENC_CHUNK) {  // (block-uniform)
#pragma unroll
    for (int k = 0; k < ENC_EPT; ++k) {
      const u64 w0 = c0 + (u64)k * ENC_THREADS + (tid & ~63u), i = w0 + lane;  // w0: the wave's first event, a multiple of 64
      if (w0 >= fr.n) break;                                                     // (wave-uniform)
      const u32 c = i < fr.n ? (u32)code[i] : 0u;
      const EncBallots b = enc_ballots(c);
      const u64 b_oor = __ballot((c & ENC_OOR) != 0);
      if (lane == 0) cnt[w0 >> 6] = make_uint2(b.total(), (u32)__popcll(b.vect) | (u32)__popcll(b_oor) << 16);
    }
  }
}

// R2 ------------------------------------------------------------------------------------------------------------------------
// one block per frame: off = exclusive scan of the word counts of the frame's ceil(n / 64) segments, the frame's statistics
__global__ __launch_bounds__(ENC_SCAN_BLOCK) void k_enc_scan(EncArgs a) {
  __shared__ u32 s_w[ENC_SCAN_BLOCK / 64], s_v[ENC_SCAN_BLOCK / 64], s_oor[ENC_SCAN_BLOCK / 64];
  const u32 f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const EncFrameRef fr = enc_frame(a, f);
  const u32 n_seg = (u32)((fr.n + 63) >> 6);
  const uint2* cnt = a.cnt + fr.seg0;
  u32* off = a.off + fr.seg0;
  const u32 ipt = (n_seg + ENC_SCAN_BLOCK - 1) / ENC_SCAN_BLOCK;  // consecutive segments per thread
  const u32 first = tid * ipt < n_seg ? tid * ipt : n_seg, last = first + ipt < n_seg ? first + ipt : n_seg;
  u32 sum = 0, vect = 0, oor = 0;
  for (u32 i = first; i < last; ++i) {
    const uint2 c = cnt[i];
    sum += c.x;
    vect += c.y & 0xffffu;
    oor += c.y >> 16;
  }
  u32 incl = sum;  // inclusive scan over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 up = __shfl_up(incl, o, 64);
    if (lane >= (u32)o) incl += up;
  }
  vect = wave_sum_u32(vect);
  oor = wave_sum_u32(oor);
  if (lane == 63) s_w[wave] = incl;
  if (lane == 0) s_v[wave] = vect, s_oor[wave] = oor;
  __syncthreads();
  u32 before = 0, total = 0, vect_total = 0, oor_total = 0;
#pragma unroll
  for (int w = 0; w < ENC_SCAN_BLOCK / 64; ++w) {
    before += (u32)w < wave ? s_w[w] : 0u;
    total += s_w[w];
    vect_total += s_v[w];
    oor_total += s_oor[w];
  }
  u32 run = before + incl - sum;
  for (u32 i = first; i < last; ++i) {
    off[i] = run;
    run += cnt[i].x;
  }
  if (tid == 0) {
    EncStats s{0, 0, 0, 0, 0, 0};
    if (fr.n) s = EncStats{fr.n, total, vect_total, oor_total, rec_t<long long>(fr.ev[0]), rec_t<long long>(fr.ev[fr.n - 1])};
    a.stats[f] = s;
  }
}

// R3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ENC_THREADS) void k_enc_emit(EncArgs a) {
  const u32 f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const EncFrameRef fr = enc_frame(a, f);
  if (a.stats[f].n_words > (u64)a.max_words) return;  // (R2 has finished: a plain load.  All or nothing; block-uniform)
  const uint16_t* code = a.code + fr.base;
  const u32* off = a.off + fr.seg0;
  uint16_t* words = a.words + fr.base * 4;
  for (u64 c0 = (u64)blockIdx.x * ENC_CHUNK; c0 < fr.n; c0 += (u64)gridDim.x * ENC_CHUNK) {  // (block-uniform)
#pragma unroll
    for (int k = 0; k < ENC_EPT; ++k) {
      const u64 w0 = c0 + (u64)k * ENC_THREADS + (tid & ~63u), i = w0 + lane;
      if (w0 >= fr.n) break;  // (wave-uniform)
      const u32 c = i < fr.n ? (u32)code[i] : 0u;
      const EncBallots b = enc_ballots(c);
      if (!(c & ENC_START)) continue;
      const uint4 r = fr.ev[i];
      uint16_t* w = words + (off[w0 >> 6] + b.below());  // < 4 * n: R1 counted exactly the words written here
      if (c & ENC_HI) *w++ = (uint16_t)(0x8000u | enc_hi(r));
      if (c & ENC_LO) *w++ = (uint16_t)(0x6000u | enc_lo(r));
      if (c & ENC_Y) *w++ = (uint16_t)(rec_y(r) & 0x7ffu);
      const u32 xp = ((enc_p(r) & 1u) << 11) | (rec_x(r) & 0x7ffu);
      if (c & ENC_VECT) {
        w[0] = (uint16_t)(0x3000u | xp);
        w[1] = (uint16_t)(0x4000u | (c & ENC_VECT) | 1u);
      } else {
        w[0] = (uint16_t)(0x2000u | xp);
      }
    }
  }
}

// R4 ------------------------------------------------------------------------------------------------------------------------
// ingest: statistics, then the tag behind them, where xm_ingest_copy_record reads both without a copy
__global__ __launch_bounds__(64) void k_enc_publish(EncArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *a.host_stats = a.stats[0];
  __hip_atomic_store(a.tag, a.tag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace xm
