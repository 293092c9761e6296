// xmaps_frameacc.hpp -- gfx950 device code the two frame stages share (xmaps_framesurface.hpp, xmaps_framecloud.hpp): the first
// pass of either walks a frame of EventCD records in chunks and reduces the extrema of t over the events that exist, and their
// count, into the frame's accumulator.  Inline functions and constants only: the kernels, their names, their launch shapes and
// their argument structs stay in the stage's own header.
//
// NOT here: the chunk load and the block reduction of the two first passes (k_fs_events, k_fc_extrema).  Their register allocation
// follows the smallest change in how the body reaches the compiler: with either written as a function -- taking the values,
// references to them, the LDS arrays or the whole argument struct; forced inline or not; even as ONE template that is the body of
// both kernels -- the two kernels' assembly differed from what it was (the same instructions on other registers, up to two more
// scalar registers), and the rule for this header is that no kernel's assembly moves (profiles/frame_stages_identity.md).  So
// k_fc_extrema stays k_fs_events without the map atomics, both written out, and the chunk load stays written out in the three
// kernels that have it; what they share by name is below.
//
// Accumulator encoding: a time stamp t is ordered as u = t ^ 2^63; the accumulator keeps max(~u) (-> the minimum) and max(u) (-> the
// maximum), so that all-zero words are neutral for every field and nothing has to be initialised per call.  An accumulator (FsAcc,
// FcAcc) starts with u64 min_enc, u64 max_enc, u32 n_events; what follows is the stage's own.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

constexpr int FRAME_THREADS = 256;                      // threads per block of a per-event pass
constexpr int FRAME_EPT = 4;                            // events per thread (independent 16-byte loads in flight)
constexpr int FRAME_CHUNK = FRAME_THREADS * FRAME_EPT;  // events per block and trip of its chunk loop
constexpr int FRAME_GROUP = 32;                         // frames per launch sequence

__device__ inline u64 frame_enc(long long t) { return (u64)t ^ (1ull << 63); }
__device__ inline long long frame_dec(u64 u) { return (long long)(u ^ (1ull << 63)); }

// does the event exist at all (with use_polarity: only p == 1 does)
__device__ inline bool frame_exists(int use_polarity, const uint4& r) { return !use_polarity || (short)(r.y & 0xffffu) == 1; }

// ingest: the ring entry is about to be rewritten by a later launch of this frame's sequence
__device__ inline void frame_tag_clear(u64* tag) {
  if (tag && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(tag, 0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace xm
