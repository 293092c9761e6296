// xmaps_slots.hpp -- housekeeping of a slot's device state: (re)initialisation, and forgetting a failed column-tile attempt's
// counts before the frame is redone inside a captured batch.  No reference lines: the slots are this build's.  (gfx950 / MI355X)
//
// Needs xmaps_common.hpp.
#pragma once
#include "xmaps_common.hpp"

namespace xm {

// slot (re)initialisation: zero the key frame, arm min/max + counters, tag = 0
__global__ __launch_bounds__(BLOCK) void k_reset_slot(SlotState* st, u64* __restrict__ frame, u64 n_cells,
                                                      unsigned char* __restrict__ dirty) {
  const u64 stride = (u64)gridDim.x * BLOCK;
  for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < n_cells; i += stride) frame[i] = 0;
  if (dirty)
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i < ((n_cells + 15) >> 4); i += stride) dirty[i] = 0;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      st->tag_a = 0;
      st->tag_b = 0;
      st->pad[1] = 0;  // (frame_attempt_failed: tags start over, a stale tag of the old numbering must not match a new one)
      // unsorted_sticky is NOT cleared here: this kernel also runs on tag wrap, and a violation recorded since the last
      // xm_sync must still be reported; it starts at 0 (xm_create zeroes the states) and xm_sync clears it
    }
    for (int i = threadIdx.x; i < 2 * MM_SLOTS; i += BLOCK) {
      st->mm[i / MM_SLOTS][i % MM_SLOTS][0] = MM_INIT_MIN;
      st->mm[i / MM_SLOTS][i % MM_SLOTS][1] = MM_INIT_MAX;
    }
    for (int i = threadIdx.x; i < 2 * CNT_SLOTS * CNT_STRIDE; i += BLOCK) (&st->cnt[0][0][0])[i] = 0;
  }
}

// A frame of a captured batch whose column-tile attempt failed: forget what the attempt counted (same tag, same parity) before
// K0 / K1 / K2 of the 64-bit path run on it.  grid = frames.
__global__ __launch_bounds__(64) void k_redo_prepare_batch(const FrameDesc* __restrict__ descs) {
  const FrameDesc d = descs[blockIdx.x];
  if (!d.valid || !frame_attempt_failed(d.st)) return;
  const u32 parity = d.st->tag_a & 1;
  for (int i = threadIdx.x; i < CNT_SLOTS * CNT_STRIDE; i += 64) (&d.st->cnt[parity][0][0])[i] = 0;
}

}  // namespace xm
