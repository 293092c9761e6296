// xm_ring_tag.hpp -- the ingest's per-frame output rings (surface, cloud and record stage): which entry a frame takes and what its tag says
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; standard C++ only, so that a CPU
// test can build it alone: tests/c_host/scratch_order_host.cpp)
//
// Frame `seq` (from 0) goes to entry seq % ring.  The entry's tag is 0 while the entry is being rewritten, else it names the frame
// whose output the entry holds: seq + 1 for a cloud or a record (the record stage uses cloud_tag as it is); (seq + 1) << 2 | dtype for a surface, whose entry has room for either dtype
// (XM_T_FLOAT32 / XM_T_FLOAT64: 1 / 2, the two low bits).  seq + 1 is taken as 64-bit arithmetic gives it: a surface tag has 62 bits
// for it, so frame 2^62 - 1 would publish the bare dtype, which names no frame.
#pragma once

#include <cstddef>
#include <cstdint>

namespace {

inline size_t ring_entry(uint64_t seq, int ring) { return (size_t)(seq % (uint64_t)ring); }

inline uint64_t cloud_tag(uint64_t seq) { return seq + 1; }
inline bool cloud_tag_names(uint64_t tag, uint64_t seq) { return tag == seq + 1; }

inline uint64_t surface_tag(uint64_t seq, int dtype) { return ((seq + 1) << 2) | (uint64_t)dtype; }
inline bool surface_tag_names(uint64_t tag, uint64_t seq) { return tag >> 2 == seq + 1; }
inline int surface_tag_dtype(uint64_t tag) { return (int)(tag & 3); }

}  // namespace
