// trigger_cut_host.cpp -- the cut rule of the triggered frames (x_maps_amd/csrc/host/xm_trigger_cut.hpp; include/xmaps.h states it),
// built alone (tests/test_ext_trigger_cpu.py: g++, AddressSanitizer + UBSan).  Every expectation below is a literal worked out by
// hand from the rule; tests/test_ext_trigger_cpu.py runs the same cases against the Python mirror (TriggerFrameCutter).
// Prints "ok"; at the first mismatch the case's name, and exits 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/xmaps.h"
#include "../../x_maps_amd/csrc/host/xm_trigger_cut.hpp"

#define EQ(name, got, want)                                                                                        \
  do {                                                                                                             \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                                 \
    if (g_ != w_) {                                                                                                \
      printf("MISMATCH %s: %s = %lld, expected %lld (line %d)\n", name, #got, g_, w_, __LINE__);                   \
      exit(1);                                                                                                     \
    }                                                                                                              \
  } while (0)

static TrigCutter cutter(uint64_t cap, int id, int edge, uint64_t min_events, int max_ready) {
  TrigCutter c;
  c.cfg.struct_size = sizeof(xm_trigframes_config);
  c.cfg.cap_events = cap, c.cfg.id = id, c.cfg.edge = edge, c.cfg.min_events = min_events, c.cfg.max_frames_ready = max_ready;
  return c;
}

struct T {
  uint32_t idx;
  int id, value;
};

// one push: room for n events (no compaction: n_in = n_kept), then the append; returns room().rc
static int push(TrigCutter& c, uint64_t n, std::vector<T> ts, TrigRoom* room_out = nullptr) {
  const TrigRoom r = c.room(n);
  if (room_out) *room_out = r;
  if (r.rc) return r.rc;
  std::vector<xm_ext_trigger> tr;
  for (const T& t : ts) {
    xm_ext_trigger x{};
    x.t = 1000 + t.idx, x.event_index = t.idx, x.id = (uint8_t)t.id, x.value = (uint8_t)t.value;
    tr.push_back(x);
  }
  c.append(n, n, tr.data(), tr.size());
  return 0;
}

static void frame(const char* name, const TrigCutter& c, size_t f, uint64_t begin, uint64_t end) {
  EQ(name, f < c.ready.size(), 1);
  EQ(name, c.ready[f].begin, begin);
  EQ(name, c.ready[f].end, end);
}

int main() {
  {  // A: two chunks, a falling edge in between is not selected
    const char* n = "A";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 0, 0);
    EQ(n, push(c, 10, {{3, 0, 1}, {7, 0, 0}, {8, 0, 1}}), 0);
    EQ(n, c.ready.size(), 1);
    frame(n, c, 0, 3, 8);
    EQ(n, c.ready[0].opening.t, 1003);
    EQ(n, c.lo, 3);
    EQ(n, c.hi, 10);
    EQ(n, push(c, 5, {{0, 0, 1}, {5, 0, 1}}), 0);
    EQ(n, c.ready.size(), 3);
    frame(n, c, 1, 8, 10);
    frame(n, c, 2, 10, 15);
    EQ(n, c.run(10), 3);
    EQ(n, c.run(2), 2);
    c.release(3);
    EQ(n, c.ready.size(), 0);
    EQ(n, c.open, 1);
    EQ(n, c.lo, 15);
    EQ(n, c.hi, 15);
    EQ(n, c.stream_pos, 15);
    EQ(n, c.st.events_in, 15);
    EQ(n, c.st.events_kept, 15);
    EQ(n, c.st.triggers_seen, 5);
    EQ(n, c.st.triggers_selected, 4);
    EQ(n, c.st.frames_cut, 3);
    EQ(n, c.st.frames_skipped, 0);
    EQ(n, c.st.events_before_first_trigger, 3);
    EQ(n, c.st.events_dropped_open_frame, 0);
    EQ(n, c.st.front_moves, 0);
  }
  {  // B: min_events = 2 skips frames of 1 and 2 events; a skipped frame ends a run
    const char* n = "B";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 2, 0);
    EQ(n, push(c, 12, {{0, 0, 1}, {5, 0, 1}, {6, 0, 1}, {8, 0, 1}, {12, 0, 1}}), 0);
    EQ(n, c.ready.size(), 2);
    frame(n, c, 0, 0, 5);
    frame(n, c, 1, 8, 12);
    EQ(n, c.st.frames_cut, 2);
    EQ(n, c.st.frames_skipped, 2);
    EQ(n, c.run(10), 1);
    c.release(1);
    EQ(n, c.run(10), 1);
    frame(n, c, 0, 8, 12);
    EQ(n, c.lo, 8);
  }
  {  // C: max_frames_ready = 2
    const char* n = "C";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 0, 2);
    EQ(n, push(c, 6, {{0, 0, 1}, {1, 0, 1}, {2, 0, 1}, {3, 0, 1}, {4, 0, 1}}), 0);
    EQ(n, c.ready.size(), 4);
    EQ(n, c.run(10), 2);
    EQ(n, c.run(1), 1);
    c.release(2);
    EQ(n, c.run(10), 2);
    frame(n, c, 0, 2, 3);
    c.release(2);
    EQ(n, c.run(10), 0);
    EQ(n, c.lo, 4);
    EQ(n, c.hi, 6);
  }
  {  // D: three adjacent triggers: two empty frames, delivered with min_events = 0
    const char* n = "D";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 0, 0);
    EQ(n, push(c, 4, {{2, 0, 1}, {2, 0, 1}, {2, 0, 1}}), 0);
    EQ(n, c.ready.size(), 2);
    frame(n, c, 0, 2, 2);
    frame(n, c, 1, 2, 2);
    EQ(n, c.run(10), 2);
    EQ(n, c.st.events_before_first_trigger, 2);
    TrigCutter s = cutter(100, -1, XM_TRIG_RISING, 1, 0);  // ... and skipped with min_events = 1
    EQ(n, push(s, 4, {{2, 0, 1}, {2, 0, 1}, {2, 0, 1}}), 0);
    EQ(n, s.ready.size(), 0);
    EQ(n, s.st.frames_skipped, 2);
  }
  {  // E: channel and edge selection with interleaved channels
    const char* n = "E";
    TrigCutter c = cutter(100, 1, XM_TRIG_FALLING, 0, 0);
    EQ(n, push(c, 6, {{1, 1, 1}, {2, 0, 0}, {3, 1, 0}, {5, 1, 0}}), 0);
    EQ(n, c.st.triggers_seen, 4);
    EQ(n, c.st.triggers_selected, 2);
    EQ(n, c.st.events_before_first_trigger, 3);
    EQ(n, c.ready.size(), 1);
    frame(n, c, 0, 3, 5);
    EQ(n, c.ready[0].opening.id, 1);
    TrigCutter b = cutter(100, -1, XM_TRIG_BOTH, 0, 0);
    EQ(n, push(b, 6, {{1, 1, 1}, {2, 0, 0}, {3, 1, 0}, {5, 1, 0}}), 0);
    EQ(n, b.ready.size(), 3);
    frame(n, b, 0, 1, 2);
    frame(n, b, 1, 2, 3);
    frame(n, b, 2, 3, 5);
  }
  {  // F: the live part moves to the front; an open frame that overflows is dropped, the next one is intact
    const char* n = "F";
    TrigCutter c = cutter(10, -1, XM_TRIG_RISING, 0, 0);
    TrigRoom r;
    EQ(n, push(c, 6, {{4, 0, 1}}, &r), 0);
    EQ(n, r.dst, 0);
    EQ(n, r.move_n, 0);
    EQ(n, c.lo, 4);
    EQ(n, c.hi, 6);
    EQ(n, push(c, 5, {{3, 0, 1}}, &r), 0);
    EQ(n, r.move_from, 4);
    EQ(n, r.move_n, 2);
    EQ(n, r.dst, 2);
    frame(n, c, 0, 0, 5);
    EQ(n, c.hi, 7);
    c.release(1);
    EQ(n, c.lo, 5);
    EQ(n, push(c, 4, {}, &r), 0);
    EQ(n, r.move_from, 5);
    EQ(n, r.move_n, 2);
    EQ(n, r.dst, 2);
    EQ(n, c.hi, 6);
    EQ(n, c.st.front_moves, 2);
    EQ(n, push(c, 5, {}, &r), 0);  // 6 + 5 > 10: the open frame goes
    EQ(n, r.dst, 0);
    EQ(n, r.move_n, 0);
    EQ(n, c.open, 0);
    EQ(n, c.st.events_dropped_open_frame, 11);
    EQ(n, c.hi, 0);
    EQ(n, push(c, 3, {{1, 0, 1}}, &r), 0);
    EQ(n, c.st.events_dropped_open_frame, 12);
    EQ(n, c.open, 1);
    EQ(n, c.open_pos, 1);
    EQ(n, push(c, 2, {{2, 0, 1}}, &r), 0);
    EQ(n, r.dst, 3);
    EQ(n, c.ready.size(), 1);
    frame(n, c, 0, 1, 5);
    EQ(n, c.st.events_in, 25);
    EQ(n, c.st.frames_cut, 2);
    EQ(n, c.st.events_before_first_trigger, 4);
    EQ(n, c.st.front_moves, 2);
    EQ(n, c.stream_pos, 25);
  }
  {  // G: ready frames that are not released leave no room
    const char* n = "G";
    TrigCutter c = cutter(10, -1, XM_TRIG_RISING, 0, 0);
    EQ(n, push(c, 8, {{0, 0, 1}, {8, 0, 1}}), 0);
    frame(n, c, 0, 0, 8);
    EQ(n, push(c, 5, {}), -1);
    EQ(n, c.ready.size(), 1);
    c.release(1);
    EQ(n, push(c, 5, {{1, 0, 1}}), 0);  // (the open frame went with the refused push: these events up to the trigger are dropped)
    EQ(n, c.st.events_dropped_open_frame, 1);
    EQ(n, c.open_pos, 1);
  }
  {  // H: reset forgets the open frame and the stream position; the counters stay
    const char* n = "H";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 0, 0);
    EQ(n, push(c, 10, {{3, 0, 1}, {8, 0, 1}}), 0);
    c.reset();
    EQ(n, c.ready.size(), 0);
    EQ(n, c.open, 0);
    EQ(n, c.stream_pos, 0);
    EQ(n, push(c, 3, {}), 0);
    EQ(n, c.st.events_before_first_trigger, 6);
    EQ(n, c.hi, 0);
    EQ(n, c.st.frames_cut, 1);
  }
  {  // an event_index behind the chunk's kept count is the kept count
    const char* n = "clip";
    TrigCutter c = cutter(100, -1, XM_TRIG_RISING, 0, 0);
    EQ(n, push(c, 4, {{0, 0, 1}, {9, 0, 1}}), 0);
    frame(n, c, 0, 0, 4);
    EQ(n, c.open_pos, 4);
  }
  printf("ok\n");
  return 0;
}
