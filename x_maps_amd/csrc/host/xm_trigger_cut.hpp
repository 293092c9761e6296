// xm_trigger_cut.hpp -- the cut rule of the triggered frames (include/xmaps.h states it in full): which records of the buffer make
// frame k, what is skipped, dropped and counted, where the next chunk goes and when the live part moves to the front
// (part of libxmaps_hip.so's host side: included by xm_api_exttrigger.hpp; standard C++ only -- no HIP, no handle --, so that a CPU
// test can build it alone: tests/c_host/trigger_cut_host.cpp.  Needs include/xmaps.h in front of it.  Python mirror:
// x_maps_amd/ext_trigger.py, TriggerFrameCutter.)
//
// All positions are record offsets into the buffer of cfg.cap_events records.  [lo, hi) is its live part: the ready frames that
// have not been released, whatever lies between them (skipped frames) and the open frame.  A push is room() -- the caller does
// the move it asks for and writes the chunk's kept records at `dst` -- then append() with the chunk's kept count and its
// triggers, event_index already in kept records.
#pragma once

#include <cstddef>
#include <cstdint>
#include <deque>

namespace {

struct TrigFrame {
  uint64_t begin, end;  // records of the buffer
  xm_ext_trigger opening;
};

struct TrigRoom {
  int rc;               // 0, or -1: the ready frames alone leave no room for the chunk
  uint64_t move_from, move_n;  // move_n records at move_from go to offset 0 first (move_n = 0: nothing moves)
  uint64_t dst;         // where the chunk's kept records go
};

struct TrigCutter {
  xm_trigframes_config cfg{};
  xm_trigframes_counters st{};
  uint64_t stream_pos = 0;  // events kept since create / reset
  uint64_t lo = 0, hi = 0;
  bool open = false, dropping = false;
  uint64_t open_pos = 0;
  xm_ext_trigger open_trig{};
  std::deque<TrigFrame> ready;

  bool selected(const xm_ext_trigger& t) const {
    if (cfg.id >= 0 && (int)t.id != cfg.id) return false;
    return cfg.edge == XM_TRIG_BOTH || (cfg.edge == XM_TRIG_RISING ? t.value == 1 : t.value == 0);
  }

  void reset() {
    stream_pos = lo = hi = open_pos = 0;
    open = dropping = false;
    ready.clear();
  }

  // room for a chunk of n_in decoded events behind the live part
  TrigRoom room(uint64_t n_in) {
    TrigRoom r{0, 0, 0, hi};
    if (hi + n_in <= cfg.cap_events) return r;
    if (hi - lo + n_in > cfg.cap_events && open) {  // the open frame cannot keep its events plus this chunk: dropped
      st.events_dropped_open_frame += hi - open_pos;
      hi = open_pos;
      open = false;
      dropping = true;
      trim();
    }
    if (hi - lo + n_in > cfg.cap_events) return r.rc = -1, r;
    if (hi + n_in > cfg.cap_events) {  // fits only at the front
      r.move_from = lo, r.move_n = hi - lo;
      for (TrigFrame& f : ready) f.begin -= lo, f.end -= lo;
      open_pos -= open ? lo : 0;
      hi -= lo, lo = 0;
      st.front_moves += 1;
    }
    r.dst = hi;
    return r;
  }

  // the chunk's n_in decoded events left n_kept records at room().dst; trig[0 .. n_trig): its triggers in word order, event_index
  // in kept records (<= n_kept)
  void append(uint64_t n_in, uint64_t n_kept, const xm_ext_trigger* trig, size_t n_trig) {
    const uint64_t base = hi;
    uint64_t cursor = 0;
    st.events_in += n_in, st.events_kept += n_kept;
    for (size_t j = 0; j < n_trig; ++j) {
      st.triggers_seen += 1;
      if (!selected(trig[j])) continue;
      st.triggers_selected += 1;
      const uint64_t idx = trig[j].event_index < n_kept ? trig[j].event_index : n_kept;
      close_segment(cursor, idx, base);
      open = true, dropping = false;
      open_pos = base + idx;
      open_trig = trig[j];
      cursor = idx;
    }
    if (!open) (dropping ? st.events_dropped_open_frame : st.events_before_first_trigger) += n_kept - cursor;
    hi = base + n_kept;
    stream_pos += n_kept;
    trim();
  }

  // the next run of ready frames that lie back to back, at most cap_frames (and cfg.max_frames_ready, if > 0)
  int run(int cap_frames) const {
    int lim = cap_frames;
    if (cfg.max_frames_ready > 0 && cfg.max_frames_ready < lim) lim = cfg.max_frames_ready;
    int n = 0;
    while (n < lim && (size_t)n < ready.size() && (n == 0 || ready[n].begin == ready[n - 1].end)) n += 1;
    return n;
  }

  void release(int n) {
    while (n-- > 0 && !ready.empty()) ready.pop_front();
    trim();
  }

 private:
  void close_segment(uint64_t cursor, uint64_t idx, uint64_t base) {
    if (!open) {
      (dropping ? st.events_dropped_open_frame : st.events_before_first_trigger) += idx - cursor;
      return;
    }
    const uint64_t end = base + idx, n = end - open_pos;
    if (cfg.min_events > 0 && n <= cfg.min_events) st.frames_skipped += 1;
    else ready.push_back(TrigFrame{open_pos, end, open_trig}), st.frames_cut += 1;
  }

  // records in front of the first frame that is still needed and behind the last one are not live
  void trim() {
    if (!open) hi = ready.empty() ? 0 : ready.back().end;
    lo = !ready.empty() ? ready.front().begin : open ? open_pos : 0;
    if (ready.empty() && !open) lo = hi = 0;
  }
};

}  // namespace
