// scratch_order_host.cpp -- the ordering record of a handle's per-entry scratch (x_maps_amd/csrc/host/xm_scratch_order.hpp) against
// the runtime calls its five call sites made by hand before the record had an owner, and the ingest rings' entry / tag arithmetic
// (x_maps_amd/csrc/host/xm_ring_tag.hpp) against literals.  The ops type appends every call to a trace -- with "reserve" for the
// site's reserve_all, "create" for the event's creation and "zero" for the site's memsets --; each case states the EXACT trace, read
// off the former code of the site named beside it (xm_process_time_surfaces, xm_frames_to_time_surfaces, xm_frames_to_point_clouds,
// xm_surface_set_cloud_tables, xm_cloud_set_tables), not off the header.  Stand-alone (its own main, no HIP, no GPU):
// tests/test_scratch_order_cpu.py builds it with -fsanitize=address,undefined and runs it.  Prints "ok", or what differs and exits 1.
#include "../../x_maps_amd/csrc/host/xm_ring_tag.hpp"
#include "../../x_maps_amd/csrc/host/xm_scratch_order.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace {

// streams and the event are addresses of these names
const char A[] = "A", B[] = "B", D[] = "D";
void* h(const char* name) { return const_cast<char*>(name); }
std::string n(void* p) { return static_cast<const char*>(p); }

struct TraceEvent {  // the event "D", once made
  bool made = false;
  void* get() const;
};

struct TraceOps {
  static std::vector<std::string> trace;
  static int fail_at;  // the call with this index (from 0) returns 7 instead of running
  static int call(const std::string& text) {
    if ((int)trace.size() == fail_at) return 7;
    trace.push_back(text);
    return 0;
  }
  static int record(void* ev, void* stream) { return call("record(" + n(ev) + "," + n(stream) + ")"); }
  static int wait(void* stream, void* ev) { return call("wait(" + n(stream) + "," + n(ev) + ")"); }
  static int sync_event(void* ev) { return call("sync_event(" + n(ev) + ")"); }
  static int sync_stream(void* stream) { return call("sync_stream(" + n(stream) + ")"); }
  static int create(TraceEvent& e) {
    if (int rc = call("create")) return rc;
    e.made = true;
    return 0;
  }
};
void* TraceEvent::get() const { return made ? h(D) : nullptr; }
std::vector<std::string> TraceOps::trace;
int TraceOps::fail_at = -1;

using Order = ScratchOrder<TraceOps, TraceEvent>;

int g_failed = 0;
// the calls since the last look are exactly `want` (separated by one blank)
void expect(const char* what, const std::string& want) {
  std::string got;
  for (const std::string& c : TraceOps::trace) got += (got.empty() ? "" : " ") + c;
  TraceOps::trace.clear();
  if (got != want) {
    fprintf(stderr, "FAILED %s:\n  want [%s]\n  got  [%s]\n", what, want.c_str(), got.c_str());
    g_failed += 1;
  }
}
void expect_rc(const char* what, int rc, int want) {
  if (rc != want) {
    fprintf(stderr, "FAILED %s: rc %d, want %d\n", what, rc, want);
    g_failed += 1;
  }
}
template <class T>
void expect_eq(const char* what, T got, T want) {
  if (got != want) {
    fprintf(stderr, "FAILED %s: got %llu, want %llu\n", what, (unsigned long long)got, (unsigned long long)want);
    g_failed += 1;
  }
}

// a call of an entry as far as the record sees it: the site's reserve_all and its memsets are "reserve" and "zero"
int enter(Order& o, const char* stream, bool grows, bool zero_lost) {
  return o.enter(h(stream), grows, zero_lost, [] { return TraceOps::call("reserve"); }, [] { return TraceOps::call("zero"); });
}
// ... a whole call on device pointers that succeeds
void device_call(Order& o, const char* stream, bool grows, bool zero_lost) {
  enter(o, stream, grows, zero_lost);
  o.launching();
  o.launched();
  o.leave_async(h(stream));
}

}  // namespace

int main() {
  {  // 1. the first call (xm_frames_to_time_surfaces: maps and accumulators are new, so they grow and are not zero yet; nothing is in
     //    flight: no synchronise; reserve_all, the event is made, no wait, the memsets; the event is recorded behind the launches)
    Order o;
    expect_rc("1", enter(o, A, true, true), 0);
    expect("1 first call", "reserve create zero");
    o.launching();
    o.launched();
    expect_rc("1 leave", o.leave_async(h(A)), 0);
    expect("1 first call leaves", "record(D,A)");
    // 2. the same stream again, nothing grows: reserve_all (which finds nothing to do), no event, no wait, no memset
    expect_rc("2", enter(o, A, false, false), 0);
    expect("2 same stream again", "reserve");
    o.launching();
    o.launched();
    o.leave_async(h(A));
    expect("2 leaves", "record(D,A)");
    // 3. the next call runs on another slot's stream: it waits for the event
    expect_rc("3", enter(o, B, false, false), 0);
    expect("3 other stream", "reserve wait(B,D)");
    o.leave_async(h(B));
    expect("3 leaves", "record(D,B)");
    // 4. growth while that call may be in flight (on B): the host waits for B, the stream is forgotten, so no wait follows; the
    //    new maps are cleared
    expect_rc("4", enter(o, A, true, true), 0);
    expect("4 growth while in flight", "sync_stream(B) reserve zero");
    o.leave_async(h(A));
    expect("4 leaves", "record(D,A)");
    // ... the same in xm_process_time_surfaces, which has no zero invariant: no memset
    expect_rc("4s", enter(o, B, true, false), 0);
    expect("4s growth while in flight, no zero invariant", "sync_stream(A) reserve");
    o.leave_async(h(B));
    expect("4s leaves", "record(D,B)");
    // 5. a call on host pointers: it waits like any other, synchronises its stream itself and forgets it -- the next call on
    //    another stream has nothing to wait for
    expect_rc("5", enter(o, A, false, false), 0);
    expect("5 synchronous call enters", "reserve wait(A,D)");
    o.launching();
    o.launched();
    o.leave_sync();
    expect("5 synchronous leave", "");
    expect_rc("5 next", enter(o, B, false, false), 0);
    expect("5 nothing in flight behind a synchronous call", "reserve");
    o.leave_async(h(B));
    expect("5 leaves", "record(D,B)");
    // 6. the tables are rewritten while a call may be in flight (xm_surface_set_cloud_tables, xm_cloud_set_tables): the host
    //    waits for its stream and forgets it; a second rewrite and the next call find nothing in flight
    expect_rc("6", o.settle(), 0);
    expect("6 table rewrite while in flight", "sync_stream(B)");
    expect_rc("6 again", o.settle(), 0);
    expect("6 second rewrite", "");
    expect_rc("6 next", enter(o, A, false, false), 0);
    expect("6 call behind a rewrite", "reserve");
  }
  {  // 6b. a rewrite before any call: nothing
    Order o;
    expect_rc("6b", o.settle(), 0);
    expect("6b rewrite before any call", "");
  }
  {  // 7. the dirty note survives what fails behind it.  A call in flight on A; the next one grows its maps (noted before anything
     //    else) and its hipStreamSynchronize fails: HIP_TRY returned in front of `last_stream = nullptr`, the note was set
    Order o;
    device_call(o, A, true, true);
    expect("7 setup", "reserve create zero record(D,A)");
    TraceOps::fail_at = 0;
    expect_rc("7 failing synchronise", enter(o, B, true, true), 7);
    expect("7 failing synchronise", "");
    TraceOps::fail_at = -1;
    // the next call, nothing grows any more: A is still in flight for it, and it clears the scratch
    expect_rc("7 next", enter(o, B, false, false), 0);
    expect("7 the note and the stream survived", "reserve wait(B,D) zero");
    // a failing memset leaves the note too
    o.launching();  // (a call that returns between its first and its last launch)
    o.leave_sync();
    TraceOps::fail_at = 1;
    expect_rc("7 failing memset", enter(o, B, false, false), 7);
    expect("7 failing memset", "reserve");
    TraceOps::fail_at = -1;
    expect_rc("7 behind it", enter(o, B, false, false), 0);
    expect("7 cleared behind a failed launch sequence and a failed memset", "reserve zero");
    o.launching();
    o.launched();
    expect_rc("7 clean", enter(o, B, false, false), 0);
    expect("7 a call that issued all its launches leaves no note", "reserve");
    // a failing reserve_all is returned before the event is made or waited for
    Order p;
    TraceOps::fail_at = 0;
    expect_rc("7 failing reserve", enter(p, A, true, true), 7);
    expect("7 failing reserve", "");
    TraceOps::fail_at = -1;
    expect_rc("7 behind a failing reserve", enter(p, A, false, false), 0);
    expect("7 the event is made by the first call that gets there; the note stayed", "reserve create zero");
  }

  // ---- the ingest rings: entry and tag (xm_ring_tag.hpp) ----
  expect_eq<size_t>("entry 0 of 4", ring_entry(0, 4), 0);
  expect_eq<size_t>("entry 5 of 4", ring_entry(5, 4), 1);
  expect_eq<size_t>("entry 7 of 2", ring_entry(7, 2), 1);
  expect_eq<size_t>("entry 65537 of 65536", ring_entry(65537, 65536), 1);
  expect_eq<size_t>("entry 2^64 - 1 of 3", ring_entry(0xffffffffffffffffull, 3), 0);
  expect_eq<size_t>("entry of a ring of one", ring_entry(123456789, 1), 0);
  // a surface's tag: (frame + 1) << 2 | dtype (XM_T_FLOAT32 = 1, XM_T_FLOAT64 = 2)
  expect_eq<uint64_t>("surface tag 0 f32", surface_tag(0, 1), 5);
  expect_eq<uint64_t>("surface tag 0 f64", surface_tag(0, 2), 6);
  expect_eq<uint64_t>("surface tag 9 f64", surface_tag(9, 2), 42);
  expect_eq<int>("dtype of 42", surface_tag_dtype(42), 2);
  expect_eq<int>("dtype of 5", surface_tag_dtype(5), 1);
  expect_eq<bool>("42 names 9", surface_tag_names(42, 9), true);
  expect_eq<bool>("42 does not name 10", surface_tag_names(42, 10), false);
  expect_eq<bool>("a cleared tag names nothing", surface_tag_names(0, 0), false);
  // a cloud's tag: frame + 1
  expect_eq<uint64_t>("cloud tag 0", cloud_tag(0), 1);
  expect_eq<uint64_t>("cloud tag 9", cloud_tag(9), 10);
  expect_eq<bool>("10 names 9", cloud_tag_names(10, 9), true);
  expect_eq<bool>("10 does not name 10", cloud_tag_names(10, 10), false);
  expect_eq<bool>("a cleared cloud tag names nothing", cloud_tag_names(0, 0), false);
  // a lapped entry: ring of 2, frame 5 has taken entry 1 from frame 3
  expect_eq<size_t>("3 and 5 share an entry", ring_entry(3, 2), ring_entry(5, 2));
  expect_eq<bool>("frame 5's surface tag does not name 3", surface_tag_names(surface_tag(5, 1), 3), false);
  expect_eq<bool>("... it names 5", surface_tag_names(surface_tag(5, 1), 5), true);
  expect_eq<bool>("frame 5's cloud tag does not name 3", cloud_tag_names(cloud_tag(5), 3), false);
  expect_eq<bool>("... it names 5", cloud_tag_names(cloud_tag(5), 5), true);
  // seq + 1 = 2^62 does not fit the 62 bits above the dtype: the shift drops it, the tag is the bare dtype and names no frame
  // (today's arithmetic, stated; 2^62 frames are out of reach); the frame before is the last whose tag is whole
  const uint64_t top = (1ull << 62) - 1;
  expect_eq<uint64_t>("surface tag 2^62 - 1", surface_tag(top, 2), 2);
  expect_eq<bool>("... names nothing", surface_tag_names(surface_tag(top, 2), top), false);
  expect_eq<int>("... keeps the dtype", surface_tag_dtype(surface_tag(top, 2)), 2);
  expect_eq<uint64_t>("surface tag 2^62 - 2", surface_tag(top - 1, 1), 0xfffffffffffffffdull);
  expect_eq<bool>("... names its frame", surface_tag_names(surface_tag(top - 1, 1), top - 1), true);
  expect_eq<uint64_t>("cloud tag 2^62 - 1", cloud_tag(top), 1ull << 62);
  expect_eq<bool>("... names its frame", cloud_tag_names(cloud_tag(top), top), true);

  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}
