// slot_order_host.cpp -- a slot's ordering record (x_maps_amd/csrc/host/xm_slot_order.hpp) against the runtime calls the call sites
// made by hand before the record had an owner.  The ops type appends every call to a trace; each case states the EXACT trace, read
// off the former code of the site named beside it (enqueue_frame, enqueue_batch, xm_graph_launch, xm_last_frame_stats, xm_sync), not
// off the header.  Stand-alone (its own main, no HIP, no GPU): tests/test_slot_order_cpu.py builds it with
// -fsanitize=address,undefined and runs it.  Prints "ok", or what differs and exits 1.
#include "../../x_maps_amd/csrc/host/xm_slot_order.hpp"

#include <cstdio>
#include <string>
#include <vector>

namespace {

// streams and events are addresses of these names
const char A[] = "A", B[] = "B", C[] = "C", O[] = "O", S0[] = "S0", S1[] = "S1";
const char G[] = "G", G2[] = "G2", J[] = "J", J0[] = "J0", J1[] = "J1", J2[] = "J2", J3[] = "J3";
void* h(const char* name) { return const_cast<char*>(name); }
std::string n(void* p) { return static_cast<const char*>(p); }

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
};
std::vector<std::string> TraceOps::trace;
int TraceOps::fail_at = -1;

using Order = SlotOrder<TraceOps>;

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

Order slot_on(const char* own, const char* join) {
  Order o;
  o.bind(h(own), h(join));
  return o;
}

}  // namespace

int main() {
  {  // 1. a group on A, then a frame on the slot's own stream B (enqueue_frame: the event's stream is not the frame's)
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    expect_rc("1", o.before_group_only(h(B)), 0);
    expect("1 group on A, frame on B", "wait(B,G)");
    o.before_group_only(h(B));  // 11. the record was forgotten
    expect("1 again", "");
  }
  {  // 2. the same with B == A: the stream orders itself; the record is dropped all the same
    Order o = slot_on(B, J);
    o.note_group(h(G), h(B));
    o.before_group_only(h(B));
    expect("2 group on B, frame on B", "");
    o.before_group_only(h(A));
    expect("2 the record is gone", "");
  }
  {  // 3. eager work on B, then a group on A (enqueue_batch: join event recorded on the own stream, the group's stream waits)
    Order o = slot_on(B, J);
    o.note_eager();
    o.before(h(A), false);
    expect("3 eager on B, group on A", "record(J,B) wait(A,J)");
    o.before(h(A), false);
    expect("3 again", "");
  }
  {  // 4. eager on B, then a group on B: nothing, and the mark is cleared (a later group on A finds nothing to wait for)
    Order o = slot_on(B, J);
    o.note_eager();
    o.before(h(B), false);
    expect("4 eager on B, group on B", "");
    o.before(h(A), false);
    expect("4 the mark is gone", "");
  }
  {  // 5. both records: the group event first, then the join (enqueue_batch's order within one slot)
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    o.note_eager();
    o.before(h(C), false);
    expect("5 group on A + eager on B, group on C", "wait(C,G) record(J,B) wait(C,J)");
    o.before(h(C), false);
    expect("5 again", "");
    o.note_group(h(G), h(A));
    o.note_eager();
    o.before(h(A), false);  // (the next group on the last group's stream: only the eager work is elsewhere)
    expect("5 group on A + eager on B, group on A", "record(J,B) wait(A,J)");
  }
  {  // 6. the group-only variant leaves the eager mark alone (enqueue_frame never looked at it): a later group still joins
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    o.note_eager();
    o.before_group_only(h(C));
    expect("6 group-only on C", "wait(C,G)");
    o.before(h(C), false);
    expect("6 the eager mark stayed", "record(J,B) wait(C,J)");
  }
  {  // 7. capturing (enqueue_batch inside xm_graph_create): no call, the group record is cleared, the eager mark is kept
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    o.note_eager();
    o.before(h(C), true);
    expect("7 capturing", "");
    o.before(h(C), false);
    expect("7 afterwards: no group event, the join", "record(J,B) wait(C,J)");
  }
  {  // 8. the set form (xm_graph_launch): four slots on two streams, one dirty slot on each -- one join per STREAM, by stream in
     // the order of the streams' first slots and with the first slot's join event, then the group events slot by slot
    std::vector<Order> s;
    s.push_back(slot_on(S0, J0));
    s.push_back(slot_on(S1, J1));
    s.push_back(slot_on(S0, J2));
    s.push_back(slot_on(S1, J3));
    const auto self = [](Order& o) -> Order& { return o; };
    s[2].note_eager();
    s[1].note_eager();
    expect_rc("8", Order::before_all(s.begin(), s.end(), self, h(O)), 0);
    expect("8 one dirty slot per stream", "record(J0,S0) wait(O,J0) record(J1,S1) wait(O,J1)");
    Order::before_all(s.begin(), s.end(), self, h(O));
    expect("8 nothing dirty", "");
    s[2].before(h(A), false);
    expect("8 every mark was cleared", "");
    // two dirty slots on ONE stream, group events on two slots (one recorded on the replay's own stream)
    s[0].note_eager();
    s[2].note_eager();
    s[0].note_group(h(G), h(A));
    s[3].note_group(h(G2), h(O));
    Order::before_all(s.begin(), s.end(), self, h(O));
    expect("8 two dirty slots on one stream + group events", "record(J0,S0) wait(O,J0) wait(O,G)");
    Order::before_all(s.begin(), s.end(), self, h(O));
    expect("8 again", "");
    s[3].before_group_only(h(S1));
    expect("8 the replay stream's own event was dropped too", "");
  }
  {  // 9. the host waits for the slot's last frame (xm_last_frame_stats): the event if there is one, then the own stream
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    expect_rc("9", o.host_wait(), 0);
    expect("9 host wait behind a group", "sync_event(G) sync_stream(B)");
    o.host_wait();
    expect("9 host wait without a group event", "sync_stream(B)");
    o.note_eager();
    o.host_wait();  // (the eager mark is not the host wait's: xm_last_frame_stats never cleared it)
    o.before(h(A), false);
    expect("9 host wait leaves the eager mark", "sync_stream(B) record(J,B) wait(A,J)");
  }
  {  // 10. forget (xm_sync, xm_graph_create: every stream is idle)
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    o.note_eager();
    o.forget();
    o.before(h(C), false);
    expect("10 forget", "");
    o.host_wait();
    expect("10 forget: host wait", "sync_stream(B)");
  }
  {  // a failing call is returned at once and nothing is forgotten (HIP_TRY returned in front of the assignment)
    Order o = slot_on(B, J);
    o.note_group(h(G), h(A));
    o.note_eager();
    TraceOps::fail_at = 0;
    expect_rc("failing wait", o.before(h(C), false), 7);
    expect("failing wait", "");
    TraceOps::fail_at = 2;
    expect_rc("failing join wait", o.before(h(C), false), 7);
    expect("failing join wait", "wait(C,G) record(J,B)");
    TraceOps::fail_at = -1;
    expect_rc("no failure", o.before(h(C), false), 0);
    expect("the eager mark survived the failure, the group event was done with", "record(J,B) wait(C,J)");
  }
  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}
