// xm_slot_order.hpp -- where a slot's last work ran, and the only code that orders a stream or the host behind it (SlotOrder)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; standard C++ only, so that a CPU
// test can build it alone: tests/c_host/slot_order_host.cpp)
//
// A slot's buffers (key frame, state, staging) are used from three kinds of stream: its OWN stream (eager frames, time surfaces),
// the stream a GROUP of frames was launched on (any of the distinct slot streams, in rotation) and the origin stream of a graph
// replay.  THE PROTOCOL: before a slot's buffers are used on stream X, X waits for whatever the slot did last on another stream.
// The record below remembers what that was -- the end-of-group / end-of-replay event and the stream it was recorded on, and whether
// eager work went to the own stream since the last synchronisation point -- and nothing else reads or writes it:
//
//   note_group(done, stream)   a group or a graph replay ran the slot's frame; `done` was recorded behind it on `stream`
//   note_eager()               work was enqueued on the slot's own stream
//   before_group_only(X)       X waits for the group event if that was recorded on another stream; the eager mark stays (a lone
//                              frame: X is the own stream, or a group's stream that enqueue_batch has just ordered)
//   before(X, capturing)       ... and, if eager work is outstanding on the own stream and that is not X, the slot's join event is
//                              recorded there and X waits for it (a group).  capturing: no runtime call -- a capture must not wait
//                              for events outside it --, the group record is dropped all the same, the eager mark is kept
//   before_all(slots, X)       the same for a whole set of slots with ONE join event per distinct dirty stream, not one per slot
//                              (a graph replay: a handle that only replays graphs pays no call here at all)
//   host_wait()                the host blocks until the slot's last work is done: the group event, then the own stream
//   forget()                   every stream is idle
//
// Whatever was ordered is forgotten: the same call again issues nothing.  Streams and events are opaque pointers; the calls
// come from Ops (static int record(ev, stream) / wait(stream, ev) / sync_event(ev) / sync_stream(stream), 0 = success, anything
// else is returned to the caller at once with the record as it stood before the failing call).
#pragma once

namespace {

template <class Ops>
class SlotOrder {
 public:
  void bind(void* own_stream, void* join_ev) { own_ = own_stream, join_ = join_ev; }
  void note_group(void* done, void* stream) { group_ev_ = done, group_stream_ = stream; }
  void note_eager() { eager_ = true; }
  void forget() { group_ev_ = nullptr, eager_ = false; }

  int before_group_only(void* stream, bool capturing = false) {
    if (!group_ev_) return 0;
    if (group_stream_ != stream && !capturing)
      if (int rc = Ops::wait(stream, group_ev_)) return rc;
    group_ev_ = nullptr;
    return 0;
  }

  int before(void* stream, bool capturing) {
    if (int rc = before_group_only(stream, capturing)) return rc;
    if (!eager_ || capturing) return 0;
    if (own_ != stream)
      if (int rc = join(stream)) return rc;
    eager_ = false;
    return 0;
  }

  // rec(*it) is the SlotOrder of an element of [first, last).  The joins come first, by stream in the order of the streams' first
  // slots, each with its first slot's join event; then the group events, slot by slot.
  template <class It, class Rec>
  static int before_all(It first, It last, Rec rec, void* stream) {
    bool dirty = false;
    for (It i = first; i != last; ++i) dirty = dirty || rec(*i).eager_;
    for (It i = first; dirty && i != last; ++i) {
      SlotOrder& lead = rec(*i);
      bool is_first = true, any = false;
      for (It j = first; j != i; ++j) is_first = is_first && rec(*j).own_ != lead.own_;
      for (It j = i; is_first && j != last; ++j) any = any || (rec(*j).own_ == lead.own_ && rec(*j).eager_);
      if (any)
        if (int rc = lead.join(stream)) return rc;
    }
    for (It i = first; i != last; ++i) {
      rec(*i).eager_ = false;
      if (int rc = rec(*i).before_group_only(stream)) return rc;
    }
    return 0;
  }

  int host_wait() {
    if (group_ev_) {
      if (int rc = Ops::sync_event(group_ev_)) return rc;
      group_ev_ = nullptr;
    }
    return Ops::sync_stream(own_);
  }

 private:
  int join(void* stream) {
    if (int rc = Ops::record(join_, own_)) return rc;
    return Ops::wait(stream, join_);
  }
  void* own_ = nullptr;           // view: the slot's own stream
  void* join_ = nullptr;          // view: the slot's join event (xm_handle::join_ev)
  void* group_ev_ = nullptr;      // view: the slot's last frame ran inside a group / a replay; this event (xm_handle::batch_ev /
  void* group_stream_ = nullptr;  // graph_ev) was recorded behind it on this stream
  bool eager_ = false;            // eager work was enqueued on the own stream since the last synchronisation point
};

}  // namespace
