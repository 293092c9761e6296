// xm_scratch_order.hpp -- how the calls on a handle's per-entry scratch follow each other, and the only code that orders them (ScratchOrder)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; standard C++ only, so that a CPU
// test can build it alone: tests/c_host/scratch_order_host.cpp)
//
// xm_process_time_surfaces, xm_frames_to_time_surfaces and xm_frames_to_point_clouds each keep ONE set of tables and grow-only
// scratch per handle, while consecutive calls run on the streams of different slots and a call on device pointers returns with its
// launches in flight.  THE PROTOCOL: a call's launches wait for the previous call's before they touch the scratch; the host waits
// for the previous call before a buffer or a table is replaced; scratch that must be all zero between calls is cleared again when
// it is new or when a call failed between its first and its last launch.  The record below remembers what that takes -- the
// end-of-call event, the stream it was recorded on, the dirty note -- and nothing else reads or writes it:
//
//   settle()                         the host waits for the call in flight, if any (tables or buffers are about to change)
//   enter(X, grows, zero_lost, reserve, zero)
//                                    a call on stream X.  zero_lost: scratch under the zero invariant is about to be replaced --
//                                    noted dirty first, so that a call that fails below leaves the note.  grows: some buffer is
//                                    about to be replaced: settle().  Then reserve() makes the buffers, the event is made by the
//                                    first call, X waits for the event if the call in flight runs on another stream, and zero()
//                                    clears the scratch if it is noted dirty (on X, behind that wait)
//   launching() / launched()         around the call's launches: a call that returns between them leaves the scratch noted dirty
//   leave_async(X)                   the call returns with its work in flight on X: the event is recorded behind it
//   leave_sync()                     the call has synchronised X itself: nothing is in flight
//
// Only these forget the stream of the call in flight; xm_sync does not, so a call behind it may issue a wait that has nothing
// left to wait for.  Streams are opaque pointers; the calls come from xm_slot_order.hpp's Ops (static int record(ev, stream) /
// wait(stream, ev) / sync_event(ev) / sync_stream(stream), and here create(Ev&); 0 = success, anything else -- also from reserve()
// and zero() -- is returned to the caller at once).  Ev owns the event: get() is NULL until Ops::create has made it.
#pragma once

namespace {

template <class Ops, class Ev>
class ScratchOrder {
 public:
  int settle() {
    if (int rc = last_ ? Ops::sync_stream(last_) : 0) return rc;
    last_ = nullptr;
    return 0;
  }

  template <class Reserve, class Zero>
  int enter(void* stream, bool grows, bool zero_lost, Reserve&& reserve, Zero&& zero) {
    if (zero_lost) dirty_ = true;
    if (int rc = grows ? settle() : 0) return rc;
    if (int rc = reserve()) return rc;
    if (int rc = done_.get() ? 0 : Ops::create(done_)) return rc;
    if (int rc = last_ && last_ != stream ? Ops::wait(stream, done_.get()) : 0) return rc;
    if (int rc = dirty_ ? zero() : 0) return rc;
    dirty_ = false;
    return 0;
  }

  void launching() { dirty_ = true; }
  void launched() { dirty_ = false; }

  int leave_async(void* stream) {
    if (int rc = Ops::record(done_.get(), stream)) return rc;
    last_ = stream;
    return 0;
  }
  void leave_sync() { last_ = nullptr; }

 private:
  Ev done_;               // recorded behind a call that returns with its work in flight
  void* last_ = nullptr;  // view: the stream of that call (nullptr: none in flight since a settle() or a synchronous call)
  bool dirty_ = false;    // scratch under the zero invariant is not known to be zero
};

}  // namespace
