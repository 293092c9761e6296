// xm_agree.hpp -- the agreement among the device threads of a sharded handle: a host barrier that hands every thread the first
// error any of them brought, and that a thread leaving the frame elsewhere poisons (Agreement)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; standard C++ only, so that a CPU
// test can build it alone: tests/c_host/agree_stress.cpp)
#pragma once

#include <condition_variable>
#include <mutex>

namespace {

// agree(rc) returns the first non-zero rc any of the `world` threads brought to the round (0: everybody is fine), to all of them.
// A thread that leaves the frame with an error anywhere else -- hipSetDevice at the top, a collective that returned an error
// right behind an agreement, the copy at the end of a virtual all-reduce -- will never arrive at the next agreement: it POISONS
// the barrier on its way out (leave), which wakes everybody waiting in agree and makes every later arrival of the frame return
// at once with that error (its own non-zero rc first).  reset(), called while the threads are idle, starts the next frame clean
// whatever the last one left.  A world of one agrees with itself.
class Agreement {
 public:
  explicit Agreement(int world) : world_(world) {}
  int agree(int rc) {
    if (world_ == 1) return rc;
    std::unique_lock<std::mutex> lk(mu_);
    if (poison_) return rc ? rc : poison_;
    if (rc && !rc_) rc_ = rc;
    const unsigned long long gen = gen_;
    if (++arrived_ == world_) {
      rc_out_ = rc_;
      rc_ = 0;
      arrived_ = 0;
      gen_ += 1;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen || poison_ != 0; });
      if (gen_ == gen) return rc ? rc : poison_;  // (poisoned while waiting: the round never completes)
    }
    return rc_out_;
  }
  // a thread leaves the frame with rc (once per thread and frame, wherever it returned from)
  void leave(int rc) {
    if (!rc || world_ == 1) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (!poison_) poison_ = rc;
    }
    cv_.notify_all();
  }
  void reset() {
    std::lock_guard<std::mutex> lk(mu_);
    arrived_ = 0;
    rc_ = 0;
    poison_ = 0;
  }

 private:
  const int world_;
  std::mutex mu_;
  std::condition_variable cv_;
  int arrived_ = 0, rc_ = 0, rc_out_ = 0;
  unsigned long long gen_ = 0;
  int poison_ = 0;  // != 0: a thread has LEFT the frame with this error outside an agreement point -- nobody waits for it any more
};

}  // namespace
