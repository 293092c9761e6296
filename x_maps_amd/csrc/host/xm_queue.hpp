// xm_queue.hpp -- the host threads' hand-over: the first error of a thread (FirstError), the spin-then-sleep wait of a consumer
// and its wake-up (Doorbell), a single-producer single-consumer job queue built on them (JobQueue)
// (part of libxmaps_hip.so's host side: included by ../xmaps_hip.hip, one translation unit; standard C++ only, so that a CPU
// test can build it alone: tests/c_host/queue_stress.cpp)
#pragma once

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>

namespace {

// The first failing return code of a thread's work and its text, for the caller that reports it.  The hot loops only look at
// code(); the mutex is taken on the error path only.
class FirstError {
 public:
  void note(int rc, const std::string& text) {
    if (rc == 0 || code_.load(std::memory_order_relaxed) != 0) return;
    std::lock_guard<std::mutex> lk(mu_);
    if (code_.load(std::memory_order_relaxed) != 0) return;
    text_ = text;
    code_.store(rc, std::memory_order_release);
  }
  int code(std::memory_order mo = std::memory_order_acquire) const { return code_.load(mo); }
  // the code (0: none) and its text, then cleared: a later error is kept again
  int take(std::string* text) {
    if (code_.load(std::memory_order_acquire) == 0) return 0;
    std::lock_guard<std::mutex> lk(mu_);
    const int rc = code_.load(std::memory_order_relaxed);
    *text = text_;
    code_.store(0, std::memory_order_release);
    return rc;
  }
  // the same, kept (an error that stays)
  int peek(std::string* text) const {
    if (code_.load(std::memory_order_acquire) == 0) return 0;
    std::lock_guard<std::mutex> lk(mu_);
    *text = text_;
    return code_.load(std::memory_order_relaxed);
  }

 private:
  std::atomic<int> code_{0};
  mutable std::mutex mu_;
  std::string text_;
};

// One consumer waits for ready(): it spins, then sleeps; the producer makes ready() true with a seq_cst store, then calls ring().
// The consumer stores `sleeping` (seq_cst) under the mutex before it looks at ready() again, so one of the two sees the other's
// store: no wake-up is lost, and a producer whose consumer is awake pays one load.
class Doorbell {
 public:
  // idle(i) runs on every empty spin i and answers whether the consumer may sleep (after `spins` pauses at the earliest)
  template <typename Ready, typename Idle>
  void wait(const Ready& ready, unsigned spins, const Idle& idle) {
    if (ready()) return;
    for (unsigned long long i = 0;; ++i) {
      if (idle(i) && i >= spins) break;
      __builtin_ia32_pause();
      if (ready()) return;
    }
    std::unique_lock<std::mutex> lk(mu_);
    sleeping_.store(true, std::memory_order_seq_cst);
    cv_.wait(lk, ready);
    sleeping_.store(false, std::memory_order_relaxed);
  }
  template <typename Ready>
  void wait(const Ready& ready, unsigned spins) {
    wait(ready, spins, [](unsigned long long) { return true; });
  }
  void ring() {
    if (sleeping_.load(std::memory_order_seq_cst)) {
      std::lock_guard<std::mutex> lk(mu_);
      cv_.notify_one();
    }
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic<bool> sleeping_{false};
};

// Jobs from one producer thread to one consumer thread, in order.  Jobs are numbered from 1: post() returns the job's number,
// wait_done(n) waits until the consumer has finished job n.
template <typename Job, unsigned CAP>
class JobQueue {
 public:
  unsigned long long post(const Job& j) {
    const unsigned long long hd = head_.load(std::memory_order_relaxed);
    while (hd - tail_.load(std::memory_order_acquire) >= CAP) __builtin_ia32_pause();  // full: back-pressure
    ring_[hd % CAP] = j;
    head_.store(hd + 1, std::memory_order_seq_cst);
    bell_.ring();
    return hd + 1;
  }
  // jobs posted so far
  unsigned long long posted() const { return head_.load(std::memory_order_acquire); }

  // the consumer: the next job (Doorbell::wait: spins, idle)
  template <typename Idle>
  Job take(unsigned spins, const Idle& idle) {
    const unsigned long long t = tail_.load(std::memory_order_relaxed);
    bell_.wait([&] { return head_.load(std::memory_order_acquire) != t; }, spins, idle);
    const Job j = ring_[t % CAP];
    tail_.store(t + 1, std::memory_order_release);
    return j;
  }
  Job take(unsigned spins) {
    return take(spins, [](unsigned long long) { return true; });
  }
  // the job posted behind the one taken last, NULL if there is none yet; its entry is not reused before the next take()
  const Job* next() const {
    const unsigned long long t = tail_.load(std::memory_order_relaxed);
    return head_.load(std::memory_order_acquire) > t ? &ring_[t % CAP] : nullptr;
  }
  // the job taken last is done
  void finish() { done_.store(tail_.load(std::memory_order_relaxed), std::memory_order_release); }

  // until job n is done, or (err given) an error has been noted
  void wait_done(unsigned long long n, const FirstError* err = nullptr) const {
    while (done_.load(std::memory_order_acquire) < n && !(err && err->code(std::memory_order_relaxed))) __builtin_ia32_pause();
  }

 private:
  Job ring_[CAP];
  std::atomic<unsigned long long> head_{0}, tail_{0}, done_{0};  // posted / taken / finished
  Doorbell bell_;
};

}  // namespace
