// The host threads' hand-over (x_maps_amd/csrc/host/xm_queue.hpp) on its own, built with ThreadSanitizer by
// tests/test_host_queue_cpu.py:
//   1. 10^6 jobs through a queue of 64: every job arrives once, in order
//   2. a producer that pauses longer than the consumer spins: the consumer sleeps and is woken again and again, no job is lost
//   3. wait_done returns once the job is done, and early once an error has been noted
//   4. FirstError: two threads note at once while a third reads: one code comes out, with its own text
//   5. the hand-over of the ingest's out side: the producer runs some jobs itself -- behind wait_done of everything it posted
//      before -- and posts them marked as done; what both sides write is never written by two at once, and job n stays frame n - 1
// Prints "ok" and exits 0; any failed check exits 1 (a lost wake-up hangs: the test's time limit catches that).
#include "../../x_maps_amd/csrc/host/xm_queue.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

struct Job {
  enum Kind : int { WORK = 0, STOP = 1 };
  int kind = WORK;
  unsigned long long seq = 0;
};

// the consumer side of the library's threads: take, check the order, finish; leaves on STOP
template <typename Q>
unsigned long long consume(Q& q, unsigned spins) {
  unsigned long long want = 1;
  for (;;) {
    const Job j = q.take(spins);
    if (j.kind == Job::STOP) {
      q.finish();
      return want - 1;
    }
    CHECK(j.seq == want);
    want += 1;
    q.finish();
  }
}

void order_under_load() {
  JobQueue<Job, 64> q;
  const unsigned long long n = 1000000;
  unsigned long long got = 0;
  std::thread c([&] { got = consume(q, 20000); });
  for (unsigned long long i = 1; i <= n; ++i) {
    Job j;
    j.seq = i;
    CHECK(q.post(j) == i);
  }
  Job stop;
  stop.kind = Job::STOP;
  q.wait_done(q.post(stop));
  c.join();
  CHECK(got == n);
}

void sleep_and_wake() {
  JobQueue<Job, 64> q;
  const unsigned spins = 64;
  const unsigned long long n = 3000;
  unsigned long long got = 0;
  std::thread c([&] { got = consume(q, spins); });
  unsigned r = 12345;
  for (unsigned long long i = 1; i <= n; ++i) {
    // mostly longer than the consumer's spin budget (it is asleep or falling asleep when the job comes), sometimes not at all
    r = r * 1103515245u + 12345u;
    const unsigned pick = (r >> 16) % 4;
    if (pick == 0) std::this_thread::sleep_for(std::chrono::microseconds(200));
    else if (pick != 3)
      for (unsigned k = 0, m = (r >> 8) % 2048; k < m; ++k) __builtin_ia32_pause();
    Job j;
    j.seq = i;
    q.post(j);
  }
  Job stop;
  stop.kind = Job::STOP;
  q.wait_done(q.post(stop));
  c.join();
  CHECK(got == n);
}

void wait_done_and_errors() {
  JobQueue<Job, 64> q;
  FirstError err;
  std::atomic<unsigned long long> finished{0};
  std::atomic<bool> release{false};
  std::thread c([&] {
    for (;;) {
      const Job j = q.take(20000);
      if (j.kind == Job::STOP) {
        q.finish();
        return;
      }
      if (j.seq == 50) {  // the job fails, and is not finished until the producer has seen the error
        err.note(7, "job 50 failed");
        while (!release.load()) std::this_thread::yield();
      } else {
        std::this_thread::sleep_for(std::chrono::microseconds(20));
      }
      finished.store(j.seq);
      q.finish();
    }
  });
  unsigned long long last = 0;
  for (unsigned long long i = 1; i <= 40; ++i) {
    Job j;
    j.seq = i;
    last = q.post(j);
  }
  q.wait_done(last);
  CHECK(finished.load() == 40);
  for (unsigned long long i = 41; i <= 60; ++i) {
    Job j;
    j.seq = i;
    last = q.post(j);
  }
  q.wait_done(last, &err);  // returns at job 50's error, with jobs 50 .. 60 not done
  CHECK(err.code() == 7);
  CHECK(finished.load() < 50);
  std::string text;
  CHECK(err.take(&text) == 7 && text == "job 50 failed");
  CHECK(err.code() == 0 && err.take(&text) == 0);
  release.store(true);
  q.wait_done(last);
  CHECK(finished.load() == 60);
  Job stop;
  stop.kind = Job::STOP;
  q.post(stop);
  c.join();
}

void first_error_races() {
  const char* texts[3] = {"", "error one from the first thread", "error two from the second thread"};
  const auto matches = [&](int code, const std::string& text) { return (code == 1 || code == 2) && text == texts[code]; };
  for (int round = 0; round < 2000; ++round) {
    FirstError e;
    std::atomic<int> go{0};
    const bool takes = round % 2 == 1;
    const auto noter = [&](int code) {
      go.fetch_add(1);
      while (go.load() < 3) {
      }
      e.note(code, texts[code]);
      if (!takes) e.note(code + 10, "a later error of the same thread");  // (kept out: the first error stays)
    };
    if (!takes) {
      // a reader that only looks: afterwards exactly one code is kept, with its own text
      std::thread a(noter, 1), b(noter, 2), r([&] {
        go.fetch_add(1);
        std::string t;
        for (int i = 0; i < 200; ++i) {
          const int c = e.peek(&t);
          CHECK(c == 0 || matches(c, t));
        }
      });
      a.join();
      b.join();
      r.join();
      std::string t;
      const int c = e.take(&t);
      CHECK(matches(c, t));
      CHECK(e.take(&t) == 0);
    } else {
      // a reader that takes: every code it gets comes with its own text, and no code twice
      int seen[3] = {0, 0, 0};
      std::thread a(noter, 1), b(noter, 2), r([&] {
        go.fetch_add(1);
        std::string t;
        for (int i = 0; i < 200; ++i) {
          const int c = e.take(&t);
          if (c) {
            CHECK(matches(c, t));
            seen[c] += 1;
          }
        }
      });
      a.join();
      b.join();
      r.join();
      std::string t;
      const int c = e.take(&t);
      if (c) {
        CHECK(matches(c, t));
        seen[c] += 1;
      }
      CHECK(seen[1] + seen[2] >= 1 && seen[1] <= 1 && seen[2] <= 1);
    }
  }
}

void producer_takes_some_itself() {
  struct OutJob {
    unsigned long long frame = 0;
    bool done = false, stop = false;
  };
  JobQueue<OutJob, 8> q;
  FirstError err;
  unsigned long long frames_out = 0;  // (plain on purpose: the queue alone orders the two sides' writes)
  std::thread c([&] {
    for (;;) {
      const OutJob j = q.take(64);
      if (!j.stop && !j.done) {
        CHECK(frames_out == j.frame);
        frames_out = j.frame + 1;
      }
      q.finish();
      if (j.stop) return;
    }
  });
  const unsigned long long n = 100000, ahead = 3;
  unsigned r = 2463534242u;
  bool self = false;
  for (unsigned long long f = 0; f < n; ++f) {
    r = r * 1103515245u + 12345u;
    if ((r >> 16) % 16 == 0) self = !self;  // (the mode changes every few frames, as between records and EVT chunks)
    if ((r >> 20) % 512 == 0) std::this_thread::sleep_for(std::chrono::microseconds(100));  // (the consumer falls asleep)
    if (f >= ahead) q.wait_done(f - ahead + 1, &err);  // at most `ahead` frames in front of the finished ones
    OutJob j;
    j.frame = f;
    if (self) {
      q.wait_done(f, &err);  // the frames posted before come first
      CHECK(frames_out == f);
      frames_out = f + 1;
      j.done = true;
    }
    CHECK(q.post(j) == f + 1);
  }
  OutJob stop;
  stop.stop = true;
  q.wait_done(q.post(stop));
  c.join();
  CHECK(frames_out == n && err.code() == 0);
}

int main() {
  order_under_load();
  sleep_and_wake();
  wait_done_and_errors();
  first_error_races();
  producer_takes_some_itself();
  std::printf("ok\n");
  return 0;
}
