// The agreement among a sharded handle's device threads (x_maps_amd/csrc/host/xm_agree.hpp) on its own, built with
// ThreadSanitizer by tests/test_host_agree_cpu.py.  W = 1, 2, 4, 8 threads that live as long as the library's device threads do
// and run frame after frame; the caller resets the agreement in front of every frame, as xm_sharded_process_frame does.
//   clean frame:    four rounds -- 1. all ranks fine: 0;  2. one rank brings a code: everybody gets it;  3. two ranks bring
//                   different codes: everybody gets the same one of the two;  4. all fine again: 0 (a round leaves nothing behind)
//   poisoned frame: one round all fine, then one rank leaves with a code instead of arriving (now and then late enough for its
//                   peers to be asleep in the round): all of them return that code, nobody hangs;  a rank that arrives after the
//                   poison returns it at once, its own code if it brings one;  then everybody leaves with what it got
//   the clean frame that follows a poisoned one is "reset() followed by a clean round".
// Prints "ok" and exits 0; any failed check exits 1 (a lost wake-up hangs: the test's time limit catches that).
#include "../../x_maps_amd/csrc/host/xm_agree.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// W threads and the start / done hand-shake of the library's device threads: run(fn) has every thread call fn(rank) once
class Crew {
 public:
  explicit Crew(int W) {
    for (int g = 0; g < W; ++g) th_.emplace_back([this, g] { loop(g); });
  }
  ~Crew() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  void run(const std::function<void(int)>& fn) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn;
      done_ = 0;
      gen_ += 1;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return done_ == (int)th_.size(); });
  }

 private:
  void loop(int g) {
    unsigned long long seen = 0;
    for (;;) {
      const std::function<void(int)>* fn;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        fn = fn_;
      }
      (*fn)(g);
      {
        std::lock_guard<std::mutex> lk(mu_);
        done_ += 1;
      }
      cv_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  const std::function<void(int)>* fn_ = nullptr;
  unsigned long long gen_ = 0;
  int done_ = 0;
  bool stop_ = false;
};

void stress(int W, int frames) {
  Agreement a(W);
  Crew crew(W);
  std::vector<int> got(W);  // (every rank writes its own entry; the caller reads them behind run())
  for (int f = 0; f < frames; ++f) {
    a.reset();
    const int r1 = f % W, r2 = W > 1 ? (r1 + 1 + (f / W) % (W - 1)) % W : 0;  // (W > 1: two different ranks)
    const int c1 = 100 + f % 7, c2 = 200 + f % 5;
    if (f % 2 == 0) {
      crew.run([&](int g) {
        CHECK(a.agree(0) == 0);
        CHECK(a.agree(g == r1 ? c1 : 0) == c1);
        const int both = a.agree(g == r1 ? c1 : g == r2 ? c2 : 0);
        CHECK(both == c1 || (W > 1 && both == c2));
        got[g] = both;
        CHECK(a.agree(0) == 0);
        a.leave(0);
      });
      for (int g = 0; g < W; ++g) CHECK(got[g] == got[0]);
    } else if (W == 1) {  // a world of one: agree hands back what it was given, leave poisons nothing
      crew.run([&](int) {
        CHECK(a.agree(0) == 0);
        a.leave(c1);
        CHECK(a.agree(0) == 0 && a.agree(c2) == c2);
      });
    } else {
      const bool late = f % 64 == 1;  // the leaver's peers are asleep in the round by then
      crew.run([&](int g) {
        CHECK(a.agree(0) == 0);
        if (g == r1) {
          if (late) std::this_thread::sleep_for(std::chrono::microseconds(300));
          a.leave(c1);
          return;
        }
        CHECK(a.agree(0) == c1);                           // waiting when the poison came, or arriving behind it
        const int own = g == r2 ? c2 : 0;
        const int after = a.agree(own);                    // behind the poison for certain: at once, the own code first
        CHECK(after == (own ? own : c1));
        a.leave(after);                                    // (the first poison stays)
      });
      crew.run([&](int g) { CHECK(a.agree(0) == c1 && a.agree(g + 1) == g + 1); });  // still poisoned until the reset
    }
  }
}

int main() {
  for (int W : {1, 2, 4, 8}) stress(W, 1500);
  std::puts("ok");
  return 0;
}
