// Stress program of lmx::LaunchHelper (csrc/lmx_launch_helper.hpp), the helper thread of the one-frame call, on the CPU alone.
//   usage: launch_helper_main ITERATIONS SPIN_US SEED
// 1. Submit loop: one thread submits job i, waits for it, checks what it wrote, then busy-waits for a gap drawn uniformly from a range around
//    the helper's spin limit, so that the next submit() falls on either side of -- and into -- the helper's spin-to-sleep transition.  The
//    job writes through references into the submitter's frame the way production's job writes rest_st and rest_msg: an int, a std::string and
//    the iteration number, all plain memory, so a thread sanitizer checks their publication through wait().
// 2. Lifetimes: 2000 helpers constructed and destroyed -- at once, after a pause that leaves them spinning or asleep, or right behind a job.
// 3. A job that throws is reported by wait(), rethrown on this thread, and the next job runs as usual -- awake and asleep.
// A watchdog thread ends the process with _Exit(3) when a step is not done 5 s after it began (a lost wake-up: the helper sleeps, the
// submitter spins in wait() for ever) and prints the iteration, the gap and the counters first.
// Last line:  jobs=J sleeps=S awake=J-notifies notifies=N   (of the submit loop's helper)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <functional>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>

#include "lmx_launch_helper.hpp"

using clk = std::chrono::steady_clock;

static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(clk::now().time_since_epoch()).count(); }
static void busy_wait_ns(int64_t ns) {
  const int64_t until = now_ns() + ns;
  while (now_ns() < until) __builtin_ia32_pause();
}

// what the watchdog reads
static std::atomic<int64_t> g_armed_at{0};   // 0: nothing pending
static std::atomic<long> g_iter{0};
static std::atomic<int64_t> g_gap_ns{0};
static std::atomic<const char*> g_phase{"start"};
static std::atomic<const lmx::LaunchHelper*> g_helper{nullptr};   // null while helpers come and go
static std::atomic<bool> g_stop{false};

static void arm(long iter, int64_t gap_ns) {
  g_iter.store(iter, std::memory_order_relaxed);
  g_gap_ns.store(gap_ns, std::memory_order_relaxed);
  g_armed_at.store(now_ns(), std::memory_order_release);
}
static void disarm() { g_armed_at.store(0, std::memory_order_release); }

static void watchdog() {
  while (!g_stop.load(std::memory_order_acquire)) {
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    const int64_t at = g_armed_at.load(std::memory_order_acquire);
    if (at == 0 || now_ns() - at < 5000000000ll) continue;
    if (g_armed_at.load(std::memory_order_acquire) != at) continue;   // that step ended, another began
    const lmx::LaunchHelper* h = g_helper.load(std::memory_order_acquire);
    const lmx::LaunchHelper::Counters k = h ? h->counters() : lmx::LaunchHelper::Counters{0, 0, 0};
    printf("LOST: %s: iteration %ld not done 5 s after it began (gap before it %.1f us); jobs=%llu sleeps=%llu awake=%lld notifies=%llu\n",
           g_phase.load(), g_iter.load(), g_gap_ns.load() / 1e3, (unsigned long long)k.jobs, (unsigned long long)k.sleeps,
           (long long)k.jobs - (long long)k.notifies, (unsigned long long)k.notifies);
    fflush(stdout);
    _Exit(3);
  }
}

static int fail(const char* what, long i) {
  printf("FAIL: %s at iteration %ld\n", what, i);
  fflush(stdout);
  _Exit(2);
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s ITERATIONS SPIN_US SEED\n", argv[0]); return 64; }
  const long iterations = atol(argv[1]);
  const int spin_us = atoi(argv[2]);
  std::mt19937_64 rng((uint64_t)atoll(argv[3]));
  if (iterations < 0 || spin_us < 1) { fprintf(stderr, "bad argument\n"); return 64; }
  // The helper reads the clock every 256 spins only and then takes the mutex, so it falls asleep a few microseconds ABOVE its limit.  The
  // gaps span a quarter of the limit (8 us at the least) on both sides of [limit, limit + 4 us]: about half of the submits find the helper
  // spinning, half asleep, and each draw lands in the transition itself with a probability of a few per cent.
  const int64_t margin_ns = 1000ll * (spin_us / 4 > 8 ? spin_us / 4 : 8);
  const int64_t gap_lo = 1000ll * spin_us - margin_ns, gap_hi = 1000ll * spin_us + 4000 + margin_ns;
  std::uniform_int_distribution<int64_t> gap_dist(gap_lo > 0 ? gap_lo : 0, gap_hi);
  std::thread dog(watchdog);

  // ---- 0. back to back: the hot path ----------------------------------------------------------------------------------------------------
  // A caller that comes straight back finds the helper spinning: no sleep, no notify_one(), no system call.
  lmx::LaunchHelper::Counters b2b;
  const long n_b2b = iterations < 20000 ? iterations : 20000;
  {
    lmx::LaunchHelper helper(spin_us);
    g_phase.store("back to back");
    g_helper.store(&helper, std::memory_order_release);
    long ran = -1;
    for (long i = 0; i < n_b2b; ++i) {
      const std::function<void()> job = [&]() { ran = i; };
      arm(i, 0);
      helper.submit(&job);
      const bool ok = helper.wait();
      disarm();
      if (!ok || ran != i) fail("back to back: the job did not run", i);
    }
    g_helper.store(nullptr, std::memory_order_release);
    b2b = helper.counters();
    g_phase.store("join of the back-to-back helper");
    arm(n_b2b, 0);
  }
  disarm();
  printf("back to back: jobs=%llu sleeps=%llu awake=%lld notifies=%llu\n", (unsigned long long)b2b.jobs, (unsigned long long)b2b.sleeps,
         (long long)b2b.jobs - (long long)b2b.notifies, (unsigned long long)b2b.notifies);

  // ---- 1. the submit loop -------------------------------------------------------------------------------------------------------------
  lmx::LaunchHelper::Counters total;
  {
    lmx::LaunchHelper helper(spin_us);
    g_phase.store("submit loop");
    g_helper.store(&helper, std::memory_order_release);
    long runs = 0;
    int64_t gap = 0;
    for (long i = 0; i < iterations; ++i) {
      int status = -1;
      std::string msg;
      long ran = -1;
      const std::function<void()> job = [&]() {
        status = (int)(i & 0x7fffffff);
        msg = "job " + std::to_string(i);
        ran = i;
        ++runs;
      };
      arm(i, gap);
      helper.submit(&job);
      const bool ok = helper.wait();
      disarm();
      if (!ok) fail("wait() reported a throw of a job that does not throw", i);
      if (ran != i || status != (int)(i & 0x7fffffff) || msg != "job " + std::to_string(i)) fail("the job's results are not job i's", i);
      if (runs != i + 1) fail("job i did not run exactly once", i);
      gap = gap_dist(rng);
      busy_wait_ns(gap);
    }
    g_helper.store(nullptr, std::memory_order_release);
    total = helper.counters();
    if ((long)total.jobs != iterations) fail("the jobs counter is not the number of jobs", iterations);
    g_phase.store("join of the submit loop's helper");
    arm(iterations, 0);
  }
  disarm();

  // ---- 2. lifetimes -------------------------------------------------------------------------------------------------------------------
  g_phase.store("lifetimes");
  std::uniform_int_distribution<int64_t> pause_dist(0, 2 * (1000ll * spin_us + 8000));
  for (long i = 0; i < 2000; ++i) {
    const int kind = (int)(rng() % 4);
    const int64_t pause = pause_dist(rng);
    arm(i, pause);
    {
      lmx::LaunchHelper h(spin_us);
      if (kind == 1) busy_wait_ns(pause);   // destroyed while it spins, or asleep, or on the way there
      if (kind >= 2) {
        if (kind == 3) busy_wait_ns(pause);   // the job's hand-off on either side of the transition too
        int hit = 0;
        const std::function<void()> job = [&]() { ++hit; };
        h.submit(&job);
        if (!h.wait() || hit != 1) fail("lifetimes: the job did not run once", i);
      }   // kind 0: destroyed at once, perhaps before its thread has started
    }
    disarm();
  }

  // ---- 3. a job that throws -----------------------------------------------------------------------------------------------------------
  g_phase.store("throwing job");
  {
    lmx::LaunchHelper h(spin_us);
    for (long i = 0; i < 40; ++i) {
      arm(i, 0);
      if (i & 1) busy_wait_ns(3 * (1000ll * spin_us + 8000));   // the helper asleep
      const std::function<void()> bad = [&]() { throw std::runtime_error("thrown by job " + std::to_string(i)); };
      h.submit(&bad);
      if (h.wait()) fail("wait() did not report the throw", i);
      bool caught = false;
      try {
        h.rethrow();
      } catch (const std::runtime_error& e) {
        caught = std::string(e.what()) == "thrown by job " + std::to_string(i);
      }
      if (!caught) fail("rethrow() did not hand over the job's exception", i);
      long ran = -1;
      const std::function<void()> good = [&]() { ran = i; };
      h.submit(&good);
      if (!h.wait() || ran != i) fail("the job behind a throwing one did not run normally", i);
      h.rethrow();   // nothing to rethrow
      disarm();
    }
    if (h.counters().jobs != 80) fail("throwing jobs are not counted", 40);
    arm(40, 0);
  }
  disarm();

  g_stop.store(true, std::memory_order_release);
  dog.join();
  printf("gaps %.1f .. %.1f us around a spin limit of %d us; 2000 lifetimes and 40 throwing jobs ok\n", (gap_lo > 0 ? gap_lo : 0) / 1e3, gap_hi / 1e3, spin_us);
  printf("jobs=%llu sleeps=%llu awake=%lld notifies=%llu\n", (unsigned long long)total.jobs, (unsigned long long)total.sleeps,
         (long long)total.jobs - (long long)total.notifies, (unsigned long long)total.notifies);
  return 0;
}
