// The helper thread of the one-frame call, on its own: standard headers only, no HIP, so that tests/cpp/launch_helper_main.cpp can build it
// with a plain compiler and a thread sanitizer (tests/test_launch_helper_host.py).  lmx_internal.hpp includes it.
#pragma once

#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>

namespace lmx {

// One persistent helper thread for the one-frame call (lmx_enqueue.cpp issue_small): the caller hands it a job (queue the rest of the kernel
// chain, then store the depth frame) and stores the colour frame itself.  A job arrives every ~100 us when frames are matched back to back and
// a condition-variable wake-up costs 10-50 us, so the helper SPINS for a bounded time after a job (spin_us, 300 us unless a test asks for
// another) before it goes to sleep: a caller in a tight loop finds it awake, a 1 Hz caller (the reference's demo node) pays a wake-up it will
// not notice and no core is kept busy.
//
// The hand-off: submit() increments gen_ (a) and then reads sleeping_ (b); the helper, on its way to sleep and with m_ held, stores
// sleeping_ = true (c) and then reads gen_ in the wait predicate (d).  All four are seq_cst, so they have ONE order: either (d) sees the
// increment and the helper does not sleep, or (d) comes before (a), then (c) before (b), and submit() sees sleeping_ and notifies -- under
// m_, which the helper gives up only inside cv_.wait, so the notification cannot come too early either.  With release / acquire, as it
// was, nothing ordered the store (c) before the load (d) of ANOTHER variable: on x86 (c) could still sit in the store buffer when (d)
// read the old gen_, (b) then read false, nobody notified, and wait() spun for ever (tests/test_launch_helper_host.py shows it).  The
// cost: (c) becomes an xchg, once per sleep; (a) was a locked instruction already, (b) and (d) are plain loads.  The spinning helper's
// own reads of gen_ stay acquire: a caller that comes back within the spin limit is found without a system call, as before.
//
// One caller at a time: submit(), then wait(), which must be reached before the job's captures leave scope (the job writes through them).
// A job that throws does not end the process: wait() returns false and rethrow() hands the exception to the caller's thread.
class LaunchHelper {
 public:
  struct Counters {
    uint64_t jobs;       // jobs run to their end (returned or thrown)
    uint64_t sleeps;     // times the helper gave up spinning and waited on the condition variable
    uint64_t notifies;   // notify_one() calls of submit(): jobs - notifies is about the number of jobs the helper found while still spinning
  };
  explicit LaunchHelper(int spin_us = 300) : spin_us_(spin_us), th_([this]() { run(); }) {}
  ~LaunchHelper() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; gen_.fetch_add(1, std::memory_order_release); }
    cv_.notify_all();
    th_.join();
  }
  LaunchHelper(const LaunchHelper&) = delete;
  LaunchHelper& operator=(const LaunchHelper&) = delete;
  void submit(const std::function<void()>* job) {
    job_ = job;
    error_ = nullptr;
    done_.store(false, std::memory_order_relaxed);
    gen_.fetch_add(1, std::memory_order_seq_cst);       // (a) of the hand-off below; publishes job_ and error_ as a release did
    if (sleeping_.load(std::memory_order_seq_cst)) {   // (b)
      bump(n_notifies_);
      std::lock_guard<std::mutex> lk(m_);
      cv_.notify_one();
    }
  }
  // Returns when the job has ended, however long that takes: the job holds references into the caller's frame.  false: the job threw
  bool wait() const {
    while (!done_.load(std::memory_order_acquire)) __builtin_ia32_pause();
    return !error_;
  }
  void rethrow() const { if (error_) std::rethrow_exception(error_); }   // after a wait() that returned false
  Counters counters() const {
    return {n_jobs_.load(std::memory_order_relaxed), n_sleeps_.load(std::memory_order_relaxed), n_notifies_.load(std::memory_order_relaxed)};
  }

 private:
  // Each counter has ONE writer (jobs and sleeps the helper, notifies the submitting thread), so a relaxed load and store will do -- and must:
  // an atomic read-modify-write is a full fence on x86, and one between the hand-off's accesses would order them by accident.
  static void bump(std::atomic<uint64_t>& n) { n.store(n.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed); }
  void run() {
    uint64_t seen = 0;
    for (;;) {
      const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
      int spins = 0;
      while (gen_.load(std::memory_order_acquire) == seen) {
        __builtin_ia32_pause();
        if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us_)) {
          std::unique_lock<std::mutex> lk(m_);
          bump(n_sleeps_);
          sleeping_.store(true, std::memory_order_seq_cst);                                        // (c)
          cv_.wait(lk, [&]() { return gen_.load(std::memory_order_seq_cst) != seen; });            // (d)
          sleeping_.store(false, std::memory_order_release);
        }
      }
      seen = gen_.load(std::memory_order_acquire);
      { std::lock_guard<std::mutex> lk(m_); if (stop_) return; }
      try {
        (*job_)();
      } catch (...) {
        error_ = std::current_exception();
      }
      bump(n_jobs_);
      done_.store(true, std::memory_order_release);
    }
  }
  const int spin_us_;
  std::mutex m_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<bool> done_{true}, sleeping_{false};
  std::atomic<uint64_t> n_jobs_{0}, n_sleeps_{0}, n_notifies_{0};
  const std::function<void()>* job_ = nullptr;
  std::exception_ptr error_;   // of the last job; written by the helper before done_, read by the caller after it
  bool stop_ = false;
  std::thread th_;   // last: the thread starts with every other member constructed
};

}  // namespace lmx
