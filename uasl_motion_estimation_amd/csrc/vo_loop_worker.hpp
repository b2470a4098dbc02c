// vo_loop_worker.hpp -- the VO loop's worker thread (vo_loop.cpp): the scale LM and the window queueing each
// run on one beside the loop thread.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "../../include/me_hip.h"

namespace me_vo {

// A one-job-at-a-time worker thread: submit() hands it a job, wait(seq)
// blocks until the job numbered seq (or a later one) has finished.
class Worker {
 public:
  ~Worker() {
    {
      std::lock_guard<std::mutex> lk(m_);
      quit_ = true;
    }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
  }
  long submit(std::function<int()> f) {
    if (!th_.joinable()) th_ = std::thread([this] { run(); });
    std::unique_lock<std::mutex> lk(m_);
    // one job at a time: a job still pending or running is finished first
    // (its result code stays for the next wait), so queued_ never runs ahead
    // of a job that would be overwritten
    cv_.wait(lk, [&] { return done_ >= queued_; });
    job_ = std::move(f);
    has_ = true;
    ++queued_;
    cv_.notify_all();
    return queued_;
  }
  // seq < 0: every job queued so far (queued_ is read under the lock)
  int wait(long seq = -1) {
    std::unique_lock<std::mutex> lk(m_);
    if (seq < 0) seq = queued_;
    cv_.wait(lk, [&] { return done_ >= seq; });
    const int r = rc_;
    rc_ = ME_OK;
    return r;
  }

 private:
  void run() {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      cv_.wait(lk, [&] { return has_ || quit_; });
      if (!has_) return;
      auto f = std::move(job_);
      has_ = false;
      lk.unlock();
      const int r = f();
      lk.lock();
      if (r != ME_OK && rc_ == ME_OK) rc_ = r;
      ++done_;
      cv_.notify_all();
    }
  }
  std::thread th_;
  std::mutex m_;
  std::condition_variable cv_;
  std::function<int()> job_;
  bool has_ = false, quit_ = false;
  long queued_ = 0, done_ = 0;
  int rc_ = ME_OK;
};

}  // namespace me_vo
