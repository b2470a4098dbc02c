// vo_loop_env.hpp -- what every part of the VO loop shares (vo_loop.cpp): the two contexts, the configuration,
// the error text, the grow-only device / page-locked buffers, the two worker threads and the wait clock.  Each
// vo_loop_*.hpp part is a plain struct that holds a reference to this and its own state, nothing else.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <map>
#include <string>

#include "../../include/me_hip.h"
#include "vo_loop_worker.hpp"

namespace me_vo {

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Buf {
  void* p = nullptr;
  size_t n = 0;
};

// A prepared 8-bit pair on the device
struct Imgs {
  const uint8_t* L = nullptr;
  const uint8_t* R = nullptr;
};

// (env: a part's reference, me_vo_loop's member, and in Env's own methods a local name for *this)
#define VL_TRY(expr, what)                          \
  do {                                              \
    int rc_ = (expr);                               \
    if (rc_ != ME_OK) return env.fail(rc_, (what)); \
  } while (0)

struct Env {
  me_ctx* ctx = nullptr;   // BA
  me_ctx* tctx = nullptr;  // front end (KLT, matchers, scale LM)
  bool shared = false;     // one context for both: nothing runs on a worker
  me_vo_loop_config cfg{};
  std::string err;
  Worker scale_worker, ba_worker;
  double wait_s = 0, wait_stage[6] = {0, 0, 0, 0, 0, 0};
  std::map<std::string, Buf> dev, pin;  // persistent device / page-locked buffers (grow-only)

  int fail(int rc, const char* what) {
    if (rc == ME_OK) return rc;
    const me_ctx* c = ctx;
    err = std::string(what) + ": " + (c ? me_last_error(c) : "");
    if (tctx && tctx != ctx) {
      const char* m2 = me_last_error(tctx);
      if (m2 && *m2) err += std::string(" | front: ") + m2;
    }
    return rc;
  }
  // Joins the worker threads before a buffer grows: the growth path
  // synchronises, frees and allocates on both contexts, which a worker may be
  // using (a ctx takes one call at a time).  reserve() sizes every
  // buffer for the configuration, so this is not expected after it.  (A job's
  // owner that waits for it again afterwards finds it finished.)
  int quiesce() {
    Env& env = *this;
    VL_TRY(scale_worker.wait(), "me_scale_optimise");
    VL_TRY(ba_worker.wait(), "window submit");
    return ME_OK;
  }
  int dbuf(const char* name, size_t nbytes, void** out) {
    Env& env = *this;
    Buf& b = dev[name];
    if (b.p == nullptr || b.n < nbytes) {
      VL_TRY(quiesce(), "grow");
      if (b.p) {
        VL_TRY(me_synchronize(tctx), "sync");
        VL_TRY(me_synchronize(ctx), "sync");
        VL_TRY(me_free(tctx, b.p), "free");
        b.p = nullptr;
      }
      const size_t nb = std::max<size_t>(4096, (size_t)(nbytes * 1.5));
      VL_TRY(me_malloc(tctx, &b.p, nb), "malloc");
      b.n = nb;
    }
    *out = b.p;
    return ME_OK;
  }
  int hbuf(const char* name, size_t nbytes, void** out) {
    Env& env = *this;
    Buf& b = pin[name];
    if (b.p == nullptr || b.n < nbytes) {
      VL_TRY(quiesce(), "grow");
      if (b.p) {
        VL_TRY(me_synchronize(tctx), "sync");
        VL_TRY(me_synchronize(ctx), "sync");
        VL_TRY(me_host_free(tctx, b.p), "host_free");
        b.p = nullptr;
      }
      const size_t nb = std::max<size_t>(4096, (size_t)(nbytes * 1.5));
      VL_TRY(me_host_alloc(tctx, &b.p, nb), "host_alloc");
      b.n = nb;
    }
    *out = b.p;
    return ME_OK;
  }
  void free_bufs() {
    for (auto& kv : dev) me_free(tctx, kv.second.p);
    for (auto& kv : pin) me_host_free(tctx, kv.second.p);
    dev.clear();
    pin.clear();
  }
  template <class F>
  int timed_wait(int stage, F&& fn) {
    const double t0 = now_s();
    const int rc = fn();
    const double dt = now_s() - t0;
    wait_s += dt;
    wait_stage[stage] += dt;
    return rc;
  }
};

}  // namespace me_vo
