// vo_loop_scale.hpp -- the VO loop's scale LM call (vo_loop.cpp): Optimiser<ScaleState,...>::optimise over the
// tracks seen in a keyframe, on that keyframe's images; on the scale worker beside the BA, or inline on one context.
// The call's arguments live here while the worker runs it.
#pragma once
#include <vector>

#include "vo_loop_env.hpp"
#include "vo_math.hpp"
#include "vo_tracks.hpp"

namespace me_vo {

struct ScaleCall {
  Env& env;
  explicit ScaleCall(Env& e) : env(e) {}
  std::vector<double> sc_X;
  std::vector<uint8_t> sc_tri;
  std::vector<uint32_t> sc_last;
  me_scale_state sc_s{};
  me_optim_params sc_p{};
  int sc_stop = 0, sc_it = 0;
  long sc_nmi = 0, sc_cnt[4] = {0, 0, 0, 0};
  std::vector<double> sc_trace = std::vector<double>(800);
  bool queued = false;
  long seq = 0;

  void close() {
    if (queued) {
      env.scale_worker.wait(seq);
      queued = false;
    }
  }
  // Keyframe t at `pose` with the prepared pair im: the landmarks of the tracks tids, read from the table now
  int submit(int t, const Pose& pose, const Imgs& im, const TrackTable& tab, const std::vector<int64_t>& tids) {
    const me_vo_loop_config& cfg = env.cfg;
    if (queued) {  // a scale job left queued by an earlier error return: it reads sc_s / sc_X
      queued = false;
      VL_TRY(env.scale_worker.wait(seq), "me_scale_optimise");
    }
    const size_t n = tids.size();
    const Mat3 R = aa_to_R(&pose[3]);
    const auto q = R_to_quat(R);
    sc_X.resize(4 * n);
    sc_tri.assign(n, 1);
    sc_last.assign(n, (uint32_t)t);
    for (size_t i = 0; i < n; ++i) {
      const int64_t j = tab.find_id(tids[i]);
      for (int k = 0; k < 3; ++k) sc_X[4 * i + k] = tab.X[3 * j + k];
      sc_X[4 * i + 3] = 1.0;
    }
    me_scale_state& s = sc_s;
    s = me_scale_state{};
    s.n_left = (int)n;
    s.n_right = 0;
    s.X_left = sc_X.data();
    s.X_right = sc_X.data();
    s.tri_left = sc_tri.data();
    s.tri_right = sc_tri.data();
    s.last_left = sc_last.data();
    s.last_right = sc_last.data();
    s.lframe = (uint32_t)t;
    for (int k = 0; k < 9; ++k) s.K1[k] = s.K2[k] = cfg.K[k];
    for (int k = 0; k < 4; ++k) s.q1[k] = s.q2[k] = q[k];
    for (int k = 0; k < 3; ++k) s.t1[k] = s.t2[k] = pose[k];
    s.scale = 1.0;
    s.baseline = cfg.baseline;
    s.window_size = kWScale;
    s.imgL = im.L;
    s.imgR = im.R;
    s.stride = s.cols = cfg.width;
    s.rows = cfg.height;
    s.bb_cols = cfg.width;
    s.bb_rows = cfg.height;
    s.mask = nullptr;
    s.mask_len = 0;
    s.img_mem = ME_DEVICE;
    s.tracks_mem = ME_HOST;
    me_optim_params& p = sc_p;
    p.type = 1;
    p.minim = 1;
    p.max_nb_iter = cfg.scale_iters;
    p.v = 2.0;
    p.tau = 1e-3;
    p.mu = 1e-20;
    p.abs_tol = p.grad_tol = p.incr_tol = p.rel_tol = 0.0;
    p.alpha = 1.0;
    p.weighting = 0;
    auto run = [this]() -> int {
      int rc = me_scale_optimise(env.tctx, &sc_s, &sc_p, 0, &sc_stop, &sc_it, sc_trace.data(), 400, &sc_nmi);
      if (rc == ME_OK) rc = me_scale_last_counters(env.tctx, &sc_cnt[0], &sc_cnt[1], &sc_cnt[2], &sc_cnt[3]);
      return rc;
    };
    if (env.shared) {  // (one context: no second caller, and no window queueing on a worker -- run it now, in loop order)
      VL_TRY(env.timed_wait(2, run), "me_scale_optimise");
      queued = false;
      return ME_OK;
    }
    seq = env.scale_worker.submit(run);
    queued = true;
    return ME_OK;
  }
  int result(double* scale, int* stop, int* iters) {
    if (queued) {
      VL_TRY(env.timed_wait(5, [&] { return env.scale_worker.wait(seq); }), "me_scale_optimise");
      queued = false;
    }
    *scale = sc_s.scale;
    *stop = sc_stop;
    *iters = sc_it;
    return ME_OK;
  }
};

}  // namespace me_vo
