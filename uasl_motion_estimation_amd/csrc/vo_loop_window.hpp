// vo_loop_window.hpp -- the VO loop's device-resident BA window and its solve queue (vo_loop.cpp;
// GPUBackend.window_add / ba_submit_window / ba_result): the observation store on the BA context, the frame map
// into it, the solves queued behind one another and the worker job that queues the newest.
#pragma once
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "vo_blocks.hpp"
#include "vo_loop_env.hpp"
#include "vo_math.hpp"

namespace me_vo {

// A chained solve's start, formed on the device from the previous window's result (the loop's chain_args)
struct Chain {
  std::vector<int32_t> cam_src;
  int32_t new_from;
  me_vo_chain_args a;
  int nc;
};

struct WindowQueue {
  Env& env;
  explicit WindowQueue(Env& e) : env(e) {}
  // the store (me_vo::WStore of wcap observations), two buffers: a full one is compacted into the other
  long wcap = 0, wend = 0;
  void* wstore[2] = {nullptr, nullptr};
  long wcaps[2] = {0, 0};
  int wcur = 0;
  std::map<int, std::pair<long, long>> wfrm;  // frame -> (offset, count)
  struct QSolve {
    me_ba_problem p{};
    me_ba_options o{};
    me_vo_window w{};
    me_ba_point_check_params chk{};  // w.check points here when the residual check is queued
    int nc = 0, npts = 0;
    const int32_t* dev_ids = nullptr;
    int n_ids = 0;
    long seq = 0;  // worker job (0: queued inline)
  };
  std::deque<std::unique_ptr<QSolve>> baq;
  int bw_k = 0;
  long enq_seq = 0;  // newest queued worker job not yet joined (0: none)

  // GPUBackend.reserve: the BA side sized for the configuration's fullest window up front
  int reserve() {
    const me_vo_loop_config& cfg = env.cfg;
    const long n_obs = (long)cfg.window * cfg.n_feats + cfg.n_feats;
    const long n_pts = n_obs;
    const int nc = cfg.window;
    const long cap = 2 * n_obs;
    if (wend == 0 && wcap < cap) {
      for (int k = 0; k < 2; ++k) {
        if (wstore[k]) VL_TRY(me_free(env.ctx, wstore[k]), "free");
        wstore[k] = nullptr;
        VL_TRY(me_malloc(env.ctx, &wstore[k], WStore{(size_t)cap}.size()), "malloc");
        wcaps[k] = cap;
      }
      wcap = cap;
    }
    const size_t nb = BaUpload{(size_t)nc, (size_t)n_pts}.size();
    void* q;
    for (int k = 0; k < 2; ++k) {
      const std::string s = "bw" + std::to_string(k);
      VL_TRY(env.hbuf(s.c_str(), nb, &q), "reserve");
      VL_TRY(env.dbuf(s.c_str(), nb, &q), "reserve");
      VL_TRY(env.dbuf(("bw_idx" + std::to_string(k)).c_str(), 8 * n_obs, &q), "reserve");
    }
    for (int k = 0; k < 2; ++k)
      VL_TRY(env.hbuf(("w_add" + std::to_string(k)).c_str(), WStore{(size_t)cfg.n_feats}.size(), &q), "reserve");
    VL_TRY(me_ba_reserve(env.ctx, nc, (int)n_pts, (int)n_obs, 4, cfg.fixed_frames), "me_ba_reserve");
    return ME_OK;
  }
  // the queued solves read back and dropped, the store freed; the first error
  int close() {
    int rc = ME_OK;
    if (enq_seq) env.ba_worker.wait(enq_seq);
    enq_seq = 0;
    while (!baq.empty()) {
      std::vector<double> c, p;
      me_ba_summary s;
      const int r = result(c, p, s);
      if (rc == ME_OK) rc = r;
    }
    return rc;
  }
  void free_store() {
    for (auto& w : wstore)
      if (w) me_free(env.ctx, w);
  }

  int join_enqueue() {
    if (enq_seq) {
      const long s = enq_seq;
      enq_seq = 0;
      VL_TRY(env.ba_worker.wait(s), "me_vo_window_submit");
    }
    return ME_OK;
  }
  int window_add(int t, const std::vector<int64_t>& fid, const std::vector<float>& feats) {
    me_ctx* ctx = env.ctx;
    VL_TRY(join_enqueue(), "window");
    const long n = (long)fid.size();
    long live0 = wend;
    for (auto& kv : wfrm) live0 = std::min(live0, kv.second.first);
    const long live = wend - live0;
    if (wend + n > wcap) {
      long cap = std::max<long>(std::max<long>(1L << 16, 2 * (live + n)), wcap);
      const int k = 1 - wcur;
      if (wcaps[k] < cap) {
        if (wstore[k]) VL_TRY(me_free(ctx, wstore[k]), "free");
        wstore[k] = nullptr;
        VL_TRY(me_malloc(ctx, &wstore[k], WStore{(size_t)cap}.size()), "malloc");
        wcaps[k] = cap;
      }
      cap = wcaps[k];
      if (live) {
        const WStore from{(size_t)wcap}, to{(size_t)cap};
        void *src = wstore[wcur], *dst = wstore[k];
        VL_TRY(me_memcpy_d2d(ctx, to.obs(dst), from.obs(src, live0), 32 * live), "window compaction");
        VL_TRY(me_memcpy_d2d(ctx, to.frame(dst), from.frame(src, live0), 4 * live), "window compaction");
        VL_TRY(me_memcpy_d2d(ctx, to.id(dst), from.id(src, live0), 4 * live), "window compaction");
      }
      wcap = cap;
      wcur = k;
      for (auto& kv : wfrm) kv.second.first -= live0;
      wend = live;
    }
    if (n) {
      void* hp;
      VL_TRY(env.hbuf((std::string("w_add") + std::to_string(t & 1)).c_str(), WStore{(size_t)n}.size(), &hp), "window");
      const WStore add{(size_t)n}, st{(size_t)wcap};
      double* ho = add.obs(hp);
      for (long i = 0; i < 4 * n; ++i) ho[i] = (double)feats[i];
      int32_t *hf = add.frame(hp), *hi = add.id(hp);
      for (long i = 0; i < n; ++i) {
        hf[i] = t;
        hi[i] = (int32_t)fid[i];
      }
      void* d = wstore[wcur];
      const long e = wend;
      VL_TRY(me_memcpy_async(ctx, st.obs(d, e), add.obs(hp), 32 * n), "window H2D");
      VL_TRY(me_memcpy_async(ctx, st.frame(d, e), add.frame(hp), 4 * n), "window H2D");
      VL_TRY(me_memcpy_async(ctx, st.id(d, e), add.id(hp), 4 * n), "window H2D");
    }
    wfrm[t] = {wend, n};
    wend += n;
    return ME_OK;
  }
  // cov: the window covariance mode handed to the solve (me_vo_window.cov); check: the residual check's parameters
  // (me_vo_window.check), null: none
  int submit(int f0, const std::vector<int32_t>& win_ids, const std::vector<double>& Xw, const std::vector<Pose>& cams,
             const Chain* chain, int cov, const me_ba_point_check_params* check, int* n_obs_out) {
    const me_vo_loop_config& cfg = env.cfg;
    VL_TRY(join_enqueue(), "window");
    const long off0 = wfrm[f0].first;
    const long n_obs = wend - off0;
    const int npts = (int)win_ids.size(), nc = (int)cams.size();
    const int k = bw_k;
    bw_k ^= 1;
    const BaUpload bw{(size_t)nc, (size_t)npts};
    void *hp, *d, *di;
    VL_TRY(env.hbuf(("bw" + std::to_string(k)).c_str(), bw.size(), &hp), "window");
    for (int c = 0; c < nc; ++c) std::memcpy(bw.cams(hp) + 6 * (size_t)c, cams[c].data(), 48);
    std::memcpy(bw.pts(hp), Xw.data(), 24 * (size_t)npts);
    std::memcpy(bw.ids(hp), win_ids.data(), 4 * (size_t)npts);
    VL_TRY(env.dbuf(("bw" + std::to_string(k)).c_str(), bw.size(), &d), "window");
    VL_TRY(env.dbuf(("bw_idx" + std::to_string(k)).c_str(), 8 * (size_t)std::max<long>(n_obs, 1), &di), "window");
    auto q = std::make_unique<QSolve>();
    me_vo_window& w = q->w;
    w = me_vo_window{};
    w.stage = hp;
    w.dev = d;
    w.stage_bytes = bw.stage_bytes(chain != nullptr);
    if (chain) {
      if (chain->nc != nc || baq.empty()) return env.fail(ME_ERR_STATE, "chain without a queued window");
      std::memcpy(bw.cam_src(hp), chain->cam_src.data(), 4 * (size_t)nc);
      const QSolve& prev = *baq.back();
      w.chain = 1;
      w.cam_src = bw.cam_src(d);
      w.prev_ids = prev.dev_ids;
      w.n_prev = prev.n_ids;
      w.new_from = chain->new_from;
      w.args = chain->a;
    }
    const WStore st{(size_t)wcap};
    void* ws = wstore[wcur];
    w.win_ids = bw.ids(d);
    w.frame = st.frame(ws, off0);
    w.ids = st.id(ws, off0);
    w.first_frame = f0;
    w.cov = cov;
    if (check) {
      q->chk = *check;
      w.check = &q->chk;
    }
    me_ba_problem& p = q->p;
    p = me_ba_problem{};
    p.n_cams = nc;
    p.n_pts = npts;
    p.n_obs = (int)n_obs;
    p.cams = bw.cams(d);
    p.pts = bw.pts(d);
    p.obs = st.obs(ws, off0);
    p.cam_idx = (const int32_t*)di;
    p.pt_idx = (const int32_t*)((uint8_t*)di + 4 * (size_t)n_obs);
    for (int i = 0; i < 9; ++i) p.K0[i] = p.K1[i] = cfg.K[i];
    p.baseline = cfg.baseline;
    p.feat_var = cfg.feat_var;
    p.fixed_frames = cfg.fixed_frames;
    p.mem = ME_DEVICE;
    p.obs_dim = 4;
    me_ba_default_options(&q->o);
    q->o.max_num_iterations = cfg.ba_iters;
    q->o.function_tolerance = q->o.gradient_tolerance = q->o.parameter_tolerance = 0.0;
    q->nc = nc;
    q->npts = npts;
    q->dev_ids = bw.ids(d);
    q->n_ids = npts;
    QSolve* qp = q.get();
    me_ctx* ctx = env.ctx;
    auto enqueue = [ctx, qp]() -> int { return me_vo_window_submit(ctx, &qp->w, &qp->p, &qp->o); };
    if (cfg.async_enqueue) {
      // queued by the worker (the loop thread goes on to wait for the
      // previous window: me_ba_wait_out may run beside the queueing)
      q->seq = enq_seq = env.ba_worker.submit(enqueue);
    } else {
      VL_TRY(env.timed_wait(3, enqueue), "me_vo_window_submit");
    }
    baq.push_back(std::move(q));
    *n_obs_out = (int)n_obs;
    return ME_OK;
  }
  // ccov / pcov / cov_ok (all three or none): the window's covariance, read back with the result; flags / check_ok
  // (both or none): the residual check's flags, one per window point
  int result(std::vector<double>& cams, std::vector<double>& pts, me_ba_summary& s, std::vector<double>* ccov = nullptr,
             std::vector<double>* pcov = nullptr, int* cov_ok = nullptr, std::vector<uint8_t>* flags = nullptr,
             int* check_ok = nullptr) {
    me_ctx* ctx = env.ctx;
    if (baq.empty()) return env.fail(ME_ERR_STATE, "no window solve queued");
    std::unique_ptr<QSolve> q = std::move(baq.front());
    baq.pop_front();
    if (q->seq) {  // this window's own queueing (a newer one's may run on beside the wait)
      VL_TRY(env.ba_worker.wait(q->seq), "me_vo_window_submit");
      if (enq_seq == q->seq) enq_seq = 0;
    }
    cams.assign(6 * (size_t)q->nc, 0.0);
    pts.assign(3 * (size_t)q->npts, 0.0);
    if (check_ok) {
      flags->assign((size_t)q->npts, 0);
      if (cov_ok) {
        ccov->assign(36 * (size_t)q->nc, 0.0);
        pcov->assign(9 * (size_t)q->npts, 0.0);
      }
      VL_TRY(env.timed_wait(4, [&] {
               return me_ba_wait_out_check(ctx, &s, cams.data(), pts.data(), cov_ok ? ccov->data() : nullptr,
                                           cov_ok ? pcov->data() : nullptr, cov_ok, flags->data(), check_ok);
             }), "me_ba_wait_out");
      return ME_OK;
    }
    if (cov_ok) {
      ccov->assign(36 * (size_t)q->nc, 0.0);
      pcov->assign(9 * (size_t)q->npts, 0.0);
      VL_TRY(env.timed_wait(4, [&] {
               return me_ba_wait_out_cov(ctx, &s, cams.data(), pts.data(), ccov->data(), pcov->data(), cov_ok);
             }), "me_ba_wait_out");
      return ME_OK;
    }
    VL_TRY(env.timed_wait(4, [&] { return me_ba_wait_out(ctx, &s, cams.data(), pts.data()); }), "me_ba_wait_out");
    return ME_OK;
  }
};

}  // namespace me_vo
