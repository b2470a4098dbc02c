// vo_loop.cpp -- the windowed stereo VO loop in native code (me_vo_loop_*).
//
// The application loop around the hot path that pipeline.py's
// WindowedStereoVO + GPUBackend run in Python, step for step in C++ over the
// library's own entry points: KLT (me_klt_track), the epipolar MI matchers
// (me_mi_epipolar_match / me_vo_new_cells or, with cfg.detector = 1, the
// corner detector me_vo_new_corners / me_mi_epipolar_match_count), the
// scale LM (me_scale_optimise) and the sliding-window BA queued behind the
// previous window (me_vo_window_submit / me_ba_wait_out).  Host only: no
// kernels here.  The loop is split by owner, each part a plain struct over
// one shared environment (vo_loop_env.hpp):
//   vo_math.hpp           the host arithmetic, pipeline.py's in the same order
//   vo_tracks.hpp         the WBA_Point bookkeeping: track table, observation store, event log
//   vo_blocks.hpp         the packed device block layouts and the pair pool's rule
//   vo_loop_worker.hpp    the worker thread
//   vo_loop_images.hpp    the image chain and the pair pool
//   vo_loop_front.hpp     tracker, matchers, gate, new features
//   vo_loop_scale.hpp     the scale LM call
//   vo_loop_window.hpp    the device-resident BA window and the solve queue
//   vo_loop_keyframe.hpp  keyframe selection and frame pose state
// me_vo_loop below keeps the parts, the lagged state, the poses, the
// covariance maps and the steps that tie them together, and the C ABI.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "me_internal.hpp"
#include "vo_blocks.hpp"
#include "vo_loop_env.hpp"
#include "vo_loop_front.hpp"
#include "vo_loop_images.hpp"
#include "vo_loop_keyframe.hpp"
#include "vo_loop_scale.hpp"
#include "vo_loop_window.hpp"
#include "vo_math.hpp"
#include "vo_tracks.hpp"

using namespace me_vo;

struct me_vo_loop {
  Env env;
  ImageChain images{env};
  FrontEnd front{env};
  ScaleCall scale{env};
  WindowQueue win{env};
  KeyframeState kf{env};
  TrackTable tab;
  // the window covariance (me_vo_loop_set_covariance): 0 off, 1 camera blocks, 2 also landmark blocks; per keyframe
  // the last camera's block of its own window, per live track the block of the latest window that held it
  // (36 / 9 doubles and the ok word behind them; zeros with ok 0 after a failed solve or covariance)
  int cov_mode = 0;
  std::map<int, std::vector<double>> pose_cov;
  std::map<int64_t, std::vector<double>> track_cov;
  // the residual check behind every window solve (me_vo_loop_set_track_check) and what it flagged so far
  bool track_check = false;
  me_ba_point_check_params check_params{};
  struct Flagged {
    int32_t t;
    int64_t id;
    uint8_t flags;
  };
  std::vector<Flagged> flagged;
  bool klt_predict = false;  // the tracker starts at each landmark's predicted pixel (me_vo_loop_set_klt_predict)
  long n_pushed = 0;
  Camera cam;
  std::map<int, Pose> poses;
  Pose first_pose{};
  std::map<int, Imgs> imgs;  // device pointers of the keyframes in use
  int depth = 0;             // the entry point the loop's keyframes come through (0: none yet, 8, 16)
  bool has_prev = false;
  int prev_t = -1;
  // ---- lagged state
  struct Pending {
    int t, n_tracked, n_new, n_active;
    bool has_ba;
    BaRec ba;
  };
  bool has_pending = false;
  Pending pending{};
  bool has_scale_args = false;
  int scale_t = -1;
  std::vector<int64_t> scale_tids;
  bool failed = false;  // a process() call returned an error: later calls are refused
  // ---- results / stats
  std::vector<me_vo_frame_result> results;
  double host_s = 0;

  // ------------------------------------------------------------ setup
  int init(const me_vo_loop_config& c) {
    env.cfg = c;
    cam = Camera{c.K[0], c.K[2], c.K[5], c.baseline};
    front.grid = make_grid(c.width, c.height, c.n_feats);
    tab.log_events = c.log_events != 0;
    for (int k = 0; k < 6; ++k) first_pose[k] = c.first_pose[k];
    env.shared = env.ctx == env.tctx;
    if (env.shared) env.cfg.async_enqueue = 0;
    return win.reserve();
  }
  int close() {
    scale.close();
    const int rc = win.close();
    me_synchronize(env.tctx);
    me_synchronize(env.ctx);
    win.free_store();
    images.close();
    env.free_bufs();
    return rc;
  }

  // ------------------------------------------------------------ loop steps (pipeline.py)
  Pose predict(int t) const {
    return predict_pose(poses, t, first_pose, env.cfg.has_velocity ? env.cfg.velocity : nullptr);
  }
  void pop(int new_first) {
    std::vector<int> frames;
    std::vector<int64_t> gone;
    tab.pop(new_first, frames, gone);
    for (int fr : frames) win.wfrm.erase(fr);  // window_pop
    if (cov_mode == 2)
      for (int64_t id : gone) track_cov.erase(id);
  }
  int scale_submit() { return scale.submit(scale_t, poses[scale_t], imgs[scale_t], tab, scale_tids); }

  // ---- WindowedStereoVO steps
  bool chain_args(int t, const Pose& pose, const Mat3& R_pose, const std::vector<int64_t>& new_ids, Chain& ch) {
    const me_vo_loop_config& cfg = env.cfg;
    if (!has_pending || !pending.has_ba) return false;
    const int f0 = std::max(0, t - cfg.window + 1);
    if (t - f0 + 1 <= cfg.fixed_frames) return false;
    const int pt = pending.ba.t, pf0 = pending.ba.f0;
    const int nc = t - f0 + 1, k1 = t - 1 - f0;
    int mode, k0;
    double vel[6] = {0, 0, 0, 0, 0, 0};
    if (t == 1 || !poses.count(t - 2)) {
      mode = 0;
      k0 = -1;
      if (cfg.has_velocity)
        for (int k = 0; k < 6; ++k) vel[k] = cfg.velocity[k];
    } else if (t - 2 >= f0) {
      mode = 1;
      k0 = t - 2 - f0;
    } else {
      return false;
    }
    if (k1 < 0 || pt != t - 1) return false;
    ch.cam_src.clear();
    for (int fr = f0; fr < t; ++fr) ch.cam_src.push_back(pf0 <= fr && fr <= pt ? fr - pf0 : -1);
    ch.cam_src.push_back(-1);
    ch.new_from = new_ids.empty() ? (int32_t)2147483647 : (int32_t)new_ids[0];
    for (int k = 0; k < 6; ++k) ch.a.pose[k] = pose[k];
    for (int k = 0; k < 9; ++k) ch.a.R[k] = R_pose[k];
    for (int k = 0; k < 6; ++k) ch.a.vel[k] = vel[k];
    ch.a.k1 = k1;
    ch.a.k0 = k0;
    ch.a.mode = mode;
    ch.nc = nc;
    return true;
  }
  int ba_submit(int t, const Chain* chain, bool* has, BaRec* rec) {
    *has = false;
    const int f0 = std::max(0, t - env.cfg.window + 1);
    if (t - f0 + 1 <= env.cfg.fixed_frames) return ME_OK;
    rec->t = t;
    rec->f0 = f0;
    std::vector<int32_t> wid32;
    std::vector<double> Xw;
    if (!tab.window_rows(f0, *rec, wid32, Xw))
      return env.fail(ME_ERR_STATE, "track IDs exceed the device window's int32");
    std::vector<Pose> cams;
    for (int fr = f0; fr <= t; ++fr) cams.push_back(poses[fr]);
    VL_TRY(win.submit(f0, wid32, Xw, cams, chain, cov_mode, track_check ? &check_params : nullptr, &rec->nobs), "window");
    *has = true;
    return ME_OK;
  }
  int ba_finish(bool has, const BaRec& ba, int* nwp, int* nwo, int* iters, double* cost) {
    if (!has) {
      *nwp = *nwo = *iters = 0;
      *cost = std::numeric_limits<double>::quiet_NaN();
      return ME_OK;
    }
    std::vector<double> c, p, ccov, pcov;
    me_ba_summary s;
    std::vector<uint8_t> flags;
    int cov_ok = 0, check_ok = 0;
    if (track_check)
      VL_TRY(win.result(c, p, s, cov_mode ? &ccov : nullptr, cov_mode ? &pcov : nullptr, cov_mode ? &cov_ok : nullptr,
                        &flags, &check_ok), "BA result");
    else if (cov_mode)
      VL_TRY(win.result(c, p, s, &ccov, &pcov, &cov_ok), "BA result");
    else
      VL_TRY(win.result(c, p, s), "BA result");
    const size_t m = ba.upts.size();
    std::vector<int64_t> j;
    std::vector<uint8_t> live;
    tab.resolve(ba, j, live);
    if (s.status == 2) {
      for (int k = 0, fr = ba.f0; fr <= ba.t; ++fr, ++k)
        for (int q = 0; q < 6; ++q) poses[fr][q] = c[6 * (size_t)k + q];
      for (size_t i = 0; i < m; ++i)
        if (live[i])
          for (int q = 0; q < 3; ++q) tab.X[3 * j[i] + q] = p[3 * i + q];
    }
    if (cov_mode) {  // (read only: nothing above depends on it)
      const bool good = s.status == 2 && cov_ok != 0;
      std::vector<double> e(37, 0.0);
      if (good) {
        std::memcpy(e.data(), &ccov[36 * (size_t)(ba.t - ba.f0)], 36 * sizeof(double));
        e[36] = 1.0;
      }
      pose_cov[ba.t] = e;
      if (cov_mode == 2)
        for (size_t i = 0; i < m; ++i) {
          if (!live[i]) continue;
          std::vector<double> b(10, 0.0);
          if (good && cov_ok == 2) {
            std::memcpy(b.data(), &pcov[9 * i], 9 * sizeof(double));
            b[9] = 1.0;
          }
          track_cov[ba.wids[i]] = b;
        }
    }
    if (track_check && s.status == 2 && check_ok) {  // the flagged tracks still in the table are tracked no further
      std::vector<int64_t> rows;
      for (size_t i = 0; i < m; ++i)
        if (live[i] && flags[i]) {
          rows.push_back(j[i]);
          flagged.push_back(Flagged{(int32_t)ba.t, ba.wids[i], flags[i]});
        }
      tab.deactivate(rows);
    }
    *nwp = (int)ba.wids.size();
    *nwo = ba.nobs;
    *iters = s.iterations;
    *cost = s.final_cost;
    return ME_OK;
  }
  int complete_result(bool have, int t, int n_tracked, int n_new, int n_active, int nwp, int nwo, int ba_iters,
                      double cost) {
    if (!have) return ME_OK;
    me_vo_frame_result r{};
    VL_TRY(scale.result(&r.scale, &r.scale_stop, &r.scale_iters), "scale");
    r.t = t;
    r.n_tracked = n_tracked;
    r.n_new = n_new;
    r.n_active = n_active;
    r.n_window_pts = nwp;
    r.n_window_obs = nwo;
    r.ba_iters = ba_iters;
    r.ba_cost = cost;
    for (int k = 0; k < 6; ++k) r.pose[k] = poses[t][k];
    results.push_back(r);
    return ME_OK;
  }

  // pipeline.WindowedStereoVO.process (the steps are numbered as there)
  // im: keyframe t's prepared pair; kf_guess (me_vo_loop_push): the tracker's guess, ahead of klt_predict's
  int process(int t, const Imgs& im, const std::vector<float>* kf_guess = nullptr) {
    const me_vo_loop_config& cfg = env.cfg;
    const double t_in = now_s();
    const double w0 = env.wait_s;
    imgs[t] = im;
    // 1. KLT of the active tracks, queued first (it needs only frame t-1's features)
    std::vector<int64_t> act;
    tab.active_rows(act);
    const bool klt = has_prev && !act.empty();
    KltIn kin{0, false, false};  // the tracker's upload, which the gate of step 4 reads again
    if (klt) {
      std::vector<float> pts(2 * act.size()), pxr(front.gate ? act.size() : 0);
      tab.klt_upload(prev_t, act, pts, pxr);
      std::vector<float> guess;
      if (kf_guess) {  // (me_vo_loop_push: the carried positions, ahead of klt_predict's projections)
        if (kf_guess->size() != 2 * act.size()) {
          env.err = "me_vo_loop_push: the carried state does not match the active tracks";
          return ME_ERR_STATE;
        }
      } else if (klt_predict) {
        // pose(t) ahead of step 3 (the pops in between change none of its inputs); pipeline.predict_uv
        const Pose gp = predict(t);
        const Mat3 R = aa_to_R(&gp[3]);
        guess.resize(2 * act.size());
        for (size_t k = 0; k < act.size(); ++k) predict_uv(&tab.X[3 * act[k]], R, gp, cam, &guess[2 * k]);
      }
      if (!kf_guess && klt_predict) kf_guess = &guess;
      kin = KltIn{act.size(), kf_guess != nullptr, front.gate};
      VL_TRY(front.klt_submit(imgs[prev_t], im, kin, pts, kf_guess, front.gate ? &pxr : nullptr), "klt");
    }
    // 2. pops of frame t-1's completion
    if (has_pending) pop(pending.t + 1 - cfg.window);
    // 3. prediction from the lagged state
    const Pose pose = predict(t);
    poses[t] = pose;
    const int nd_new = cfg.d_max - cfg.d_min + 1;
    std::vector<int64_t> trk_idx;
    std::vector<float> trk_uv, xr_trk, nuv, nxr;
    std::vector<uint8_t> nok;
    if (klt) {
      // 4. KLT gate + matching of the tracked features around their predicted disparity, the new
      // features of the cells they leave empty -- one round trip
      tab.active_rows(act);
      const int n = (int)act.size();
      const Mat3 R = aa_to_R(&pose[3]);
      std::vector<int32_t> lo(n);
      std::vector<uint8_t> dvalid(n);
      for (int k = 0; k < n; ++k)
        search_window(predicted_disparity(&tab.X[3 * act[k]], R, pose, cam), cfg.d_min, cfg.d_max, &lo[k], &dvalid[k]);
      std::vector<float> uv, xr_all;
      std::vector<uint8_t> st, ok;
      VL_TRY(front.klt_match_new(kin, im, lo, dvalid, t, 2 * kHalf + 1, nd_new, uv, st, xr_all, ok, nuv, nxr, nok),
             "klt_match_new");
      for (int k = 0; k < n; ++k) {
        const bool good = st[k] == 1 && in_margin(uv[2 * k], uv[2 * k + 1], cfg.width, cfg.height) && ok[k];
        if (!good) {
          tab.active[act[k]] = 0;
          continue;
        }
        trk_idx.push_back(act[k]);
        trk_uv.push_back(uv[2 * k]);
        trk_uv.push_back(uv[2 * k + 1]);
        xr_trk.push_back(xr_all[k]);
      }
    } else if (cfg.detector == 1) {
      VL_TRY(front.corners_match(im, nd_new, nuv, nxr, nok), "corners_match");
    } else {
      new_cells_host(t, 0, nullptr, front.grid, cfg.n_feats, nuv);
      VL_TRY(front.match(im, nuv, nd_new, nxr, nok), "match");
    }
    // 6. frame t-1's scale LM queued now (front end, beside BA(t-1))
    if (has_scale_args) {
      VL_TRY(scale_submit(), "scale");
      has_scale_args = false;
    }
    const int n_tracked = (int)trk_idx.size();
    // 5. bookkeeping: new tracks (triangulated at the predicted pose), this frame's features
    const Mat3 R_pose = aa_to_R(&pose[3]);
    std::vector<double> new_X;
    for (size_t k = 0; k < nok.size(); ++k) {
      if (!nok[k]) continue;
      double Xn[3];
      triangulate(nuv[2 * k], nuv[2 * k + 1], nxr[k], cam, pose, R_pose, Xn);
      new_X.insert(new_X.end(), Xn, Xn + 3);
    }
    std::vector<int64_t> fid, new_ids;
    tab.book(t, trk_idx, trk_uv, xr_trk, nuv, nxr, nok, new_X, fid, new_ids);
    // 8 (chained). BA(t) queued now, behind BA(t-1), its start formed on the device
    Chain ch;
    const bool chained = chain_args(t, pose, R_pose, new_ids, ch);
    bool has_ba = false;
    BaRec rec;
    if (chained) {
      VL_TRY(win.window_add(t, fid, tab.obs[t].feats), "window");
      VL_TRY(ba_submit(t, &ch, &has_ba, &rec), "BA");
    }
    // 7. frame t-1's BA applied
    bool done = false;
    int d_t = 0, d_tr = 0, d_new = 0, d_act = 0, nwp = 0, nwo = 0, bit = 0;
    double bcost = 0;
    if (has_pending) {
      done = true;
      d_t = pending.t;
      d_tr = pending.n_tracked;
      d_new = pending.n_new;
      d_act = pending.n_active;
      const Pending pd = pending;
      has_pending = false;
      VL_TRY(ba_finish(pd.has_ba, pd.ba, &nwp, &nwo, &bit, &bcost), "BA");
    }
    // pose(t) again from the refined poses; the new landmarks of t keep their camera-frame coordinates
    const Pose pose2 = predict(t);
    if (pose2 != pose && !new_ids.empty()) {
      const Mat3 R2 = rot_series(&pose2[3]);
      for (int64_t id : new_ids) move_landmark(&tab.X[3 * tab.find_id(id)], R_pose, pose, pose2, R2);
    }
    poses[t] = pose2;
    // 8. the window's observations, BA(t) queued (unchained)
    if (!chained) {
      VL_TRY(win.window_add(t, fid, tab.obs[t].feats), "window");
      VL_TRY(ba_submit(t, nullptr, &has_ba, &rec), "BA");
    }
    has_scale_args = true;
    scale_t = t;
    scale_tids = fid;
    int n_act = 0;
    for (uint8_t a : tab.active) n_act += a;
    pending = Pending{t, n_tracked, (int)new_ids.size(), n_act, has_ba, std::move(rec)};
    has_pending = true;
    has_prev = true;
    prev_t = t;
    // (images older than t - 1 are no longer read: KLT(t+1) reads t, the scale LM of t runs in process(t + 1))
    for (auto it = imgs.begin(); it != imgs.end();)
      it = it->first < t - 1 ? imgs.erase(it) : std::next(it);
    // 9. frame t-1's FrameResult (its scale LM result), while BA(t) runs
    VL_TRY(complete_result(done, d_t, d_tr, d_new, d_act, nwp, nwo, bit, bcost), "result");
    host_s += (now_s() - t_in) - (env.wait_s - w0);
    return ME_OK;
  }
  // ------------------------------------------------------------ me_vo_loop_push (pipeline.WindowedStereoVO.push)
  int kf_seed(int t) {
    std::vector<float> ref, xr;
    tab.seeded(t, kf.fpose, ref, xr);
    return kf.kf_seed(ref, xr);
  }
  int push(const uint8_t* left, const uint8_t* right, me_mem mem, int* keyframe_t) {
    *keyframe_t = -1;
    const int slot = images.pick(true);
    Imgs im;
    VL_TRY(images.prepare(left, right, mem, 8, true, slot, im), "images");
    ++n_pushed;
    std::vector<float> guess;
    bool guided = false;
    if (has_prev) {
      ++kf.kf_gap;
      const Imgs pv = images.slot_prev >= 0 ? images.push_imgs : imgs[prev_t];
      alignas(8) unsigned char info[160] = {0};
      VL_TRY(kf.kf_track(pv, im, info), "kf_track");
      int32_t flags;
      std::memcpy(&flags, info + 12, 4);
      if (kf.fpose)  // the record: nothing below reads it
        kf.record_pose(info, (int32_t)(n_pushed - 1), flags != 0 ? prev_t + 1 : -1, prev_t);
      if (flags == 0) {  // no keyframe: the frame becomes the previous pushed frame, nothing else moves
        images.slot_prev = slot;
        images.push_imgs = im;
        return ME_OK;
      }
      if (kf.kf_gap >= 2 && kf.kf_n > 0) {
        VL_TRY(kf.kf_read_guess(guess), "kf_guess");
        guided = true;
      }
    }
    const int t = has_prev ? prev_t + 1 : 0;
    if (const int rc = process(t, im, guided ? &guess : nullptr)) return rc;
    images.hold_keyframe(slot);
    VL_TRY(kf_seed(t), "kf_seed");
    *keyframe_t = t;
    return ME_OK;
  }
  // me_vo_loop_process / me_vo_loop_process16 (bits 8 / 16): every frame is a keyframe, the pool's pick is t % 3
  int keyframe(int t, const void* left, const void* right, me_mem mem, int bits) {
    const double t_in = now_s();
    const int slot = images.pick(false);
    Imgs im;
    VL_TRY(images.prepare(left, right, mem, bits, false, slot, im), "images");
    host_s += now_s() - t_in;
    if (const int rc = process(t, im)) return rc;
    images.hold_keyframe(slot);
    return ME_OK;
  }
  int finish() {
    const double t_in = now_s();
    const double w0 = env.wait_s;
    if (has_pending) pop(pending.t + 1 - env.cfg.window);
    if (has_scale_args) {
      VL_TRY(scale_submit(), "scale");
      has_scale_args = false;
    }
    if (has_pending) {
      int nwp, nwo, bit;
      double bcost;
      const Pending pd = pending;
      has_pending = false;
      VL_TRY(ba_finish(pd.has_ba, pd.ba, &nwp, &nwo, &bit, &bcost), "BA");
      VL_TRY(complete_result(true, pd.t, pd.n_tracked, pd.n_new, pd.n_active, nwp, nwo, bit, bcost), "result");
    }
    host_s += (now_s() - t_in) - (env.wait_s - w0);
    return ME_OK;
  }
};

#undef VL_TRY

namespace {

// A switch is set before the loop's first frame: refused (msg) once a keyframe went through, or a call failed
bool started(me_vo_loop* v, const char* msg) {
  if (v->has_prev || v->failed) v->env.err = msg;
  return v->has_prev || v->failed;
}

// The checks the frame entries share, in this order: frames come through me_vo_loop_push or keyframes through
// me_vo_loop_process*, never both; keyframes in order (a pushed frame has no t: the loop numbers its keyframes); no
// earlier failure; one depth (bits 8 / 16) per loop, which is recorded
int enter(me_vo_loop* v, const char* who, bool push, int t, int bits) {
  const auto refuse = [&](const std::string& why) {
    v->env.err = std::string(who) + ": " + why;
    return ME_ERR_STATE;
  };
  if (!push && v->n_pushed > 0) return refuse("this loop's frames come through me_vo_loop_push");
  if (!push && t != (v->has_prev ? v->prev_t + 1 : 0)) return refuse("keyframes must come in order 0, 1, 2, ...");
  if (v->failed) return refuse("an earlier call failed (" + v->env.err + "); the loop state is undefined");
  if (push ? v->has_prev && v->n_pushed == 0 : v->depth != 0 && v->depth != bits)
    return refuse(std::string("this loop's keyframes come through ") +
                  (v->depth == 16 ? "me_vo_loop_process16" : "me_vo_loop_process"));
  v->depth = bits;
  return ME_OK;
}

}  // namespace

extern "C" {

void me_vo_loop_default_config(me_vo_loop_config* c) {
  *c = me_vo_loop_config{};
  c->width = 1280;
  c->height = 720;
  c->n_feats = 2000;
  c->window = 20;
  c->ba_iters = 10;
  c->scale_iters = 10;
  c->fixed_frames = 2;
  c->d_min = 2;
  c->d_max = 128;
  c->baseline = 0.5;
  c->feat_var = 0.25;
  const double f = 0.9 * c->width;
  const double K[9] = {f, 0, c->width / 2.0, 0, f, c->height / 2.0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) c->K[k] = K[k];
  c->async_enqueue = 1;
  c->detector = 0;
  c->corner_win = 21;
  c->corner_min_eig = 1e-4;
  c->klt_fb_max = 0.0;
}

int me_vo_loop_create(me_ctx* ba, me_ctx* front, const me_vo_loop_config* cfg, me_vo_loop** out) {
  if (!out) return ME_ERR_INVALID;
  *out = nullptr;
  if (!ba || !front || !cfg) return ME_ERR_INVALID;
  if (cfg->width < 2 * kMargin + 1 || cfg->height < 2 * kMargin + 1 || cfg->n_feats <= 0 || cfg->window < 1 ||
      cfg->d_min < 0 || cfg->d_max < cfg->d_min || cfg->ba_iters < 0 || cfg->scale_iters < 0)
    return me_set_error(ba, ME_ERR_INVALID, "me_vo_loop_create: bad configuration");
  if (cfg->detector != 0 && cfg->detector != 1)
    return me_set_error(ba, ME_ERR_INVALID, "me_vo_loop_create: detector must be 0 (grid) or 1 (corners)");
  if (cfg->detector == 1 &&
      (cfg->corner_win < 3 || cfg->corner_win > 31 || !(cfg->corner_win & 1) || !(cfg->corner_min_eig > 0.0)))
    return me_set_error(ba, ME_ERR_INVALID,
                        "me_vo_loop_create: corner_win must be odd and in [3, 31], corner_min_eig > 0");
  if (!(cfg->klt_fb_max >= 0.0))  // (false for NaN)
    return me_set_error(ba, ME_ERR_INVALID,
                        "me_vo_loop_create: klt_fb_max must be >= 0 (0: no forward-backward check)");
  auto v = std::make_unique<me_vo_loop>();
  v->env.ctx = ba;
  v->env.tctx = front;
  const int rc = v->init(*cfg);
  if (rc != ME_OK) {
    v->close();
    return rc;
  }
  *out = v.release();
  return ME_OK;
}

void me_vo_loop_destroy(me_vo_loop* v) {
  if (!v) return;
  v->close();
  delete v;
}

const char* me_vo_loop_last_error(const me_vo_loop* v) { return v ? v->env.err.c_str() : "null loop"; }

int me_vo_loop_set_match_lr(me_vo_loop* v, double lr_max) {
  if (!v) return ME_ERR_INVALID;
  if (!(lr_max >= 0.0)) {  // (false for NaN)
    v->env.err = "me_vo_loop_set_match_lr: match_lr_max must be >= 0 (0: no left-right check)";
    return ME_ERR_INVALID;
  }
  if (started(v, "me_vo_loop_set_match_lr: match_lr_max is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  v->front.match_lr = lr_max;
  return ME_OK;
}

int me_vo_loop_set_motion_gate(me_vo_loop* v, const me_motion_gate_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (p)
    if (const char* why = me_motion_gate_check(p)) {
      v->env.err = std::string("me_vo_loop_set_motion_gate: ") + why;
      return ME_ERR_INVALID;
    }
  if (started(v, "me_vo_loop_set_motion_gate: the rigid-motion gate is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  v->front.gate = p != nullptr;
  if (p) v->front.gate_params = *p;
  return ME_OK;
}

int me_vo_loop_set_klt_predict(me_vo_loop* v, int on) {
  if (!v) return ME_ERR_INVALID;
  if (on != 0 && on != 1) {
    v->env.err = "me_vo_loop_set_klt_predict: on must be 0 or 1";
    return ME_ERR_INVALID;
  }
  if (started(v, "me_vo_loop_set_klt_predict: guided tracking is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  v->klt_predict = on == 1;
  return ME_OK;
}

int me_vo_loop_set_covariance(me_vo_loop* v, const me_vo_cov_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (started(v, "me_vo_loop_set_covariance: the window covariance is set before the first frame")) return ME_ERR_STATE;
  v->cov_mode = p ? (p->landmarks ? 2 : 1) : 0;
  return ME_OK;
}

int me_vo_loop_set_track_check(me_vo_loop* v, const me_ba_point_check_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (p)
    if (const char* why = me_ba_point_check_check(p)) {
      v->env.err = std::string("me_vo_loop_set_track_check: ") + why;
      return ME_ERR_INVALID;
    }
  if (started(v, "me_vo_loop_set_track_check: the residual check is set before the first frame")) return ME_ERR_STATE;
  v->track_check = p != nullptr;
  if (p) v->check_params = *p;
  return ME_OK;
}

int me_vo_loop_flagged(me_vo_loop* v, int32_t* ts, int64_t* ids, uint8_t* flags, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->flagged.size();
  for (int i = 0; i < std::min(cap, *n); ++i) {
    if (ts) ts[i] = v->flagged[(size_t)i].t;
    if (ids) ids[i] = v->flagged[(size_t)i].id;
    if (flags) flags[i] = v->flagged[(size_t)i].flags;
  }
  return ME_OK;
}

int me_vo_loop_pose_covs(me_vo_loop* v, int32_t* ts, double* cov36, uint8_t* ok, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->pose_cov.size();
  int i = 0;
  for (auto& kv : v->pose_cov) {
    if (i >= cap) break;
    if (ts) ts[i] = kv.first;
    if (cov36) std::memcpy(cov36 + 36 * (size_t)i, kv.second.data(), 36 * sizeof(double));
    if (ok) ok[i] = kv.second[36] != 0.0;
    ++i;
  }
  return ME_OK;
}

int me_vo_loop_track_covs(me_vo_loop* v, int64_t* ids, double* cov9, uint8_t* ok, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->tab.size();
  const int m = std::min(cap, *n);
  for (int i = 0; i < m; ++i) {
    const auto it = v->track_cov.find(v->tab.ids[i]);
    const bool have = it != v->track_cov.end();
    if (ids) ids[i] = v->tab.ids[i];
    if (cov9)
      for (int q = 0; q < 9; ++q) cov9[9 * (size_t)i + q] = have ? it->second[q] : 0.0;
    if (ok) ok[i] = have && it->second[9] != 0.0;
  }
  return ME_OK;
}

int me_vo_loop_set_rectify(me_vo_loop* v, const me_camera_model* left, const me_camera_model* right, int border) {
  if (!v) return ME_ERR_INVALID;
  if ((left == nullptr) != (right == nullptr)) {
    v->env.err = "me_vo_loop_set_rectify: left and right are both models or both NULL";
    return ME_ERR_INVALID;
  }
  if (left && (border < 0 || border > 255)) {
    v->env.err = "me_vo_loop_set_rectify: border must be in 0..255";
    return ME_ERR_INVALID;
  }
  if (started(v, "me_vo_loop_set_rectify: rectification is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  me_range range_("me_vo_loop_set_rectify");
  if (!left) {
    v->images.rectify_off();
    return ME_OK;
  }
  const int rc = v->images.rectify_on(left, right, border);
  if (rc != ME_OK) v->images.rectify_off();
  return rc;
}

int me_vo_loop_set_equalise(me_vo_loop* v, const me_clahe_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (started(v, "me_vo_loop_set_equalise: equalisation is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  v->images.equalise = false;
  if (!p) return ME_OK;
  if (const char* why = me_clahe_check(p, v->env.cfg.width, v->env.cfg.height)) {
    v->env.err = std::string("me_vo_loop_set_equalise: ") + why;
    return ME_ERR_INVALID;
  }
  v->images.eq_params = *p;
  v->images.equalise = true;
  return ME_OK;
}

int me_vo_loop_set_tonemap(me_vo_loop* v, const me_tonemap_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (started(v, "me_vo_loop_set_tonemap: the tone map is set before the first me_vo_loop_process"))
    return ME_ERR_STATE;
  v->images.tonemap_off();
  if (!p) return ME_OK;
  if (v->kf.kf_on) {
    v->env.err = "me_vo_loop_set_tonemap: the tone map together with keyframe selection is not supported";
    return ME_ERR_INVALID;
  }
  if (const char* why = me_tonemap_check(p)) {
    v->env.err = std::string("me_vo_loop_set_tonemap: ") + why;
    return ME_ERR_INVALID;
  }
  const int rc = v->images.tonemap_on(p);
  if (rc != ME_OK) v->images.tonemap_off();
  return rc;
}

int me_vo_loop_set_keyframe_select(me_vo_loop* v, const me_kf_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (p) {
    if (const char* why = me_kf_check(p)) {
      v->env.err = std::string("me_vo_loop_set_keyframe_select: ") + why;
      return ME_ERR_INVALID;
    }
    if (v->images.tonemap) {
      v->env.err = "me_vo_loop_set_keyframe_select: keyframe selection together with the tone map is not supported";
      return ME_ERR_INVALID;
    }
  }
  if (started(v, "me_vo_loop_set_keyframe_select: keyframe selection is set before the first frame"))
    return ME_ERR_STATE;
  v->kf.kf_on = p != nullptr;
  if (p) v->kf.kf_params = *p;
  if (!p) v->kf.fpose = false;  // (the frame pose refines pushed frames: it goes with the switch it needs)
  return ME_OK;
}

int me_vo_loop_set_frame_pose(me_vo_loop* v, const me_frame_pose_params* p) {
  if (!v) return ME_ERR_INVALID;
  if (p) {
    if (const char* why = me_frame_pose_check(p)) {
      v->env.err = std::string("me_vo_loop_set_frame_pose: ") + why;
      return ME_ERR_INVALID;
    }
    if (!v->kf.kf_on) {
      v->env.err = "me_vo_loop_set_frame_pose: the frame pose needs me_vo_loop_set_keyframe_select first";
      return ME_ERR_INVALID;
    }
    if (!(std::isfinite(v->env.cfg.baseline) && v->env.cfg.baseline > 0.0)) {
      v->env.err = "me_vo_loop_set_frame_pose: baseline must be finite and > 0";
      return ME_ERR_INVALID;
    }
  }
  if (v->has_prev || v->n_pushed > 0) {
    v->env.err = "me_vo_loop_set_frame_pose: the frame pose is set before the first frame";
    return ME_ERR_INVALID;
  }
  v->kf.fpose = p != nullptr;
  if (p) v->kf.fpose_params = *p;
  return ME_OK;
}

int me_vo_loop_frame_poses(me_vo_loop* v, me_vo_frame_pose* out, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->kf.fposes.size();
  if (out)
    for (int i = 0; i < std::min(cap, *n); ++i) out[i] = v->kf.fposes[(size_t)i];
  return ME_OK;
}

int me_vo_loop_push(me_vo_loop* v, const uint8_t* left, const uint8_t* right, me_mem mem, int* keyframe_t) {
  if (!v || !left || !right || !keyframe_t) return ME_ERR_INVALID;
  *keyframe_t = -1;
  if (!v->kf.kf_on) {
    v->env.err = "me_vo_loop_push: camera frames need me_vo_loop_set_keyframe_select";
    return ME_ERR_STATE;
  }
  if (const int rc = enter(v, "me_vo_loop_push", true, 0, 8)) return rc;
  me_range range_("me_vo_loop_push");
  const int rc = v->push(left, right, mem, keyframe_t);
  if (rc != ME_OK) v->failed = true;
  return rc;
}

int me_vo_loop_process(me_vo_loop* v, int t, const uint8_t* left, const uint8_t* right, me_mem mem) {
  if (!v || !left || !right) return ME_ERR_INVALID;
  if (const int rc = enter(v, "me_vo_loop_process", false, t, 8)) return rc;
  me_range range_("me_vo_loop_process");
  const int rc = v->keyframe(t, left, right, mem, 8);
  if (rc != ME_OK) v->failed = true;  // the loop may have stopped half-way through a keyframe
  return rc;
}

int me_vo_loop_process16(me_vo_loop* v, int t, const uint16_t* left, const uint16_t* right, me_mem mem) {
  if (!v || !left || !right) return ME_ERR_INVALID;
  if (!v->images.tonemap) {
    v->env.err = "me_vo_loop_process16: 16-bit keyframes need me_vo_loop_set_tonemap";
    return ME_ERR_STATE;
  }
  if (const int rc = enter(v, "me_vo_loop_process16", false, t, 16)) return rc;
  me_range range_("me_vo_loop_process16");
  const int rc = v->keyframe(t, left, right, mem, 16);
  if (rc != ME_OK) v->failed = true;
  return rc;
}

int me_vo_loop_finish(me_vo_loop* v) {
  if (!v) return ME_ERR_INVALID;
  me_range range_("me_vo_loop_finish");
  return v->finish();
}

int me_vo_loop_results(me_vo_loop* v, me_vo_frame_result* out, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->results.size();
  if (out)
    for (int i = 0; i < std::min(cap, *n); ++i) out[i] = v->results[i];
  return ME_OK;
}

int me_vo_loop_events(me_vo_loop* v, me_vo_event* out, long cap, long* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (long)v->tab.events.size();
  if (out && cap > 0) std::memcpy(out, v->tab.events.data(), sizeof(me_vo_event) * (size_t)std::min(cap, *n));
  return ME_OK;
}

int me_vo_loop_tracks(me_vo_loop* v, int64_t* ids, double* X, uint8_t* active, int64_t* first, int64_t* last, int cap,
                      int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->tab.size();
  const int m = std::min(cap, *n);
  for (int i = 0; i < m; ++i) {
    if (ids) ids[i] = v->tab.ids[i];
    if (X)
      for (int q = 0; q < 3; ++q) X[3 * i + q] = v->tab.X[3 * (size_t)i + q];
    if (active) active[i] = v->tab.active[i];
    if (first) first[i] = v->tab.first[i];
    if (last) last[i] = v->tab.last[i];
  }
  return ME_OK;
}

int me_vo_loop_poses(me_vo_loop* v, int32_t* ts, double* poses, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->poses.size();
  int i = 0;
  for (auto& kv : v->poses) {
    if (i >= cap) break;
    if (ts) ts[i] = kv.first;
    if (poses)
      for (int q = 0; q < 6; ++q) poses[6 * i + q] = kv.second[q];
    ++i;
  }
  return ME_OK;
}

int me_vo_loop_frame_obs(me_vo_loop* v, int t, int64_t* ids, float* feats, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  auto it = v->tab.obs.find(t);
  if (it == v->tab.obs.end()) {
    *n = -1;
    return ME_OK;
  }
  *n = (int)it->second.ids.size();
  const int m = std::min(cap, *n);
  if (ids && m > 0) std::memcpy(ids, it->second.ids.data(), 8 * (size_t)m);
  if (feats && m > 0) std::memcpy(feats, it->second.feats.data(), 16 * (size_t)m);
  return ME_OK;
}

int me_vo_loop_frames(me_vo_loop* v, int32_t* ts, int cap, int* n) {
  if (!v || !n) return ME_ERR_INVALID;
  *n = (int)v->tab.obs.size();
  int i = 0;
  for (auto& kv : v->tab.obs) {
    if (i >= cap) break;
    if (ts) ts[i] = kv.first;
    ++i;
  }
  return ME_OK;
}

int me_vo_loop_stats(me_vo_loop* v, double* out, int n) {
  if (!v || !out) return ME_ERR_INVALID;
  const double s[9] = {v->host_s, v->env.wait_s, (double)v->tab.latest_id, v->env.wait_stage[0], v->env.wait_stage[1],
                       v->env.wait_stage[2], v->env.wait_stage[3], v->env.wait_stage[4], v->env.wait_stage[5]};
  for (int i = 0; i < std::min(n, 9); ++i) out[i] = s[i];
  return ME_OK;
}

}  // extern "C"
