// vo_loop_keyframe.hpp -- the VO loop's keyframe selection and frame pose state (vo_loop.cpp; me_vo_loop_push,
// me_hip.h A12i / A12j): the features seeded at the last keyframe in device block "kf" (me_vo::Kf), tracked
// through every pushed frame.  me_vo_loop::push, which decides what a frame becomes, stays in the loop: it
// needs the image chain and process() as well.
#pragma once
#include <cstring>
#include <vector>

#include "vo_blocks.hpp"
#include "vo_loop_env.hpp"
#include "vo_loop_front.hpp"
#include "vo_math.hpp"

namespace me_vo {

struct KeyframeState {
  Env& env;
  explicit KeyframeState(Env& e) : env(e) {}
  bool kf_on = false;
  me_kf_params kf_params{};
  int kf_n = 0, kf_gap = 0;   // seeded features; frames pushed since the last keyframe
  std::vector<float> kf_ref;  // the seeded features' positions in the last keyframe
  // the frame pose (me_vo_loop_set_frame_pose): me_vo::Kf with the pose block
  bool fpose = false;
  me_frame_pose_params fpose_params{};
  std::vector<me_vo_frame_pose> fposes;  // per pushed frame after the first

  // The state seeded from a keyframe's active tracks: their left positions (ref, in the order the next
  // klt_submit uploads them: TrackTable::seeded) and, with the frame pose, their x_r
  int kf_seed(const std::vector<float>& ref, const std::vector<float>& xr) {
    kf_ref = ref;
    kf_n = (int)(kf_ref.size() / 2);
    kf_gap = 0;
    const Kf kf{(size_t)kf_n, fpose};
    void *hp, *d;
    VL_TRY(env.dbuf("kf", kf.size(), &d), "kf");
    // one copy.  With the frame pose the whole block: x_r rides beside the positions, the pose block behind the
    // info block is zeroed (valid = 0: the first frame after the keyframe starts at identity).  Without it up to
    // alive: new_uv's bytes ride along, the tracker writes them before they are read
    const size_t total = fpose ? kf.size() : kf.o_status();
    if (total == 0) return ME_OK;
    VL_TRY(env.hbuf("kf_in", total, &hp), "kf");
    if (fpose) std::memset(hp, 0, total);
    std::memcpy(kf.ref(hp), kf_ref.data(), 8 * kf.n);
    std::memcpy(kf.cur(hp), kf_ref.data(), 8 * kf.n);
    if (fpose) std::memcpy(kf.ref_xr(hp), xr.data(), 4 * kf.n);
    std::memset(kf.alive(hp), 1, kf.n);
    VL_TRY(me_memcpy_async(env.tctx, d, hp, total), "kf H2D");
    return ME_OK;
  }
  // One pushed frame: the loop's tracker (not guided) pv -> cur at cur_uv, me_kf_update behind it, the info block back
  int kf_track(const Imgs& pv, const Imgs& cur, unsigned char* info_out) {
    const me_vo_loop_config& cfg = env.cfg;
    me_ctx* tctx = env.tctx;
    const Kf kf{(size_t)kf_n, fpose};
    const int n = kf_n;
    void *d, *ho;
    VL_TRY(env.dbuf("kf", kf.size(), &d), "kf");  // (sized by the seed: it does not grow here)
    if (n)
      if (const int rc = track(env, pv, cur, kf.cur(d), nullptr, kf.nw(d), kf.status(d), n)) return rc;
    VL_TRY(me_kf_update(tctx, n ? kf.ref(d) : nullptr, n ? kf.cur(d) : nullptr, n ? kf.alive(d) : nullptr,
                        n ? kf.nw(d) : nullptr, n ? kf.status(d) : nullptr, n, cfg.width, cfg.height, (float)kMargin,
                        kf_gap, &kf_params, kf.info(d)),
           "me_kf_update");
    if (fpose)  // right behind the update, from the previous frame's pose (start == info)
      VL_TRY(me_frame_pose(tctx, n ? kf.ref(d) : nullptr, n ? kf.ref_xr(d) : nullptr, n ? kf.cur(d) : nullptr,
                           n ? kf.alive(d) : nullptr, n, cfg.K[0], cfg.K[2], cfg.K[5], cfg.baseline, &fpose_params,
                           kf.pose_block(d), nullptr, kf.pose_block(d)),
             "me_frame_pose");
    VL_TRY(env.hbuf("kf_out", kf.info_bytes(), &ho), "kf");
    VL_TRY(me_memcpy_async(tctx, ho, kf.info(d), kf.info_bytes()), "kf D2H");
    VL_TRY(me_synchronize(tctx), "kf_track");
    std::memcpy(info_out, ho, kf.info_bytes());
    return ME_OK;
  }
  // The keyframe tracker's guess: cur_uv of the alive features, the keyframe's positions of the others
  int kf_read_guess(std::vector<float>& guess) {
    const Kf kf{(size_t)kf_n, fpose};
    void *d, *ho;
    VL_TRY(env.dbuf("kf", kf.size(), &d), "kf");
    const size_t nb = kf.o_status() - kf.o_cur();  // cur_uv | new_uv | (ref_xr |) alive
    VL_TRY(env.hbuf("kf_state", nb, &ho), "kf");
    VL_TRY(me_memcpy_async(env.tctx, ho, kf.cur(d), nb), "kf D2H");
    VL_TRY(me_synchronize(env.tctx), "kf_guess");
    const float* cu = (const float*)ho;
    const uint8_t* al = (const uint8_t*)ho + (kf.o_alive() - kf.o_cur());
    guess.resize(2 * kf.n);
    for (size_t k = 0; k < kf.n; ++k) {
      guess[2 * k] = al[k] ? cu[2 * k] : kf_ref[2 * k];
      guess[2 * k + 1] = al[k] ? cu[2 * k + 1] : kf_ref[2 * k + 1];
    }
    return ME_OK;
  }
  // The frame pose record of a pushed frame from its info block: relative to the keyframe the state was seeded
  // from (t_ref); frame: its number among the pushed frames; t: the keyframe it became, or -1
  void record_pose(const unsigned char* info, int32_t frame, int t, int t_ref) {
    me_vo_frame_pose r{};
    int32_t w[5];
    std::memcpy(w, info + 32, 20);
    r.frame = frame;
    r.t = t;
    r.t_ref = t_ref;
    r.gap = kf_gap;
    r.n_usable = w[0];
    r.n_inliers = w[2];
    r.steps = w[3];
    r.valid = w[4];
    std::memcpy(r.R, info + 64, 72);
    std::memcpy(r.t_rel, info + 64 + 72, 24);
    fposes.push_back(r);
  }
};

}  // namespace me_vo
