// vo_loop_front.hpp -- the VO loop's front-end calls (vo_loop.cpp): the tracker, the epipolar MI matchers, the
// rigid-motion gate and the new features of a keyframe, each one submission on the front context with one
// round trip.  Its own state: the grid of feature cells and the matcher / gate switches.
#pragma once
#include <cstring>
#include <vector>

#include "vo_blocks.hpp"
#include "vo_loop_env.hpp"
#include "vo_math.hpp"

namespace me_vo {

// The loop's tracker call (a free function: the keyframe state of vo_loop_keyframe.hpp tracks with it too): the
// guided tracker when there is a guess, and with cfg.klt_fb_max > 0 the forward-backward form, whose combined
// status is the byte the matcher gates on
inline int track(Env& env, const Imgs& prev, const Imgs& cur, const float* pts, const float* guess, float* out,
                 uint8_t* status, int n) {
  me_klt_params kp;
  me_klt_default_params(&kp);
  me_ctx* tctx = env.tctx;
  const int w = env.cfg.width, h = env.cfg.height;
  const double fb = env.cfg.klt_fb_max;
  if (guess && fb > 0.0)
    VL_TRY(me_klt_track_guided_fb(tctx, ME_DEVICE, prev.L, cur.L, w, h, w, pts, guess, out, status, nullptr, n, &kp, fb),
           "me_klt_track_guided_fb");
  else if (guess)
    VL_TRY(me_klt_track_guided(tctx, ME_DEVICE, prev.L, cur.L, w, h, w, pts, guess, out, status, n, &kp),
           "me_klt_track_guided");
  else if (fb > 0.0)
    VL_TRY(me_klt_track_fb(tctx, ME_DEVICE, prev.L, cur.L, w, h, w, pts, out, status, nullptr, n, &kp, fb),
           "me_klt_track_fb");
  else
    VL_TRY(me_klt_track(tctx, ME_DEVICE, prev.L, cur.L, w, h, w, pts, out, status, n, &kp), "me_klt_track");
  return ME_OK;
}

struct FrontEnd {
  Env& env;
  explicit FrontEnd(Env& e) : env(e) {}
  Grid grid;              // make_grid of the configuration (the loop's init)
  double match_lr = 0.0;  // > 0: every matcher call takes its _lr form with this bound (me_vo_loop_set_match_lr)
  // the rigid-motion gate (me_vo_loop_set_motion_gate, me_hip.h A12h): queued behind the tracked features' matcher
  bool gate = false;
  me_motion_gate_params gate_params{};

  // guess (klt_predict): the features' predicted pixels, uploaded behind them in the same copy; prev_xr (the
  // rigid-motion gate): the previous keyframe's x_r, behind both
  int klt_submit(const Imgs& prev, const Imgs& cur, const KltIn& in, const std::vector<float>& pts,
                 const std::vector<float>* guess, const std::vector<float>* prev_xr) {
    const Res res{in.n};
    void *hp, *d_in, *dres;
    VL_TRY(env.hbuf("klt_in", in.size(), &hp), "klt");
    std::memcpy(in.pts(hp), pts.data(), 8 * in.n);
    if (guess) std::memcpy(in.guess(hp), guess->data(), 8 * in.n);
    if (prev_xr) std::memcpy(in.xr(hp), prev_xr->data(), 4 * in.n);
    VL_TRY(env.dbuf("klt_in", in.size(), &d_in), "klt");
    VL_TRY(env.dbuf("res", res.size(), &dres), "klt");
    VL_TRY(me_memcpy_async(env.tctx, d_in, hp, in.size()), "klt H2D");
    return track(env, prev, cur, in.pts(d_in), in.guess(d_in), res.uv(dres), res.status(dres), (int)in.n);
  }
  // The loop's matcher calls: the plain entry points, or their left-right forms (me_hip.h A2b) when match_lr > 0
  int epi_match(const Imgs& im, const float* uv, const int32_t* lo, const uint8_t* valid, const uint8_t* status, int n,
                int nd, int unique, float* xr, uint8_t* ok) {
    const me_vo_loop_config& cfg = env.cfg;
    if (match_lr > 0.0)
      return me_mi_epipolar_match_lr(env.tctx, im.L, im.R, cfg.width, cfg.height, cfg.width, uv, lo, valid, status, n, nd,
                                     kPatch, cfg.d_max, unique, kRatio, (float)kMargin, match_lr, xr, ok, nullptr);
    return me_mi_epipolar_match(env.tctx, im.L, im.R, cfg.width, cfg.height, cfg.width, uv, lo, valid, status, n, nd,
                                kPatch, cfg.d_max, unique, kRatio, (float)kMargin, xr, ok);
  }
  int epi_match_count(const Imgs& im, const float* uv, const int32_t* lo, const int32_t* n_dev, int n_max, int nd,
                      float* xr, uint8_t* ok) {
    const me_vo_loop_config& cfg = env.cfg;
    if (match_lr > 0.0)
      return me_mi_epipolar_match_lr_count(env.tctx, im.L, im.R, cfg.width, cfg.height, cfg.width, uv, lo, n_dev, n_max,
                                           nd, kPatch, cfg.d_max, 1, kRatio, (float)kMargin, match_lr, xr, ok,
                                           nullptr);
    return me_mi_epipolar_match_count(env.tctx, im.L, im.R, cfg.width, cfg.height, cfg.width, uv, lo, n_dev, n_max, nd,
                                      kPatch, cfg.d_max, 1, kRatio, (float)kMargin, xr, ok);
  }
  // The new features of a keyframe, queued on the front end into block "new": the corner detector or the
  // grid's empty cells, given the n tracked features in block "res" (n = 0: none), then their matcher
  int new_features(const Imgs& im, void* dres, int n, int t, int nd_new, const NewFeats& nf, void* dn) {
    const me_vo_loop_config& cfg = env.cfg;
    const Res res{(size_t)n};
    const float* uv = n ? res.uv(dres) : nullptr;
    const uint8_t *st = n ? res.status(dres) : nullptr, *ok = n ? res.ok(dres) : nullptr;
    if (cfg.detector == 1) {
      const me_corner_params cp{cfg.corner_win, cfg.corner_min_eig};
      VL_TRY(me_vo_new_corners(env.tctx, im.L, cfg.width, cfg.height, cfg.width, uv, st, ok, n, (float)kMargin, grid.nx,
                               grid.ny, grid.cw, grid.ch, cfg.n_feats, cfg.d_min, &cp, nf.uv(dn), nf.lo(dn), nf.count(dn)),
             "me_vo_new_corners");
    } else {
      VL_TRY(me_vo_new_cells(env.tctx, uv, st, ok, n, cfg.width, cfg.height, (float)kMargin, grid.nx, grid.ny, grid.cw,
                             grid.ch, cfg.n_feats, t, cfg.d_min, nf.uv(dn), nf.lo(dn), nf.count(dn)),
             "me_vo_new_cells");
    }
    VL_TRY(epi_match_count(im, nf.uv(dn), nf.lo(dn), nf.count(dn), (int)nf.m, nd_new, nf.xr(dn), nf.ok(dn)),
           "me_mi_epipolar_match_count");
    return ME_OK;
  }
  // GPUBackend.klt_match_new: tracked features' matcher, the cells they leave
  // empty, the new features' matcher -- one submission, one round trip
  int klt_match_new(const KltIn& in, const Imgs& im, const std::vector<int32_t>& lo, const std::vector<uint8_t>& dvalid,
                    int t, int nd, int nd_new, std::vector<float>& uv, std::vector<uint8_t>& st, std::vector<float>& xr,
                    std::vector<uint8_t>& ok, std::vector<float>& nuv, std::vector<float>& nxr, std::vector<uint8_t>& nok) {
    const me_vo_loop_config& cfg = env.cfg;
    me_ctx* tctx = env.tctx;
    const int n = (int)in.n;
    const Res res{in.n};
    const NewFeats nf{(size_t)std::max(cfg.n_feats, 1)};
    void *hp, *dl, *dres, *dn, *ho;
    VL_TRY(env.hbuf("lo", 5 * in.n, &hp), "match");
    std::memcpy(hp, lo.data(), 4 * in.n);
    std::memcpy((uint8_t*)hp + 4 * in.n, dvalid.data(), n);
    VL_TRY(env.dbuf("lo", 5 * in.n, &dl), "match");
    VL_TRY(me_memcpy_async(tctx, dl, hp, 5 * in.n), "match H2D");
    VL_TRY(env.dbuf("res", res.size(), &dres), "match");
    VL_TRY(epi_match(im, res.uv(dres), (const int32_t*)dl, (const uint8_t*)dl + 4 * in.n, res.status(dres), n, nd, 0,
                     res.xr(dres), res.ok(dres)),
           "me_mi_epipolar_match");
    if (gate) {  // in place on the ok byte the detector below and the host's good mask read
      void* d_in = env.dev["klt_in"].p;
      VL_TRY(me_motion_gate(tctx, in.pts(d_in), in.xr(d_in), res.uv(dres), res.xr(dres), res.status(dres), res.ok(dres),
                            n, cfg.K[0], cfg.K[2], cfg.K[5], cfg.baseline, cfg.width, cfg.height, (float)kMargin, t,
                            &gate_params, res.ok(dres), nullptr, nullptr),
             "me_motion_gate");
    }
    VL_TRY(env.dbuf("new", nf.size(), &dn), "match");
    if (const int rc = new_features(im, dres, n, t, nd_new, nf, dn)) return rc;
    const size_t o = res.o_new_mirror();
    VL_TRY(env.hbuf("out", o + nf.size(), &ho), "match");
    VL_TRY(me_memcpy_async(tctx, ho, dres, res.size()), "match D2H");
    VL_TRY(me_memcpy_async(tctx, (uint8_t*)ho + o, dn, nf.size()), "match D2H");
    VL_TRY(env.timed_wait(0, [&] { return me_synchronize(tctx); }), "klt_match_new");
    uv.assign(res.uv(ho), res.uv(ho) + 2 * in.n);
    xr.assign(res.xr(ho), res.xr(ho) + in.n);
    st.assign(res.status(ho), res.status(ho) + in.n);
    ok.assign(res.ok(ho), res.ok(ho) + in.n);
    nf.decode((uint8_t*)ho + o, nuv, nxr, nok);
    return ME_OK;
  }
  // A keyframe without tracked features under the corner detector: the detector and the new
  // features' matcher in one submission (klt_match_new without its tracked half)
  int corners_match(const Imgs& im, int nd_new, std::vector<float>& nuv, std::vector<float>& nxr,
                    std::vector<uint8_t>& nok) {
    const NewFeats nf{(size_t)std::max(env.cfg.n_feats, 1)};
    void *dn, *ho;
    VL_TRY(env.dbuf("new", nf.size(), &dn), "match");
    if (const int rc = new_features(im, nullptr, 0, 0, nd_new, nf, dn)) return rc;
    VL_TRY(env.hbuf("out", nf.size(), &ho), "match");
    VL_TRY(me_memcpy_async(env.tctx, ho, dn, nf.size()), "match D2H");
    VL_TRY(env.timed_wait(1, [&] { return me_synchronize(env.tctx); }), "corners_match");
    nf.decode(ho, nuv, nxr, nok);
    return ME_OK;
  }
  // GPUBackend.match: the first keyframe's new features (uniqueness test)
  int match(const Imgs& im, const std::vector<float>& uv, int nd, std::vector<float>& xr, std::vector<uint8_t>& ok) {
    const int n = (int)uv.size() / 2;
    xr.assign(n, 0.0f);
    ok.assign(n, 0);
    if (n == 0) return ME_OK;
    const FirstMatch fm{(size_t)n};
    void *hp, *d, *ho;
    VL_TRY(env.hbuf("m_in", fm.o_xr(), &hp), "match");  // (the uploaded part: uv | lo)
    std::memcpy(fm.uv(hp), uv.data(), 8 * fm.n);
    std::fill_n(fm.lo(hp), n, (int32_t)env.cfg.d_min);
    VL_TRY(env.dbuf("m", fm.size(), &d), "match");
    VL_TRY(me_memcpy_async(env.tctx, d, hp, fm.o_xr()), "match H2D");
    VL_TRY(epi_match(im, fm.uv(d), fm.lo(d), nullptr, nullptr, n, nd, 1, fm.xr(d), fm.ok(d)), "me_mi_epipolar_match");
    const size_t nb = fm.size() - fm.o_xr();  // (the part read back: x_r | ok)
    VL_TRY(env.hbuf("m_out", nb, &ho), "match");
    VL_TRY(me_memcpy_async(env.tctx, ho, fm.xr(d), nb), "match D2H");
    VL_TRY(env.timed_wait(1, [&] { return me_synchronize(env.tctx); }), "match");
    std::memcpy(xr.data(), ho, 4 * fm.n);
    std::memcpy(ok.data(), (uint8_t*)ho + (fm.o_ok() - fm.o_xr()), n);
    return ME_OK;
  }
};

}  // namespace me_vo
