// vo_loop_images.hpp -- the VO loop's image chain (vo_loop.cpp): the pair pool and its slots, the chain's
// intermediates, and the rectify / equalise / tone-map switches with their state.
#pragma once
#include "vo_blocks.hpp"
#include "vo_loop_env.hpp"

namespace me_vo {

struct ImageChain {
  Env& env;
  explicit ImageChain(Env& e) : env(e) {}
  // the pair pool (me_vo::pool_pick): 8-bit pairs of width x height x 2 bytes that the image chain's last stage
  // writes, allocated on first use; the slots of the previous pushed frame (-1: a keyframe) and the last two
  // keyframes, and the previous pushed frame's pair (while slot_prev >= 0)
  void* pool[kPoolSlots] = {nullptr, nullptr, nullptr, nullptr};
  int slot_prev = -1, slot_kf[2] = {-1, -1};
  Imgs push_imgs;
  // the chain's intermediates, single buffers allocated on first use and reused in stream order: host images
  // that a tone map or a remap reads are uploaded into stage_in, the tone map ahead of a remap writes stage_tm
  void *stage_in = nullptr, *stage_tm = nullptr;
  // ---- rectification (me_vo_loop_set_rectify): the two maps and the raw sizes
  bool rectify = false;
  int rect_border = 0;
  int raw_w[2] = {0, 0}, raw_h[2] = {0, 0};
  void* rect_map[2] = {nullptr, nullptr};
  // ---- equalisation (me_vo_loop_set_equalise)
  bool equalise = false;
  me_clahe_params eq_params{};
  // ---- 16-bit ingest (me_vo_loop_set_tonemap): the parameters and a state per camera
  bool tonemap = false;
  me_tonemap_params tm_params{};
  me_tonemap_state* tm_state[2] = {nullptr, nullptr};

  void rectify_off() {
    for (auto& p : rect_map) {
      if (p) me_free(env.tctx, p);
      p = nullptr;
    }
    rectify = false;
  }
  // The maps of the two cameras, built once on the front context; the rectified model is the loop's own
  int rectify_on(const me_camera_model* left, const me_camera_model* right, int border) {
    rectify_off();
    const me_vo_loop_config& cfg = env.cfg;
    const me_rectified_model rm{cfg.width, cfg.height, cfg.K[0], cfg.K[4], cfg.K[2], cfg.K[5]};
    const me_camera_model* cam[2] = {left, right};
    const size_t npx = (size_t)cfg.width * cfg.height;
    for (int k = 0; k < 2; ++k) {
      VL_TRY(me_malloc(env.tctx, &rect_map[k], 8 * npx), "malloc");
      VL_TRY(me_rectify_map(env.tctx, ME_DEVICE, cam[k], &rm, (int32_t*)rect_map[k]), "me_vo_loop_set_rectify");
      raw_w[k] = cam[k]->width;
      raw_h[k] = cam[k]->height;
    }
    VL_TRY(me_synchronize(env.tctx), "me_vo_loop_set_rectify");
    rect_border = border;
    rectify = true;
    return ME_OK;
  }
  void tonemap_off() {
    for (auto& st : tm_state) {
      if (st) me_tonemap_state_destroy(st);
      st = nullptr;
    }
    tonemap = false;
  }
  int tonemap_on(const me_tonemap_params* p) {
    tonemap_off();
    for (auto& st : tm_state) VL_TRY(me_tonemap_state_create(env.tctx, &st), "me_tonemap_state_create");
    tm_params = *p;
    tonemap = true;
    return ME_OK;
  }
  void close() {
    for (void** p : {&pool[0], &pool[1], &pool[2], &pool[3], &stage_in, &stage_tm}) {
      if (*p) me_free(env.tctx, *p);
      *p = nullptr;
    }
    rectify_off();
    tonemap_off();
  }

  // The slot of the next frame's pair; keyframes only (pushed = false): t % 3
  int pick(bool pushed) const { return pool_pick(pushed ? slot_prev : -1, slot_kf[0], slot_kf[1]); }
  // A keyframe took pool slot `slot`: it is held for this keyframe and the next
  void hold_keyframe(int slot) {
    slot_kf[1] = slot_kf[0];
    slot_kf[0] = slot;
    slot_prev = -1;
  }

  // The image chain of every frame entry, queued on the front-end stream ahead of the tracker: bring to the
  // device -> me_tonemap16 (depth 16) -> two me_remap_q5 -> two me_clahe, each stage only with its switch.  The
  // last of the first three that runs writes pool[slot], earlier ones the intermediates; CLAHE then runs in place
  // there, or out of place from the caller's device images, which are never written.  With no stage at all the
  // caller's device pair is used as it is, unless the result must be the loop's (owned: me_vo_loop_push), then
  // it is copied.  Sizes ahead of the remap are the camera models', the loop's otherwise.
  int prepare(const void* L, const void* R, me_mem mem, int bits, bool owned, int slot, Imgs& im) {
    const me_vo_loop_config& cfg = env.cfg;
    me_ctx* tctx = env.tctx;
    const bool wide = bits == 16, host = mem != ME_DEVICE;
    const uint8_t *sl = (const uint8_t*)L, *sr = (const uint8_t*)R;  // the pair so far
    if (!(host || wide || rectify || equalise || owned)) {
      im = Imgs{sl, sr};
      return ME_OK;
    }
    const size_t npx = (size_t)cfg.width * cfg.height;
    if (pool[slot] == nullptr) VL_TRY(me_malloc(tctx, &pool[slot], 2 * npx), "malloc");
    uint8_t *oL = (uint8_t*)pool[slot], *oR = oL + npx;
    const int w[2] = {rectify ? raw_w[0] : cfg.width, rectify ? raw_w[1] : cfg.width};
    const int h[2] = {rectify ? raw_h[0] : cfg.height, rectify ? raw_h[1] : cfg.height};
    const size_t nl = (size_t)w[0] * h[0], nr = (size_t)w[1] * h[1], px = wide ? 2 : 1;
    if (host || !(wide || rectify || equalise)) {
      uint8_t *dl = oL, *dr = oR;
      if (wide || rectify) {
        if (stage_in == nullptr) VL_TRY(me_malloc(tctx, &stage_in, px * (nl + nr) + 16), "malloc");
        dl = (uint8_t*)stage_in;
        dr = dl + (wide ? align16(2 * nl) : nl);
      }
      VL_TRY(me_memcpy_async(tctx, dl, sl, px * nl), "image upload");
      VL_TRY(me_memcpy_async(tctx, dr, sr, px * nr), "image upload");
      sl = dl;
      sr = dr;
    }
    if (wide) {
      uint8_t *dl = oL, *dr = oR;
      if (rectify) {
        if (stage_tm == nullptr) VL_TRY(me_malloc(tctx, &stage_tm, nl + nr + 16), "malloc");
        dl = (uint8_t*)stage_tm;
        dr = dl + align16(nl);
      }
      VL_TRY(me_tonemap16(tctx, ME_DEVICE, (const uint16_t*)sl, w[0], h[0], w[0], dl, w[0], &tm_params, tm_state[0]),
             "me_tonemap16");
      VL_TRY(me_tonemap16(tctx, ME_DEVICE, (const uint16_t*)sr, w[1], h[1], w[1], dr, w[1], &tm_params, tm_state[1]),
             "me_tonemap16");
      sl = dl;
      sr = dr;
    }
    if (rectify) {
      VL_TRY(me_remap_q5(tctx, ME_DEVICE, sl, w[0], h[0], w[0], (const int32_t*)rect_map[0], cfg.width, cfg.height,
                         rect_border, oL, cfg.width, nullptr),
             "me_remap_q5");
      VL_TRY(me_remap_q5(tctx, ME_DEVICE, sr, w[1], h[1], w[1], (const int32_t*)rect_map[1], cfg.width, cfg.height,
                         rect_border, oR, cfg.width, nullptr),
             "me_remap_q5");
      sl = oL;
      sr = oR;
    }
    if (equalise) {  // (sl == oL: in place)
      VL_TRY(me_clahe(tctx, ME_DEVICE, sl, cfg.width, cfg.height, cfg.width, &eq_params, oL, cfg.width, nullptr), "me_clahe");
      VL_TRY(me_clahe(tctx, ME_DEVICE, sr, cfg.width, cfg.height, cfg.width, &eq_params, oR, cfg.width, nullptr), "me_clahe");
    }
    im = Imgs{oL, oR};
    return ME_OK;
  }
};

}  // namespace me_vo
