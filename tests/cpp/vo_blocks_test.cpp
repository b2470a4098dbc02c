// Host test of the VO loop's block layouts and pair-pool rule
// (uasl_motion_estimation_amd/csrc/vo_blocks.hpp).  The expected offsets are written out here as the byte
// arithmetic the loop used before the header existed, not read from the header.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../uasl_motion_estimation_amd/csrc/vo_blocks.hpp"

namespace {

int failures = 0;
std::vector<uint8_t> arena(1 << 17);

#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// byte offset of an accessor's pointer over the arena
template <class T>
size_t off(T* p) {
  return (size_t)(reinterpret_cast<uint8_t*>(p) - arena.data());
}

void layouts(size_t n) {
  void* b = arena.data();
  const size_t m = n;
  {
    const me_vo::Res r{n};
    CHECK(off(r.uv(b)) == 0 && off(r.xr(b)) == 8 * n && off(r.status(b)) == 12 * n && off(r.ok(b)) == 13 * n);
    CHECK(r.o_xr() == 8 * n && r.o_status() == 12 * n && r.o_ok() == 13 * n && r.size() == 14 * n);
    CHECK(r.o_new_mirror() == 16 * ((14 * n + 15) / 16));
  }
  {
    const me_vo::NewFeats f{m};
    CHECK(off(f.count(b)) == 0 && off(f.uv(b)) == 16 && off(f.xr(b)) == 16 + 8 * m);
    CHECK(off(f.lo(b)) == 16 + 12 * m && off(f.ok(b)) == 16 + 16 * m && f.size() == 16 + 17 * m);
    CHECK(f.o_uv() == 16 && f.o_xr() == 16 + 8 * m && f.o_lo() == 16 + 12 * m && f.o_ok() == 16 + 16 * m);
  }
  {
    const me_vo::FirstMatch f{n};
    CHECK(off(f.uv(b)) == 0 && off(f.lo(b)) == 8 * n && off(f.xr(b)) == 12 * n && off(f.ok(b)) == 16 * n);
    CHECK(f.size() == 17 * n);
  }
  for (int guided = 0; guided < 2; ++guided)
    for (int gated = 0; gated < 2; ++gated) {
      const me_vo::KltIn k{n, guided == 1, gated == 1};
      CHECK(off(k.pts(b)) == 0 && off(k.xr(b)) == (guided ? 16 : 8) * n && k.o_xr() == (guided ? 16 : 8) * n);
      CHECK(guided ? off(k.guess(b)) == 8 * n : k.guess(b) == nullptr);
      CHECK(k.size() == (guided ? 16 : 8) * n + (gated ? 4 : 0) * n);
    }
  {
    const me_vo::Kf k{n, false};
    CHECK(off(k.ref(b)) == 0 && off(k.cur(b)) == 8 * n && off(k.nw(b)) == 16 * n);
    CHECK(off(k.alive(b)) == 24 * n && off(k.status(b)) == 25 * n);
    CHECK(off(k.info(b)) == 16 * ((26 * n + 15) / 16) && k.info_bytes() == 32);
    CHECK(k.o_cur() == 8 * n && k.o_new() == 16 * n && k.o_alive() == 24 * n && k.o_status() == 25 * n);
    CHECK(k.size() == 16 * ((26 * n + 15) / 16) + 32);
  }
  {
    const me_vo::Kf k{n, true};
    CHECK(off(k.ref(b)) == 0 && off(k.cur(b)) == 8 * n && off(k.nw(b)) == 16 * n && off(k.ref_xr(b)) == 24 * n);
    CHECK(off(k.alive(b)) == 28 * n && off(k.status(b)) == 29 * n);
    CHECK(off(k.info(b)) == 16 * ((30 * n + 15) / 16) && k.info_bytes() == 160);
    CHECK(off(k.pose_block(b)) == 16 * ((30 * n + 15) / 16) + 32);
    CHECK(k.size() == 16 * ((30 * n + 15) / 16) + 160);
  }
  {  // the window store of capacity n, element e (wview and the compaction / per-frame copies of window_add)
    const me_vo::WStore w{n};
    const size_t cap = n;
    CHECK(w.size() == 40 * cap && w.o_frame() == 32 * cap && w.o_id() == 36 * cap);
    CHECK(off(w.obs(b)) == 0 && off(w.frame(b)) == 32 * cap && off(w.id(b)) == 36 * cap);
    for (size_t e : {(size_t)0, n / 2, n})
      CHECK(off(w.obs(b, e)) == 32 * e && off(w.frame(b, e)) == 32 * cap + 4 * e && off(w.id(b, e)) == 36 * cap + 4 * e);
  }
  for (size_t nc : {(size_t)1, (size_t)3, (size_t)50}) {  // the BA upload block of nc cameras and n points
    const me_vo::BaUpload u{nc, n};
    const size_t npts = n, o_ids = 48 * nc + 24 * npts, o_cs = o_ids + 4 * npts, nb = o_cs + 4 * nc;
    CHECK(off(u.cams(b)) == 0 && off(u.pts(b)) == 48 * nc && off(u.ids(b)) == o_ids && off(u.cam_src(b)) == o_cs);
    CHECK(u.o_pts() == 48 * nc && u.o_ids() == o_ids && u.o_cam_src() == o_cs && u.size() == nb);
    CHECK(u.size() == 48 * nc + 24 * npts + 4 * npts + 4 * nc);  // (reserve)
    CHECK(u.stage_bytes(true) == nb && u.stage_bytes(false) == o_cs);
  }
}

// The host decode of the new-feature block: the first count features, the count clamped to [0, m]
void decode() {
  const me_vo::NewFeats f{5};
  void* b = arena.data();
  for (size_t i = 0; i < 10; ++i) f.uv(b)[i] = (float)i;
  for (size_t i = 0; i < 5; ++i) {
    f.xr(b)[i] = 100.0f + i;
    f.ok(b)[i] = (uint8_t)(i & 1);
  }
  const int counts[4] = {-3, 0, 3, 9}, want[4] = {0, 0, 3, 5};
  for (int c = 0; c < 4; ++c) {
    *f.count(b) = counts[c];
    std::vector<float> uv, xr;
    std::vector<uint8_t> ok;
    f.decode(b, uv, xr, ok);
    const size_t k = (size_t)want[c];
    CHECK(uv.size() == 2 * k && xr.size() == k && ok.size() == k);
    for (size_t i = 0; i < k && i < xr.size(); ++i)
      CHECK(uv[2 * i] == (float)(2 * i) && uv[2 * i + 1] == (float)(2 * i + 1) && xr[i] == 100.0f + i && ok[i] == (i & 1));
  }
}

// 10 000 frames: keyframes decided at random, or every frame one (the loop of me_vo_loop_process)
void pool(bool all_keyframes) {
  std::mt19937 rng(20240611u);
  int prev = -1, kf[2] = {-1, -1};
  for (int t = 0; t < 10000; ++t) {
    const int s = me_vo::pool_pick(prev, kf[0], kf[1]);
    CHECK(s >= 0 && s < me_vo::kPoolSlots && s < 4);
    CHECK(s != prev && s != kf[0] && s != kf[1]);
    if (all_keyframes) CHECK(s == t % 3);
    if (all_keyframes || t == 0 || (rng() & 3) == 0) {  // a keyframe (the first frame always is)
      kf[1] = kf[0];
      kf[0] = s;
      prev = -1;
    } else {
      prev = s;
    }
  }
}

}  // namespace

int main() {
  for (size_t n : {0, 1, 2, 15, 16, 17, 2000}) layouts(n);
  decode();
  pool(false);
  pool(true);
  if (failures) {
    std::fprintf(stderr, "vo_blocks_test: %d failures\n", failures);
    return 1;
  }
  std::printf("vo_blocks_test: ok\n");
  return 0;
}
