// vo_blocks.hpp -- the VO loop's packed device blocks and its pair pool's slot rule (vo_loop.cpp).
//
// The loop keeps several arrays in one device buffer each, so that a stage costs one copy each way.  The kernels
// take separate pointers: the layouts are the loop's own, and every offset is defined here, once.  A layout is a
// small value made from its element counts; o_*() are byte offsets, the accessors type them over any base, the
// device buffer or its page-locked host mirror alike.  Host only, no HIP: tests/cpp/vo_blocks_test.cpp checks
// the numbers on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace me_vo {

inline size_t align16(size_t nbytes) { return 16 * ((nbytes + 15) / 16); }
template <class T>
T* at(void* base, size_t offset) {
  return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + offset);
}

// "res": the n tracked features of the keyframe in flight.  uv (8n) | x_r (4n) | status (n) | ok (n)
struct Res {
  size_t n;
  size_t o_xr() const { return 8 * n; }
  size_t o_status() const { return 12 * n; }
  size_t o_ok() const { return 13 * n; }
  size_t size() const { return 14 * n; }
  float* uv(void* b) const { return at<float>(b, 0); }
  float* xr(void* b) const { return at<float>(b, o_xr()); }
  uint8_t* status(void* b) const { return at<uint8_t>(b, o_status()); }
  uint8_t* ok(void* b) const { return at<uint8_t>(b, o_ok()); }
  // one host buffer mirrors "res" and "new": the new-feature block starts at the next 16-byte boundary
  size_t o_new_mirror() const { return align16(size()); }
};

// "new": up to m new features.  count (int32, 16 bytes kept) | uv (8m) | x_r (4m) | lo (4m) | ok (m)
struct NewFeats {
  size_t m;
  size_t o_uv() const { return 16; }
  size_t o_xr() const { return 16 + 8 * m; }
  size_t o_lo() const { return 16 + 12 * m; }
  size_t o_ok() const { return 16 + 16 * m; }
  size_t size() const { return 16 + 17 * m; }
  int32_t* count(void* b) const { return at<int32_t>(b, 0); }
  float* uv(void* b) const { return at<float>(b, o_uv()); }
  float* xr(void* b) const { return at<float>(b, o_xr()); }
  int32_t* lo(void* b) const { return at<int32_t>(b, o_lo()); }
  uint8_t* ok(void* b) const { return at<uint8_t>(b, o_ok()); }
  // the host mirror's first count features (the count clamped to [0, m])
  void decode(void* host, std::vector<float>& uv_out, std::vector<float>& xr_out, std::vector<uint8_t>& ok_out) const {
    const size_t k = (size_t)std::max<int64_t>(0, std::min<int64_t>(*count(host), (int64_t)m));
    uv_out.assign(uv(host), uv(host) + 2 * k);
    xr_out.assign(xr(host), xr(host) + k);
    ok_out.assign(ok(host), ok(host) + k);
  }
};

// "m": the first keyframe's n grid features.  uv (8n) | lo (4n), uploaded | x_r (4n) | ok (n), read back
struct FirstMatch {
  size_t n;
  size_t o_lo() const { return 8 * n; }
  size_t o_xr() const { return 12 * n; }
  size_t o_ok() const { return 16 * n; }
  size_t size() const { return 17 * n; }
  float* uv(void* b) const { return at<float>(b, 0); }
  int32_t* lo(void* b) const { return at<int32_t>(b, o_lo()); }
  float* xr(void* b) const { return at<float>(b, o_xr()); }
  uint8_t* ok(void* b) const { return at<uint8_t>(b, o_ok()); }
};

// "klt_in": the tracker's upload.  pts (8n) | guess (8n, guided only) | the previous keyframe's x_r (4n, gate only)
struct KltIn {
  size_t n;
  bool guided, gated;
  size_t o_guess() const { return 8 * n; }
  size_t o_xr() const { return (guided ? 16 : 8) * n; }
  size_t size() const { return o_xr() + (gated ? 4 : 0) * n; }
  float* pts(void* b) const { return at<float>(b, 0); }
  float* guess(void* b) const { return guided ? at<float>(b, o_guess()) : nullptr; }
  float* xr(void* b) const { return at<float>(b, o_xr()); }
};

// "kf": the n features seeded at the last keyframe (me_vo_loop_push).  ref_uv (8n) | cur_uv (8n) | new_uv (8n) |
// alive (n) | status (n), the 32-byte info block at the next 16-byte boundary.  With the frame pose: ref_xr (4n)
// ahead of alive, and the 128-byte pose block directly behind the info block.
struct Kf {
  size_t n;
  bool pose;
  size_t o_cur() const { return 8 * n; }
  size_t o_new() const { return 16 * n; }
  size_t o_ref_xr() const { return 24 * n; }  // (pose only)
  size_t o_alive() const { return (pose ? 28 : 24) * n; }
  size_t o_status() const { return o_alive() + n; }
  size_t o_info() const { return align16(o_status() + n); }
  size_t info_bytes() const { return pose ? 160 : 32; }  // the info block, and the pose block behind it
  size_t o_pose() const { return o_info() + 32; }        // (pose only)
  size_t size() const { return o_info() + info_bytes(); }
  float* ref(void* b) const { return at<float>(b, 0); }
  float* cur(void* b) const { return at<float>(b, o_cur()); }
  float* nw(void* b) const { return at<float>(b, o_new()); }
  float* ref_xr(void* b) const { return at<float>(b, o_ref_xr()); }
  uint8_t* alive(void* b) const { return at<uint8_t>(b, o_alive()); }
  uint8_t* status(void* b) const { return at<uint8_t>(b, o_status()); }
  uint8_t* info(void* b) const { return at<uint8_t>(b, o_info()); }
  uint8_t* pose_block(void* b) const { return at<uint8_t>(b, o_pose()); }
};

// The device-resident BA window store of capacity cap observations, frame by frame: obs (4 doubles, 32 cap) |
// frame (int32, 4 cap) | track ID (int32, 4 cap).  The same layout with cap = n is a frame's page-locked staging
// block "w_add", copied part by part to element e of the store.
struct WStore {
  size_t cap;
  size_t o_frame() const { return 32 * cap; }
  size_t o_id() const { return 36 * cap; }
  size_t size() const { return 40 * cap; }
  double* obs(void* b, size_t e = 0) const { return at<double>(b, 32 * e); }
  int32_t* frame(void* b, size_t e = 0) const { return at<int32_t>(b, o_frame() + 4 * e); }
  int32_t* id(void* b, size_t e = 0) const { return at<int32_t>(b, o_id() + 4 * e); }
};

// "bw": a window solve's upload.  cams (6 doubles, 48 nc) | pts (3 doubles, 24 npts) | ids (int32, 4 npts) |
// cam_src (int32, 4 nc; chained solves only: the copy stops ahead of it otherwise)
struct BaUpload {
  size_t nc, npts;
  size_t o_pts() const { return 48 * nc; }
  size_t o_ids() const { return 48 * nc + 24 * npts; }
  size_t o_cam_src() const { return o_ids() + 4 * npts; }
  size_t size() const { return o_cam_src() + 4 * nc; }
  size_t stage_bytes(bool chained) const { return chained ? size() : o_cam_src(); }
  double* cams(void* b) const { return at<double>(b, 0); }
  double* pts(void* b) const { return at<double>(b, o_pts()); }
  int32_t* ids(void* b) const { return at<int32_t>(b, o_ids()); }
  int32_t* cam_src(void* b) const { return at<int32_t>(b, o_cam_src()); }
};

// The pair pool's rule: a frame's 8-bit pair goes into the lowest slot held neither by the previous pushed frame
// (prev; -1: that frame was a keyframe) nor by either of the last two keyframes (-1: none yet).  A keyframe's pair
// is read during its call and the next one, and by the scale LM queued in the call after.  Three held at the most,
// so the pick is < 4; on a loop of keyframes only (prev always -1) it is t % 3.
constexpr int kPoolSlots = 4;
inline int pool_pick(int prev, int kf0, int kf1) {
  int s = 0;
  while (s == prev || s == kf0 || s == kf1) ++s;
  return s;
}

}  // namespace me_vo
