// C++ caller of the guided overloads of me::calcOpticalFlowPyrLK
// (include/MotionEstimationAMD/motion_estimation_amd.hpp) -- tests only.
//
//   klt_guided_cli <in.bin>
// in.bin: int32 {width, height, n}, double fb_max (0: no forward-backward
// check), prev (width * height bytes), next, n (x, y) float pairs, n (x, y)
// float pairs of initial flow.  Prints one line per feature:
// "<status> <fb_err bits as 8 hex digits> <x bits> <y bits>" (fb_err bits 0
// without the check).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "MotionEstimationAMD/motion_estimation_amd.hpp"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: klt_guided_cli <in.bin>\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t hdr[3];
  double fb_max = 0;
  bool ok = std::fread(hdr, 4, 3, fh) == 3 && std::fread(&fb_max, 8, 1, fh) == 1;
  ok = ok && hdr[0] > 0 && hdr[1] > 0 && hdr[2] >= 0;
  std::vector<uint8_t> prev, next;
  std::vector<me::Point2f> pts, flow;
  if (ok) {
    const size_t npx = (size_t)hdr[0] * hdr[1], n = (size_t)hdr[2];
    prev.resize(npx);
    next.resize(npx);
    pts.resize(n);
    flow.resize(n);
    ok = std::fread(prev.data(), 1, npx, fh) == npx && std::fread(next.data(), 1, npx, fh) == npx &&
         (n == 0 || (std::fread(pts.data(), sizeof(me::Point2f), n, fh) == n &&
                     std::fread(flow.data(), sizeof(me::Point2f), n, fh) == n));
  }
  std::fclose(fh);
  if (!ok) {
    std::fprintf(stderr, "klt_guided_cli: short or malformed input\n");
    return 2;
  }
  try {
    const me::amd::ImageView vp{prev.data(), hdr[1], hdr[0], hdr[0]}, vn{next.data(), hdr[1], hdr[0], hdr[0]};
    std::vector<me::Point2f> out;
    std::vector<uint8_t> status;
    std::vector<float> fb_err(pts.size(), 0.f);
    if (fb_max > 0.0)
      me::calcOpticalFlowPyrLK(vp, vn, pts, flow, out, status, fb_err, fb_max);
    else
      me::calcOpticalFlowPyrLK(vp, vn, pts, flow, out, status);
    for (size_t i = 0; i < pts.size(); ++i)
      std::printf("%d %08x %08x %08x\n", (int)status[i], bits(fb_err[i]), bits(out[i].x), bits(out[i].y));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "klt_guided_cli: %s\n", e.what());
    return 1;
  }
  return 0;
}
