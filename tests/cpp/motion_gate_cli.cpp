// C++ caller of me::amd::motionGate
// (include/MotionEstimationAMD/motion_estimation_amd.hpp) -- tests only.
//
//   motion_gate_cli <in.bin>
// in.bin: int32 {n, width, height, t, n_hyp, refine, min_inliers}, uint32
// seed, double {f, cx, cy, baseline, gate_max, min_disp}, float margin, n
// (u, v, xr) float triples of keyframe t - 1, n of keyframe t, n status
// bytes, n ok bytes.  Prints the info block's 32 words as hex on one line,
// then one line per feature: "<ok> <err bits as 8 hex digits>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "MotionEstimationAMD/motion_estimation_amd.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: motion_gate_cli <in.bin>\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t hdr[7];
  uint32_t seed = 0;
  double d[6];
  float margin = 0;
  bool good = std::fread(hdr, 4, 7, fh) == 7 && std::fread(&seed, 4, 1, fh) == 1 && std::fread(d, 8, 6, fh) == 6 &&
              std::fread(&margin, 4, 1, fh) == 1 && hdr[0] >= 0;
  std::vector<me::amd::Point3f> prev, cur;
  std::vector<uint8_t> status, ok;
  if (good) {
    const size_t n = (size_t)hdr[0];
    prev.resize(n);
    cur.resize(n);
    status.resize(n);
    ok.resize(n);
    good = n == 0 || (std::fread(prev.data(), 12, n, fh) == n && std::fread(cur.data(), 12, n, fh) == n &&
                      std::fread(status.data(), 1, n, fh) == n && std::fread(ok.data(), 1, n, fh) == n);
  }
  std::fclose(fh);
  if (!good) {
    std::fprintf(stderr, "motion_gate_cli: short or malformed input\n");
    return 2;
  }
  try {
    me_motion_gate_params p;
    me_motion_gate_default_params(&p);
    p.n_hyp = hdr[4];
    p.refine = hdr[5];
    p.min_inliers = hdr[6];
    p.seed = seed;
    p.gate_max = d[4];
    p.min_disp = d[5];
    const me::amd::MotionGateCamera cam{d[0], d[1], d[2], d[3], hdr[1], hdr[2], margin};
    std::vector<float> err;
    me::amd::MotionGateInfo info;
    me::amd::motionGate(prev, cur, status, ok, cam, hdr[3], p, err, info);
    uint32_t w[32];
    std::memcpy(w, &info, 128);
    for (int i = 0; i < 32; ++i) std::printf("%08x%c", w[i], i == 31 ? '\n' : ' ');
    for (size_t i = 0; i < ok.size(); ++i) {
      uint32_t u;
      std::memcpy(&u, &err[i], 4);
      std::printf("%d %08x\n", (int)ok[i], u);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "motion_gate_cli: %s\n", e.what());
    return 1;
  }
  return 0;
}
