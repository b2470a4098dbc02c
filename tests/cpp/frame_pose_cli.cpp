// C++ caller of me::WindowedStereoVO::push with setFramePose
// (include/MotionEstimationAMD/motion_estimation_amd.hpp) -- tests only.
//
//   frame_pose_cli <in.bin>
// in.bin: int32 {width, height, n_feats, window, ba_iters, n_frames,
// min_tracked_pct, max_gap}, double {min_parallax, K[9], first_pose[6],
// velocity[6]}, then n_frames pairs of width x height 8-bit images (left,
// right), then int32 {iters, min_inliers}, double {huber, gate_max, min_disp}.
// Prints the keyframe index of every pushed frame (-1: none) on one line, then
// one line per frame pose: frame, t_ref, valid, n_inliers, steps, and R and
// t_rel as hexadecimal floating-point ("%a": python's float.fromhex reads it).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "MotionEstimationAMD/motion_estimation_amd.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: frame_pose_cli <in.bin>\n");
    return 2;
  }
  std::FILE* fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t hdr[8];
  double d[22];
  bool good = std::fread(hdr, 4, 8, fh) == 8 && std::fread(d, 8, 22, fh) == 22 && hdr[0] > 0 && hdr[1] > 0 && hdr[5] >= 0;
  std::vector<std::vector<uint8_t>> imgs;
  if (good) {
    const size_t npx = (size_t)hdr[0] * hdr[1];
    imgs.assign(2 * (size_t)hdr[5], std::vector<uint8_t>(npx));
    for (auto& im : imgs) good = good && std::fread(im.data(), 1, npx, fh) == npx;
  }
  int32_t fi[2] = {0, 0};
  double fd[3] = {0, 0, 0};
  good = good && std::fread(fi, 4, 2, fh) == 2 && std::fread(fd, 8, 3, fh) == 3;
  std::fclose(fh);
  if (!good) {
    std::fprintf(stderr, "frame_pose_cli: short or malformed input\n");
    return 2;
  }
  try {
    me::amd::Context ctx(0);
    me::WindowedStereoVO::Config cfg;
    cfg.width = hdr[0];
    cfg.height = hdr[1];
    cfg.n_feats = hdr[2];
    cfg.window = hdr[3];
    cfg.ba_iters = hdr[4];
    for (int k = 0; k < 9; ++k) cfg.K[k] = d[1 + k];
    for (int k = 0; k < 6; ++k) cfg.first_pose[k] = d[10 + k];
    for (int k = 0; k < 6; ++k) cfg.velocity[k] = d[16 + k];
    cfg.has_velocity = 1;
    me::WindowedStereoVO vo(ctx, ctx, cfg);
    const me_kf_params p{d[0], hdr[6], hdr[7]};
    vo.setKeyframeSelect(&p);
    const me_frame_pose_params fp{fd[0], fd[1], fd[2], fi[0], fi[1]};
    vo.setFramePose(&fp);
    for (int i = 0; i < hdr[5]; ++i) {
      me::amd::ImageView l, r;
      l.data = imgs[2 * (size_t)i].data();
      r.data = imgs[2 * (size_t)i + 1].data();
      l.rows = r.rows = hdr[1];
      l.cols = r.cols = l.step = r.step = hdr[0];
      std::printf("%d%c", vo.push(l, r), i + 1 == hdr[5] ? '\n' : ' ');
    }
    vo.finish();
    for (const me_vo_frame_pose& r : vo.framePoses()) {
      std::printf("%d %d %d %d %d", r.frame, r.t_ref, r.valid, r.n_inliers, r.steps);
      for (int k = 0; k < 9; ++k) std::printf(" %a", r.R[k]);
      for (int k = 0; k < 3; ++k) std::printf(" %a", r.t_rel[k]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frame_pose_cli: %s\n", e.what());
    return 1;
  }
  return 0;
}
