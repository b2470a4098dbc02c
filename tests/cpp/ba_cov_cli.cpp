// ba_cov_cli — the window covariance through the C++ mirror
// (include/MotionEstimationAMD/motion_estimation_amd.hpp): BundleAdjuster<M>
// with compute_cov, whose getPosesCovariance() and getPointsCovariance() fill
// together.  tests/test_window_cov_gpu.py compiles it and compares the blocks
// with the Python mirror's.
//   ba_cov_cli <in.bin> <out.bin> <iterations>
// in:  nc np no fixed obs_dim | K0 K1 | baseline feat_var | cams pts obs cam_idx pt_idx [cam_id]
// out: status | cams | pts | n, n x 36 pose blocks | n, n x 9 landmark blocks
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

#include "MotionEstimationAMD/motion_estimation_amd.hpp"

namespace {
struct Reader {
  std::vector<char> buf;
  size_t pos = 0;
  void need(size_t bytes) const {
    if (bytes > buf.size() - pos) throw std::runtime_error("input file is shorter than its header says");
  }
  template <class T>
  T get() {
    T v;
    need(sizeof(T));
    std::memcpy(&v, buf.data() + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
  template <class T>
  void get(T* dst, size_t n) {
    if (n > (buf.size() - pos) / sizeof(T)) throw std::runtime_error("input file is shorter than its header says");
    if (n) std::memcpy(dst, buf.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
  }
};

template <int M>
int run(Reader& in, FILE* out, int nc, int np, int no, int fixed, int iterations) {
  using namespace me::optimisation;
  CalibrationParameters calib;
  calib.K.resize(2);
  in.get(calib.K[0].data(), 9);
  in.get(calib.K[1].data(), 9);
  calib.baseline = in.get<double>();
  calib.feat_var = in.get<double>();
  calib.compute_cov = true;
  std::vector<std::array<double, 6>> cams(nc);
  std::vector<std::array<double, 3>> pts(np);
  in.get(cams[0].data(), 6 * (size_t)nc);
  in.get(pts[0].data(), 3 * (size_t)np);
  std::vector<double> o(M * (size_t)no);
  in.get(o.data(), o.size());
  std::vector<int32_t> ci(no), pi(no), cid(no, 0);
  in.get(ci.data(), no);
  in.get(pi.data(), no);
  if (M == 2) in.get(cid.data(), no);
  std::vector<Observation<M>> obs(no);
  for (int k = 0; k < no; ++k) {
    for (int a = 0; a < M; ++a) obs[k].xy[a] = o[M * k + a];
    obs[k].camIdx = ci[k];
    obs[k].ptIdx = pi[k];
    obs[k].camID = cid[k];
  }
  BundleAdjuster<M> ba(calib, cams, pts, obs);
  ba.options().max_num_iterations = iterations;  // fixed work: tolerances off
  ba.options().function_tolerance = ba.options().gradient_tolerance = ba.options().parameter_tolerance = 0.0;
  const int32_t st = (int32_t)ba.optimise(fixed);
  fwrite(&st, 4, 1, out);
  fwrite(ba.getCameraParams()[0].data(), 8, 6 * (size_t)nc, out);
  fwrite(ba.getPoints()[0].data(), 8, 3 * (size_t)np, out);
  const int32_t ncam = (int32_t)ba.getPosesCovariance().size(), npt = (int32_t)ba.getPointsCovariance().size();
  fwrite(&ncam, 4, 1, out);
  for (const auto& c : ba.getPosesCovariance()) fwrite(c.data(), 8, 36, out);
  fwrite(&npt, 4, 1, out);
  for (const auto& c : ba.getPointsCovariance()) fwrite(c.data(), 8, 9, out);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ba_cov_cli <in.bin> <out.bin> <iterations>\n");
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "ba_cov_cli: cannot open %s\n", argv[1]);
    return 2;
  }
  Reader in;
  in.buf.assign(std::istreambuf_iterator<char>(f), {});
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) {
    std::fprintf(stderr, "ba_cov_cli: cannot write %s\n", argv[2]);
    return 2;
  }
  int rc = 1;
  try {
    const int nc = in.get<int32_t>(), np = in.get<int32_t>(), no = in.get<int32_t>(), fixed = in.get<int32_t>();
    const int od = in.get<int32_t>(), it = std::atoi(argv[3]);
    if (nc < 1 || np < 1 || no < 0 || (od != 2 && od != 4)) throw std::runtime_error("bad sizes in the input header");
    rc = od == 2 ? run<2>(in, out, nc, np, no, fixed, it) : run<4>(in, out, nc, np, no, fixed, it);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ba_cov_cli: %s\n", e.what());
  }
  std::fclose(out);
  return rc;
}
