// vo_math.hpp -- the VO loop's pure host arithmetic (vo_loop.cpp).
//
// Every function here is pipeline.py's / synthetic.py's, in the same expression order: rot_series, move_landmark,
// cell_jitter, the grid, new_cells_host, in_margin, predict_pose and the disparity window use only + - * /,
// rounding and comparisons, so they match Python bit for bit; aa_to_R, triangulate, predict_uv and
// predicted_disparity go through sin / cos or a matrix product and match to rounding.  Host only, no HIP and no
// context: tests/cpp/vo_host_cli.cpp runs them on the CPU (tests/test_vo_loop_host.py).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <vector>

namespace me_vo {

constexpr int kPatch = 11;                // MI patch (11 x 11)
constexpr int kWScale = 5;                // ScaleState::window_size
constexpr int kMargin = 4 * kWScale + 4;  // feature margin (pipeline.MARGIN)
constexpr int kHalf = 6;                  // tracked features search +-6 px around the predicted disparity
constexpr double kRatio = 1.2;            // uniqueness ratio of new features

using Pose = std::array<double, 6>;  // {t, angle-axis} world -> camera
using Mat3 = std::array<double, 9>;

// synthetic.aa_to_R: Rodrigues, I + sin(th) [w]x + (1 - cos th) [w]x^2
inline Mat3 aa_to_R(const double* aa) {
  const double th = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  Mat3 R{1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (th < 1e-12) return R;
  const double w[3] = {aa[0] / th, aa[1] / th, aa[2] / th};
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  const double s = std::sin(th), c1 = 1 - std::cos(th);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double w2 = 0.0;
      for (int k = 0; k < 3; ++k) w2 += W[3 * i + k] * W[3 * k + j];
      R[3 * i + j] = (R[3 * i + j] + s * W[3 * i + j]) + c1 * w2;
    }
  return R;
}

// synthetic.R_to_quat: (w, x, y, z), w >= 0, through the trace angle-axis
inline std::array<double, 4> R_to_quat(const Mat3& R) {
  const double c = std::max(-1.0, std::min(1.0, ((R[0] + R[4] + R[8]) - 1) / 2));
  const double th = std::acos(c);
  if (th < 1e-12) return {1.0, 0.0, 0.0, 0.0};
  const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double k = th / (2 * std::sin(th));
  const double aa[3] = {v[0] * k, v[1] * k, v[2] * k};
  const double n = std::sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
  if (n < 1e-12) return {1.0, 0.0, 0.0, 0.0};
  const double s = std::sin(n / 2);
  return {std::cos(n / 2), aa[0] / n * s, aa[1] / n * s, aa[2] / n * s};
}

// pipeline.rot_series / vo_chain_kernel's rot_series: the same literals and order
constexpr double kRotA[24] = {1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984,
                              2.7557319223985893e-06, -2.505210838544172e-08, 1.6059043836821613e-10,
                              -7.647163731819816e-13, 2.8114572543455206e-15, -8.22063524662433e-18,
                              1.9572941063391263e-20, -3.868170170630684e-23, 6.446950284384474e-26,
                              -9.183689863795546e-29, 1.1309962886447716e-31, -1.216125041553518e-34,
                              1.151633562077195e-37, -9.67759295863189e-41, 7.265460179153071e-44,
                              -4.902469756513544e-47, 2.9893108271424046e-50, -1.6552108677421951e-53,
                              8.359650847182804e-57, -3.866628513960594e-60};
constexpr double kRotB[24] = {0.5, -0.041666666666666664, 0.001388888888888889, -2.48015873015873e-05,
                              2.755731922398589e-07, -2.08767569878681e-09, 1.1470745597729725e-11,
                              -4.779477332387385e-14, 1.5619206968586225e-16, -4.110317623312165e-19,
                              8.896791392450574e-22, -1.6117375710961184e-24, 2.4795962632247976e-27,
                              -3.279889237069838e-30, 3.7699876288159054e-33, -3.8003907548547434e-36,
                              3.387157535521162e-39, -2.6882202662866363e-42, 1.911963205040282e-45,
                              -1.2256174391283858e-48, 7.117406731291439e-52, -3.7618428812322616e-55,
                              1.817315401561479e-58, -8.055476070751236e-62};
inline Mat3 rot_series(const double* a) {
  const double a0 = a[0], a1 = a[1], a2 = a[2];
  const double t2 = (a0 * a0 + a1 * a1) + a2 * a2;
  double A = kRotA[23], B = kRotB[23];
  for (int k = 22; k >= 0; --k) {
    A = A * t2 + kRotA[k];
    B = B * t2 + kRotB[k];
  }
  const double av[3] = {a0, a1, a2};
  const double K[9] = {0.0, -a2, a1, a2, 0.0, -a0, -a1, a0, 0.0};
  Mat3 R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double k2 = av[i] * av[j] - (i == j ? t2 : 0.0);
      R[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
    }
  return R;
}

// pipeline.move_landmarks: x_c = R X + t, then R2^T (x_c - t2), elementwise in that order
inline void move_landmark(double* X, const Mat3& R, const Pose& pose, const Pose& pose2, const Mat3& R2) {
  double d[3];
  for (int k = 0; k < 3; ++k)
    d[k] = (((X[0] * R[3 * k] + X[1] * R[3 * k + 1]) + X[2] * R[3 * k + 2]) + pose[k]) - pose2[k];
  for (int k = 0; k < 3; ++k) X[k] = (d[0] * R2[k] + d[1] * R2[3 + k]) + d[2] * R2[6 + k];
}

// pipeline._cell_jitter: deterministic jitter in [-0.3, 0.3) per (frame, cell)
inline void cell_jitter(int t, int64_t cell, double* j) {
  uint64_t h = ((uint64_t)cell * 2654435761ull + (uint64_t)t * 40503ull) & 0xFFFFFFFFull;
  h ^= h >> 15;
  h = (h * 2246822519ull) & 0xFFFFFFFFull;
  const double a = (double)(h & 0xFFFF) / 65536.0, b = (double)((h >> 16) & 0xFFFF) / 65536.0;
  j[0] = a * 0.6 - 0.3;
  j[1] = b * 0.6 - 0.3;
}

// The grid of feature cells over the margin-free interior (WindowedStereoVO.__init__)
struct Grid {
  int nx = 1, ny = 1;
  double cw = 1, ch = 1;
};
inline Grid make_grid(int width, int height, int n_feats) {
  const double aw = width - 2 * kMargin, ah = height - 2 * kMargin;
  Grid g;
  g.nx = std::max(1, (int)std::nearbyint(std::sqrt(n_feats * aw / ah)));
  g.ny = std::max(1, (int)std::ceil((double)n_feats / g.nx));
  g.cw = aw / g.nx;
  g.ch = ah / g.ny;
  return g;
}

inline bool in_margin(float u, float v, int width, int height) {
  return u >= kMargin && u < width - kMargin && v >= kMargin && v < height - kMargin;
}

// pipeline.new_cells on the host (first keyframe: no tracked features)
inline void new_cells_host(int t, int n_good, const float* uv_good, const Grid& g, int n_feats, std::vector<float>& out) {
  const int nx = g.nx, ny = g.ny;
  const double cw = g.cw, ch = g.ch;
  std::vector<uint8_t> occ((size_t)nx * ny, 0);
  for (int i = 0; i < n_good; ++i) {
    long ccx = (long)(((double)uv_good[2 * i] - kMargin) / cw), ccy = (long)(((double)uv_good[2 * i + 1] - kMargin) / ch);
    ccx = std::min<long>(std::max<long>(ccx, 0), nx - 1);
    ccy = std::min<long>(std::max<long>(ccy, 0), ny - 1);
    occ[ccy * nx + ccx] = 1;
  }
  const long want = std::max(0, n_feats - n_good);
  out.clear();
  for (long cell = 0; cell < (long)occ.size() && (long)out.size() / 2 < want; ++cell) {
    if (occ[cell]) continue;
    double j[2];
    cell_jitter(t, cell, j);
    out.push_back((float)(kMargin + (((double)(cell % nx) + 0.5) + j[0]) * cw));
    out.push_back((float)(kMargin + (((double)(cell / nx) + 0.5) + j[1]) * ch));
  }
}

// The loop's camera: K[0], K[2], K[5] and the stereo baseline
struct Camera {
  double f = 0, cx = 0, cy = 0, baseline = 0;
};

// WindowedStereoVO._triangulate: R^T (p_c - t) of the feature's camera-frame point
inline void triangulate(float u, float v, float xr, const Camera& cam, const Pose& pose, const Mat3& R, double* Xo) {
  const double disp = (double)u - (double)xr;
  const double Z = cam.f * cam.baseline / disp;
  const double pc[3] = {((double)u - cam.cx) * Z / cam.f, ((double)v - cam.cy) * Z / cam.f, Z};
  for (int j = 0; j < 3; ++j) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i) s += (pc[i] - pose[i]) * R[3 * i + j];
    Xo[j] = s;
  }
}

// WindowedStereoVO._predict_pose: constant velocity from the last two poses; the prior velocity (nullptr: none)
// for the second keyframe or when pose(t - 2) is gone
inline Pose predict_pose(const std::map<int, Pose>& poses, int t, const Pose& first_pose, const double* velocity) {
  if (t == 0) return first_pose;
  const Pose& p1 = poses.at(t - 1);
  Pose v{};
  const auto p2 = t == 1 ? poses.end() : poses.find(t - 2);
  if (p2 == poses.end()) {
    if (velocity)
      for (int k = 0; k < 6; ++k) v[k] = velocity[k];
  } else {
    for (int k = 0; k < 6; ++k) v[k] = p1[k] - p2->second[k];
  }
  Pose out;
  for (int k = 0; k < 6; ++k) out[k] = p1[k] + v[k];
  return out;
}

// WindowedStereoVO._predicted_disparity of one landmark: f b / Z at the pose (rotation R), NaN where Z <= 0
inline double predicted_disparity(const double* X, const Mat3& R, const Pose& pose, const Camera& cam) {
  const double Z = (X[0] * R[6] + X[1] * R[7] + X[2] * R[8]) + pose[2];
  return Z > 0 ? cam.f * cam.baseline / Z : std::numeric_limits<double>::quiet_NaN();
}

// WindowedStereoVO.search_window of one tracked feature: the first of the 2 kHalf + 1 candidates around the
// predicted disparity dp, clamped to [d_min, d_max], and whether dp is usable at all
inline void search_window(double dp, int d_min, int d_max, int32_t* lo, uint8_t* dvalid) {
  const bool fin = std::isfinite(dp);
  const double dpc = fin ? std::min(dp, 1e9) : -1e9;  // (numpy's float -> int64 of a huge rint is undefined too)
  long l = (long)std::nearbyint(dpc) - kHalf;
  l = std::min<long>(std::max<long>(l, d_min), d_max);
  *lo = (int32_t)l;
  *dvalid = fin && dp > 0;
}

// pipeline.predict_uv of one landmark (klt_predict's guess): its pixel at the pose (rotation R), NaN where Z <= 0
inline void predict_uv(const double* X, const Mat3& R, const Pose& pose, const Camera& cam, float* uv) {
  const double Xc = (X[0] * R[0] + X[1] * R[1]) + X[2] * R[2] + pose[0];
  const double Yc = (X[0] * R[3] + X[1] * R[4]) + X[2] * R[5] + pose[1];
  const double Z = (X[0] * R[6] + X[1] * R[7] + X[2] * R[8]) + pose[2];
  const float nan = std::numeric_limits<float>::quiet_NaN();
  uv[0] = Z > 0 ? (float)(cam.f * Xc / Z + cam.cx) : nan;
  uv[1] = Z > 0 ? (float)(cam.f * Yc / Z + cam.cy) : nan;
}

}  // namespace me_vo
