// gate_math.hpp — device helpers shared by the rigid-motion gate
// (motion_gate.hip, me_hip.h A12h) and the frame pose (frame_pose.hip, A12j):
// the reprojection, the 6 x 6 Cholesky and the Cayley update, so that both
// files compile the same text.  FP64, + - * / sqrt only, every expression as
// the header writes it; the library is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace me_gate {

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Y = R P + t and its left-image projection (A12h step 6); g holds f, cx, cy
template <class G>
__device__ __forceinline__ void project(const double* R, const double* t, const double* P, const G& g, double* Y,
                                        double& uh, double& vh) {
  for (int i = 0; i < 3; ++i) Y[i] = ((R[3 * i] * P[0] + R[3 * i + 1] * P[1]) + R[3 * i + 2] * P[2]) + t[i];
  uh = g.f * Y[0] / Y[2] + g.cx;
  vh = g.f * Y[1] / Y[2] + g.cy;
}

// Y = R P + t, the three stereo residuals and their squared norm; g holds f, cx, cy, fb
template <class G>
__device__ __forceinline__ void reproject(const double* R, const double* t, const double* P, double u, double v,
                                          double xr, const G& g, double* Y, double* r, double& e2) {
  double uh, vh;
  project(R, t, P, g, Y, uh, vh);
  const double xh = uh - g.fb / Y[2];
  r[0] = uh - u;
  r[1] = vh - v;
  r[2] = xh - xr;
  e2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}

// x with A x = b, A 6 x 6 symmetric (full storage), by a textbook Cholesky; false at the first pivot not > 0
__device__ inline bool cholesky6(const double (*A)[6], const double* b, double* x) {
  double L[6][6];
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      s = A[i][j];
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return true;
}

// One Gauss-Newton solve and update from the 27 ordered sums tot (the upper triangle of H row-major, then b):
// H d = -b, then the Cayley rotation of c = w / 2 with R <- C R, t <- C t + dt into pose (R row-major, t).
// False where the Cholesky stops: pose keeps its values.
__device__ inline bool gn_update(const double* tot, double* pose) {
  double A[6][6], b[6], d[6];
  int s = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = tot[s];
      A[j][i] = tot[s];
      ++s;
    }
  for (int i = 0; i < 6; ++i) b[i] = -tot[21 + i];
  if (!cholesky6(A, b, d)) return false;
  const double* R = pose;
  const double* t = pose + 9;
  const double c[3] = {0.5 * d[0], 0.5 * d[1], 0.5 * d[2]};
  const double cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  const double den = 1.0 + cc, om = 1.0 - cc;
  double C[9];
  C[0] = (om + 2.0 * (c[0] * c[0])) / den;
  C[4] = (om + 2.0 * (c[1] * c[1])) / den;
  C[8] = (om + 2.0 * (c[2] * c[2])) / den;
  C[1] = (2.0 * (c[0] * c[1]) - 2.0 * c[2]) / den;
  C[2] = (2.0 * (c[0] * c[2]) + 2.0 * c[1]) / den;
  C[3] = (2.0 * (c[1] * c[0]) + 2.0 * c[2]) / den;
  C[5] = (2.0 * (c[1] * c[2]) - 2.0 * c[0]) / den;
  C[6] = (2.0 * (c[2] * c[0]) - 2.0 * c[1]) / den;
  C[7] = (2.0 * (c[2] * c[1]) + 2.0 * c[0]) / den;
  double Rn[9], tn[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (C[3 * i] * R[j] + C[3 * i + 1] * R[3 + j]) + C[3 * i + 2] * R[6 + j];
    tn[i] = ((C[3 * i] * t[0] + C[3 * i + 1] * t[1]) + C[3 * i + 2] * t[2]) + d[3 + i];
  }
  for (int i = 0; i < 9; ++i) pose[i] = Rn[i];
  for (int i = 0; i < 3; ++i) pose[9 + i] = tn[i];
  return true;
}

}  // namespace me_gate
