// ba_residual.hpp — part of ba.hip: one observation's residual and analytic
// Jacobian.  Defines no kernel: the angle-axis rotation and its table form
// (rotate, rot_entry, rotate_tab, rotate_cam), the stereo and mono residuals,
// obs_residual[_tab] and the Huber corrector.  Reads no other part.
#pragma once
#include "ba_types.hpp"

using namespace ba;

namespace {

constexpr double kDblMin = 2.2250738585072014e-308;
constexpr double kDblEps = 2.220446049250313e-16;

// p = R(aa) X + t with dp/daa and dp/dX (ceres::AngleAxisRotatePoint values;
// derivative: Gallego & Yezzi, d(Ru)/dw = -R[u]x (w w^T + (R^T - I)[w]x)/theta^2)
__device__ __forceinline__ void rotate(const double* aa, const double* X, double* P, double* dPdw, double* dPdX) {
  const double t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (t2 > kDblEps) {
    const double th = sqrt(t2), c = cos(th), s = sin(th), ti = 1.0 / th;
    const double w0 = aa[0] * ti, w1 = aa[1] * ti, w2 = aa[2] * ti;
    const double wx0 = w1 * X[2] - w2 * X[1], wx1 = w2 * X[0] - w0 * X[2], wx2 = w0 * X[1] - w1 * X[0];
    const double tmp = (w0 * X[0] + w1 * X[1] + w2 * X[2]) * (1.0 - c);
    P[0] = X[0] * c + wx0 * s + w0 * tmp;
    P[1] = X[1] * c + wx1 * s + w1 * tmp;
    P[2] = X[2] * c + wx2 * s + w2 * tmp;
    if (dPdX) {
      const double oc = 1.0 - c;
      double R[9] = {c + oc * w0 * w0,      oc * w0 * w1 - s * w2, oc * w0 * w2 + s * w1,
                     oc * w1 * w0 + s * w2, c + oc * w1 * w1,      oc * w1 * w2 - s * w0,
                     oc * w2 * w0 - s * w1, oc * w2 * w1 + s * w0, c + oc * w2 * w2};
      for (int i = 0; i < 9; ++i) dPdX[i] = R[i];
      // M = (w w^T + (R^T - I)[w]x) / theta^2 with w = aa (unnormalised)
      const double a0 = aa[0], a1 = aa[1], a2 = aa[2];
      double Wx[9] = {0, -a2, a1, a2, 0, -a0, -a1, a0, 0};
      double M[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double acc = aa[i] * aa[j];
          for (int k = 0; k < 3; ++k) acc += (R[k * 3 + i] - (i == k ? 1.0 : 0.0)) * Wx[k * 3 + j];
          M[i * 3 + j] = acc / t2;
        }
      // -R [X]x M
      double Xx[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
      double RX[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) RX[i * 3 + j] = R[i * 3 + 0] * Xx[0 * 3 + j] + R[i * 3 + 1] * Xx[1 * 3 + j] + R[i * 3 + 2] * Xx[2 * 3 + j];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          dPdw[i * 3 + j] = -(RX[i * 3 + 0] * M[0 * 3 + j] + RX[i * 3 + 1] * M[1 * 3 + j] + RX[i * 3 + 2] * M[2 * 3 + j]);
    }
  } else {
    const double wx0 = aa[1] * X[2] - aa[2] * X[1], wx1 = aa[2] * X[0] - aa[0] * X[2], wx2 = aa[0] * X[1] - aa[1] * X[0];
    P[0] = X[0] + wx0;
    P[1] = X[1] + wx1;
    P[2] = X[2] + wx2;
    if (dPdX) {
      double D[9] = {1, -aa[2], aa[1], aa[2], 1, -aa[0], -aa[1], aa[0], 1};
      for (int i = 0; i < 9; ++i) dPdX[i] = D[i];
      double N[9] = {0, X[2], -X[1], -X[2], 0, X[0], X[1], -X[0], 0};  // -[X]x
      for (int i = 0; i < 9; ++i) dPdw[i] = N[i];
    }
  }
}

// One camera's entry of the rotation table (Bufs::rot, kRotStride doubles)
// from its angle-axis vector: rotate()'s own expressions for R and M, formed
// once per camera instead of once per observation.  Called where cameras are
// written: plan_count_kernel (the starting cameras) and rot_step_body (the
// candidates).
__device__ __forceinline__ void rot_entry(const double* aa, double* e) {
  const double t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  double R[9], M[9];
  if (t2 > kDblEps) {
    const double th = sqrt(t2), c = cos(th), s = sin(th), ti = 1.0 / th;
    const double w0 = aa[0] * ti, w1 = aa[1] * ti, w2 = aa[2] * ti;
    const double oc = 1.0 - c;
    const double Rr[9] = {c + oc * w0 * w0,      oc * w0 * w1 - s * w2, oc * w0 * w2 + s * w1,
                          oc * w1 * w0 + s * w2, c + oc * w1 * w1,      oc * w1 * w2 - s * w0,
                          oc * w2 * w0 - s * w1, oc * w2 * w1 + s * w0, c + oc * w2 * w2};
    const double a0 = aa[0], a1 = aa[1], a2 = aa[2];
    const double Wx[9] = {0, -a2, a1, a2, 0, -a0, -a1, a0, 0};
    for (int i = 0; i < 9; ++i) R[i] = Rr[i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double acc = aa[i] * aa[j];
        for (int k = 0; k < 3; ++k) acc += (R[k * 3 + i] - (i == k ? 1.0 : 0.0)) * Wx[k * 3 + j];
        M[i * 3 + j] = acc / t2;
      }
  } else {
    const double D[9] = {1, -aa[2], aa[1], aa[2], 1, -aa[0], -aa[1], aa[0], 1};  // I + [aa]x
    for (int i = 0; i < 9; ++i) {
      R[i] = D[i];
      M[i] = 0.0;
    }
  }
  for (int i = 0; i < 9; ++i) {
    e[ROT_R + i] = R[i];
    e[ROT_M + i] = M[i];
  }
  e[ROT_BRANCH] = t2 > kDblEps ? 1.0 : 0.0;
  e[ROT_BRANCH + 1] = 0.0;
}

// rotate() from the camera's table entry: P = R X, dP/dX = R and
// dP/dw = -(R [X]x) M; an entry of the small-angle branch keeps that branch's
// meaning, P = X + aa x X (aa read back from R = I + [aa]x: rotate()'s bits),
// dP/dX = I + [aa]x, dP/dw = -[X]x.
__device__ __forceinline__ void rotate_tab(const double* e, const double* X, double* P, double* dPdw, double* dPdX) {
  double R[9];
  for (int i = 0; i < 9; ++i) R[i] = e[ROT_R + i];
  if (e[ROT_BRANCH] != 0.0) {
    for (int i = 0; i < 3; ++i) P[i] = R[i * 3 + 0] * X[0] + R[i * 3 + 1] * X[1] + R[i * 3 + 2] * X[2];
    if (dPdX) {
      double M[9];
      for (int i = 0; i < 9; ++i) M[i] = e[ROT_M + i];
      for (int i = 0; i < 9; ++i) dPdX[i] = R[i];
      // -R [X]x M
      double Xx[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
      double RX[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) RX[i * 3 + j] = R[i * 3 + 0] * Xx[0 * 3 + j] + R[i * 3 + 1] * Xx[1 * 3 + j] + R[i * 3 + 2] * Xx[2 * 3 + j];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          dPdw[i * 3 + j] = -(RX[i * 3 + 0] * M[0 * 3 + j] + RX[i * 3 + 1] * M[1 * 3 + j] + RX[i * 3 + 2] * M[2 * 3 + j]);
    }
  } else {
    const double a0 = R[7], a1 = R[2], a2 = R[3];
    const double wx0 = a1 * X[2] - a2 * X[1], wx1 = a2 * X[0] - a0 * X[2], wx2 = a0 * X[1] - a1 * X[0];
    P[0] = X[0] + wx0;
    P[1] = X[1] + wx1;
    P[2] = X[2] + wx2;
    if (dPdX) {
      for (int i = 0; i < 9; ++i) dPdX[i] = R[i];
      double N[9] = {0, X[2], -X[1], -X[2], 0, X[0], X[1], -X[0], 0};  // -[X]x
      for (int i = 0; i < 9; ++i) dPdw[i] = N[i];
    }
  }
}

// TAB: the camera's rotation comes from its table entry `rot` (rotate_tab: the
// linearisation and the camera assembly), else from cam[3..5] (rotate: rot unused)
template <bool TAB>
__device__ __forceinline__ void rotate_cam(const double* cam, const double* rot, const double* X, double* P,
                                           double* dPdw, double* dPdX) {
  if constexpr (TAB) rotate_tab(rot, X, P, dPdw, dPdX);
  else rotate(cam + 3, X, P, dPdw, dPdX);
}

// StereoReprojectionError (BundleAdjuster.h:153-171): residual, optional J
template <bool TAB>
__device__ __forceinline__ void stereo_residual(const Geo& g, const double* cam, const double* rot, const double* X,
                                                const double* f, double* r, double* Jc, double* Jp) {
  double P[3], dPdw[9], dPdX[9];
  rotate_cam<TAB>(cam, rot, X, P, Jc ? dPdw : nullptr, Jc ? dPdX : nullptr);
  P[0] = P[0] + cam[0];
  P[1] = P[1] + cam[1];
  P[2] = P[2] + cam[2];
  const double x1 = g.K0[0] * (P[0] / P[2]) + g.K0[2];
  const double x2 = g.K1[0] * ((P[0] - g.baseline) / P[2]) + g.K1[2];
  const double y = g.K0[4] * (P[1] / P[2]) + g.K0[5];
  r[0] = g.sinv * (x1 - f[0]);
  r[1] = g.sinv * (y - f[1]);
  r[2] = g.sinv * (x2 - f[2]);
  r[3] = g.sinv * (y - f[3]);
  if (!Jc) return;
  const double iz = 1.0 / P[2], iz2 = iz * iz;
  double dr[4][3] = {{g.sinv * g.K0[0] * iz, 0.0, -g.sinv * g.K0[0] * P[0] * iz2},
                     {0.0, g.sinv * g.K0[4] * iz, -g.sinv * g.K0[4] * P[1] * iz2},
                     {g.sinv * g.K1[0] * iz, 0.0, -g.sinv * g.K1[0] * (P[0] - g.baseline) * iz2},
                     {0.0, g.sinv * g.K0[4] * iz, -g.sinv * g.K0[4] * P[1] * iz2}};
  for (int k = 0; k < 4; ++k) {
    for (int j = 0; j < 3; ++j) Jc[k * 6 + j] = dr[k][j];
    for (int j = 0; j < 3; ++j) {
      Jc[k * 6 + 3 + j] = dr[k][0] * dPdw[0 * 3 + j] + dr[k][1] * dPdw[1 * 3 + j] + dr[k][2] * dPdw[2 * 3 + j];
      Jp[k * 3 + j] = dr[k][0] * dPdX[0 * 3 + j] + dr[k][1] * dPdX[1 * 3 + j] + dr[k][2] * dPdX[2 * 3 + j];
    }
  }
}

// BundleAdjuster<2> residuals: StandardReprojectionError (BundleAdjuster.h:71-103)
// for camID 0, StereoRightError (:106-139, p.x += cam[0] - baseline) otherwise;
// both project with K[0].  Rows 2, 3 are zero so the 4-row pipeline is shared
// (zero rows add nothing to J^T J, J^T r or the Huber argument).
template <bool TAB>
__device__ __forceinline__ void mono_residual(const Geo& g, const double* cam, const double* rot, const double* X,
                                              const double* f, bool right, double* r, double* Jc, double* Jp) {
  double P[3], dPdw[9], dPdX[9];
  rotate_cam<TAB>(cam, rot, X, P, Jc ? dPdw : nullptr, Jc ? dPdX : nullptr);
  P[0] = P[0] + (right ? cam[0] - g.baseline : cam[0]);
  P[1] = P[1] + cam[1];
  P[2] = P[2] + cam[2];
  const double x = g.K0[0] * (P[0] / P[2]) + g.K0[2];
  const double y = g.K0[4] * (P[1] / P[2]) + g.K0[5];
  r[0] = g.sinv * (x - f[0]);
  r[1] = g.sinv * (y - f[1]);
  r[2] = 0.0;
  r[3] = 0.0;
  if (!Jc) return;
  const double iz = 1.0 / P[2], iz2 = iz * iz;
  double dr[2][3] = {{g.sinv * g.K0[0] * iz, 0.0, -g.sinv * g.K0[0] * P[0] * iz2},
                     {0.0, g.sinv * g.K0[4] * iz, -g.sinv * g.K0[4] * P[1] * iz2}};
  for (int k = 0; k < 2; ++k) {
    for (int j = 0; j < 3; ++j) Jc[k * 6 + j] = dr[k][j];
    for (int j = 0; j < 3; ++j) {
      Jc[k * 6 + 3 + j] = dr[k][0] * dPdw[0 * 3 + j] + dr[k][1] * dPdw[1 * 3 + j] + dr[k][2] * dPdw[2 * 3 + j];
      Jp[k * 3 + j] = dr[k][0] * dPdX[0 * 3 + j] + dr[k][1] * dPdX[1 * 3 + j] + dr[k][2] * dPdX[2 * 3 + j];
    }
  }
  for (int k = 12; k < 24; ++k) Jc[k] = 0.0;
  for (int k = 6; k < 12; ++k) Jp[k] = 0.0;
}

// residual (+ optional Jacobian) of observation o; OD = rows of the model
// (a template parameter: one branch-free kernel instance per model)
template <int OD>
__device__ __forceinline__ void obs_residual(const Geo& g, const Bufs& b, long o, const double* cam, const double* X,
                                             double* r, double* Jc, double* Jp) {
  if (OD == 4)
    stereo_residual<false>(g, cam, nullptr, X, b.obs + 4 * o, r, Jc, Jp);
  else
    mono_residual<false>(g, cam, nullptr, X, b.obs + 2 * o, b.cam_id[o] != 0, r, Jc, Jp);
}
// The table form: the rotation terms from the camera's entry `rot` of Bufs::rot
// (cam gives the translation).  The linearisation (lin_pieces) and the camera
// assembly use this one; the cost, evaluation and covariance entry points keep
// rotate()'s per-observation form above.
template <int OD>
__device__ __forceinline__ void obs_residual_tab(const Geo& g, const Bufs& b, long o, const double* cam,
                                                 const double* rot, const double* X, double* r, double* Jc,
                                                 double* Jp) {
  if (OD == 4)
    stereo_residual<true>(g, cam, rot, X, b.obs + 4 * o, r, Jc, Jp);
  else
    mono_residual<true>(g, cam, rot, X, b.obs + 2 * o, b.cam_id[o] != 0, r, Jc, Jp);
}

// ceres::HuberLoss(1.0): rho0 and sqrt(rho1) (Corrector with rho'' <= 0)
__device__ __forceinline__ void huber(double s, double* rho0, double* sqrt_rho1) {
  if (s > 1.0) {
    const double rr = sqrt(s);
    *rho0 = 2.0 * rr - 1.0;
    *sqrt_rho1 = sqrt(fmax(kDblMin, 1.0 / rr));
  } else {
    *rho0 = s;
    *sqrt_rho1 = 1.0;
  }
}

}  // namespace
