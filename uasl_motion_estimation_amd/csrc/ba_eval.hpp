// ba_eval.hpp — part of ba.hip: the read-only entry points' kernels, outside
// the LM iteration.  Kernels: cost_kernel, eval_kernel, cov_kernel,
// cov_prep_kernel.  Reads the residuals of ba_residual.hpp and, for the
// covariance, the reduced system of ba_assemble.hpp.
#pragma once
#include "ba_types.hpp"
#include "ba_reduce.hpp"
#include "ba_residual.hpp"

using namespace ba;

namespace {

template <int OD>
__global__ __launch_bounds__(kBlock) void cost_kernel(Geo g, Bufs b, int which, double* part) {
  __shared__ double lds[4];
  const int o = blockIdx.x * kBlock + threadIdx.x;
  double c = 0;
  if (o < g.no) {
    double r[4];
    obs_residual<OD>(g, b, o, b.cams[which] + 6 * b.cam_idx[o], b.pts[which] + 3 * b.pt_idx[o], r, nullptr, nullptr);
    const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
    double rho0, sc;
    huber(s, &rho0, &sc);
    c = 0.5 * rho0;
  }
  double v[1] = {c}, out[1];
  block_sum<1>(v, out, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = out[0];
}

template <int OD>
__global__ __launch_bounds__(kBlock) void eval_kernel(Geo g, Bufs b, double* res, double* Jc, double* Jp) {
  const int o = blockIdx.x * kBlock + threadIdx.x;
  if (o >= g.no) return;
  double r[4], jc[24], jp[12];
  obs_residual<OD>(g, b, o, b.cams[0] + 6 * b.cam_idx[o], b.pts[0] + 3 * b.pt_idx[o], r, jc, jp);
  constexpr int od = OD;  // output rows per observation: Observation<M>::data size
  for (int k = 0; k < od; ++k) res[od * (long)o + k] = r[k];
  if (Jc)
    for (int k = 0; k < 6 * od; ++k) Jc[6 * od * (long)o + k] = jc[k];
  if (Jp)
    for (int k = 0; k < 3 * od; ++k) Jp[3 * od * (long)o + k] = jp[k];
}

// Pose covariance (BundleAdjuster<M>::extract_covariance, BundleAdjuster.h:478-528):
// the camera blocks of (J^T J)^-1 are the blocks of S^-1, S the undamped,
// unscaled point-eliminated camera system.  One workgroup: in-place dense
// Cholesky of S (global memory, the matrix is at most 300 x 300), X = L^-1 one
// column per thread, then cov_i = (X^T X) over camera i's six columns.  Not on
// the frame path (compute_cov is off by default, BundleAdjuster.h:41-42).
constexpr int kCovBlock = 1024;
__global__ __launch_bounds__(kCovBlock) void cov_kernel(Geo g, Bufs b, double* X, double* cov, int* ok_out) {
  __shared__ int sfail;
  const int n = g.n6, tid = threadIdx.x;
  double* A = b.S;  // row-major n x n, symmetric
  if (tid == 0) sfail = b.st->fail || b.st->bad_input;
  __syncthreads();
  for (int j = 0; j < n && !sfail; ++j) {
    if (tid == 0) {
      const double d = A[(long)j * n + j];
      if (!(d > 0.0)) sfail = 1;
      else A[(long)j * n + j] = sqrt(d);
    }
    __syncthreads();
    if (sfail) break;
    const double djj = A[(long)j * n + j];
    for (int i = j + 1 + tid; i < n; i += kCovBlock) A[(long)i * n + j] /= djj;
    __syncthreads();
    const int m = n - j - 1;  // trailing lower triangle, m(m+1)/2 entries
    for (long e = tid; e < (long)m * (m + 1) / 2; e += kCovBlock) {
      int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) / 2.0);
      while ((long)i * (i + 1) / 2 > e) --i;
      while ((long)(i + 1) * (i + 2) / 2 <= e) ++i;
      const int k = (int)(e - (long)i * (i + 1) / 2);
      const int ii = j + 1 + i, kk = j + 1 + k;
      A[(long)ii * n + kk] -= A[(long)ii * n + j] * A[(long)kk * n + j];
    }
    __syncthreads();
  }
  if (sfail) {
    if (tid == 0) *ok_out = 0;
    return;
  }
  // X = L^-1, column c by forward substitution (X column-major: X[c * n + k] = (L^-1)[k][c])
  for (int c = tid; c < n; c += kCovBlock) {
    double* x = X + (long)c * n;
    for (int k = 0; k < c; ++k) x[k] = 0.0;
    for (int k = c; k < n; ++k) {
      double acc = k == c ? 1.0 : 0.0;
      for (int l = c; l < k; ++l) acc -= A[(long)k * n + l] * x[l];
      x[k] = acc / A[(long)k * n + k];
    }
  }
  __syncthreads();
  for (int e = tid; e < 36 * g.nc; e += kCovBlock) {
    const int ci = e / 36, a = (e % 36) / 6, c = e % 6;
    double v = 0.0;
    if (ci >= g.nf) {  // constant cameras: zero block (ceres::Covariance)
      const int p = 6 * (ci - g.nf) + a, q = 6 * (ci - g.nf) + c;
      const double *xp = X + (long)p * n, *xq = X + (long)q * n;
      for (int k = max(p, q); k < n; ++k) v += xp[k] * xq[k];
    }
    cov[e] = v;
  }
  if (tid == 0) *ok_out = 1;
}

// Ceres covariance ignores the point bounds: an infeasible point does not stop it.
__global__ void cov_prep_kernel(Bufs b) {
  if (!b.st->bad_input) b.st->done = 0;
}

}  // namespace
