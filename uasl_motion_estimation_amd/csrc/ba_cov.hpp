// ba_cov.hpp — part of ba.hip: the window covariance, camera and landmark
// blocks of (J^T J)^-1 on the device (me_ba_covariance_full).  Kernels:
// cov_full_kernel, cov_points_kernel, cov_commit_kernel.  Reads the reduced
// camera system S of ba_assemble.hpp (undamped, unscaled: the plan
// me_ba_covariance builds) and the linearisation pieces of ba_linearize.hpp.
//
// With J = [Jc | Jp] (loss-corrected rows), U = Jc^T Jc, V = Jp^T Jp (3 x 3
// blocks V_j), W = Jc^T Jp and S = U - W V^-1 W^T:
//   Sigma_cc   = S^-1 = L^-T L^-1, S = L L^T
//   Sigma_pp,j = V_j^-1 + sum_a sum_b T_a^T Sigma_cc[a, b] T_b,
//                T_a = W_a V_j^-1 (6 x 3) over landmark j's observations in
//                variable cameras (the T form, not Y^T Y with Y = L^-1 W V^-1).
// All FP64, contraction off, every sum in a fixed order: two runs give the
// same bits, and the LDS and global-memory forms of the factor run the same
// arithmetic.
#pragma once
#include "ba_types.hpp"
#include "ba_linearize.hpp"

using namespace ba;

namespace {

constexpr int kCovFullBlock = 1024;
constexpr int kCovNb = 6;      // block step of the factor and the inverse: one camera
constexpr int kCovGroup = 8;   // lanes sharing one column of L^-1
// The factor works in LDS on a square of leading dimension n6 | 1 (odd: the
// column walks of the panel and trailing steps spread over the banks) up to
// n6 = 126 (21 variable cameras, 125 KiB of the CU's 160 KiB: config 3's 108
// fits); wider windows factor S where it lies.
constexpr int kCovLdsMaxN = 126;
__host__ __device__ inline int cov_ld(int n) { return n | 1; }
__host__ __device__ inline size_t cov_lds_bytes(int n) { return 8 * (size_t)n * cov_ld(n); }
constexpr int kCovMaxN = 6 * 50;  // (plan_build: npairs <= 192 keeps n6 below this)

__device__ __forceinline__ double cov_group_sum(double x) {
#pragma unroll
  for (int m = 1; m < kCovGroup; m <<= 1) x += __shfl_xor(x, m, 64);  // (every lane of the group: the same bits)
  return x;
}

// In place on the n x n row-major square A (leading dimension ld), whose
// lower triangle holds S: blocked right-looking Cholesky S = L L^T (lower
// triangle), then X = L^-1 by block rows, stored transposed in the strict
// upper triangle (A[c][k] = X[k][c], k > c) with its diagonal 1 / L[c][c] in
// dinv.  Returns false (on every thread) when S is not positive definite.
// Called by all kCovFullBlock threads of the workgroup.
__device__ bool cov_factor_invert(double* A, int ld, int n, double* dinv, int* sfail) {
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  for (int j0 = 0; j0 < n; j0 += kCovNb) {
    if (tid == 0) {  // the diagonal block, unblocked, in registers (one round of loads, not one per dependent step)
      double a[kCovNb][kCovNb];
#pragma unroll
      for (int i = 0; i < kCovNb; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) a[i][j] = A[(j0 + i) * ld + j0 + j];
      bool pd = true;
#pragma unroll
      for (int j = 0; j < kCovNb; ++j) {
        double d = a[j][j];
#pragma unroll
        for (int l = 0; l < j; ++l) d -= a[j][l] * a[j][l];
        pd = pd && d > 0.0;
        d = sqrt(d);
        a[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < kCovNb; ++i) {
          double v = a[i][j];
#pragma unroll
          for (int l = 0; l < j; ++l) v -= a[i][l] * a[j][l];
          a[i][j] = v / d;
        }
      }
      if (!pd) {
        *sfail = 1;
      } else {
#pragma unroll
        for (int i = 0; i < kCovNb; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) A[(j0 + i) * ld + j0 + j] = a[i][j];
          dinv[j0 + i] = 1.0 / a[i][i];
        }
      }
    }
    __syncthreads();
    if (*sfail) return false;
    // panel: the rows below, one thread each, L_iJ = A_iJ L_JJ^-T (the row and L_JJ in registers)
    if (j0 + kCovNb + tid < n) {
      double Lb[kCovNb][kCovNb];
#pragma unroll
      for (int c = 0; c < kCovNb; ++c)
#pragma unroll
        for (int l = 0; l <= c; ++l) Lb[c][l] = A[(j0 + c) * ld + j0 + l];
      for (int i = j0 + kCovNb + tid; i < n; i += kCovFullBlock) {
        double r[kCovNb];
#pragma unroll
        for (int c = 0; c < kCovNb; ++c) r[c] = A[i * ld + j0 + c];
#pragma unroll
        for (int c = 0; c < kCovNb; ++c) {
          double v = r[c];
#pragma unroll
          for (int l = 0; l < c; ++l) v -= r[l] * Lb[c][l];
          r[c] = v / Lb[c][c];
        }
#pragma unroll
        for (int c = 0; c < kCovNb; ++c) A[i * ld + j0 + c] = r[c];
      }
    }
    __syncthreads();
    // trailing lower triangle: A_ik -= L_iJ L_kJ^T, 32 x 32 threads over (i, k <= i)
    const int t0 = j0 + kCovNb;
    for (int i = t0 + ty; i < n; i += 32)
      for (int k = t0 + tx; k <= i; k += 32) {
        double v = A[i * ld + k];
        for (int l = 0; l < kCovNb; ++l) v -= A[i * ld + j0 + l] * A[k * ld + j0 + l];
        A[i * ld + k] = v;
      }
    __syncthreads();
  }
  // X = L^-1 by block rows K: for every earlier column c, kCovGroup lanes share
  // the sums t_r = sum_{l = c}^{k0 - 1} L[k0 + r][l] X[l][c] (lane s the terms
  // l = c + s, c + s + G, ...; added across the group in butterfly order),
  // then each solves the block's six rows X[k0 + r][c] = -(t_r + sum_{s < r}
  // L[k0 + r][k0 + s] X[k0 + s][c]) / L[k0 + r][k0 + r] and lane r stores row r.
  const int grp = tid / kCovGroup, gl = tid % kCovGroup;
  for (int k0 = 0; k0 < n; k0 += kCovNb) {
    for (int c = grp; c < k0 + kCovNb; c += kCovFullBlock / kCovGroup) {
      if (c < k0) {
        double t[kCovNb];
#pragma unroll
        for (int r = 0; r < kCovNb; ++r) t[r] = 0.0;
        for (int l = c + gl; l < k0; l += kCovGroup) {
          const double x = l == c ? dinv[c] : A[c * ld + l];
#pragma unroll
          for (int r = 0; r < kCovNb; ++r) t[r] += A[(k0 + r) * ld + l] * x;
        }
        double x[kCovNb];
#pragma unroll
        for (int r = 0; r < kCovNb; ++r) {
          double v = cov_group_sum(t[r]);
#pragma unroll
          for (int s = 0; s < r; ++s) v += A[(k0 + r) * ld + k0 + s] * x[s];
          x[r] = -v * dinv[k0 + r];
        }
#pragma unroll
        for (int r = 0; r < kCovNb; ++r)
          if (gl == r) A[c * ld + k0 + r] = x[r];
      } else if (gl == 0) {  // a column of the diagonal block: rows c + 1 .. k0 + 5 (constant indices: registers)
        double x[kCovNb];
        const int rc = c - k0;
#pragma unroll
        for (int r = 0; r < kCovNb; ++r) {
          double v = 0.0;
#pragma unroll
          for (int s = 0; s < r; ++s)
            if (s >= rc) v += A[(k0 + r) * ld + k0 + s] * x[s];
          x[r] = r < rc ? 0.0 : r == rc ? dinv[c] : -v * dinv[k0 + r];
          if (r > rc) A[c * ld + k0 + r] = x[r];
        }
      }
    }
    __syncthreads();  // (the next block row reads these rows of X, and the lower triangle is never written here)
  }
  return true;
}

// One workgroup: Sigma_cc (n6 x n6, both triangles) into Sig and the cameras'
// diagonal blocks into cam_cov (n_cams x 36, constant cameras zero).
// fail[0] = 1 where me_ba_covariance reports ok = 0: the linearisation failed
// (a landmark block not positive definite), bad_input, or S not positive
// definite (a variable camera without observations has a zero row).
template <bool LDS>
__global__ __launch_bounds__(kCovFullBlock) void cov_full_kernel(Geo g, Bufs b, double* Sig, double* cam_cov, int* fail) {
  extern __shared__ double cov_lds[];
  __shared__ double dinv[kCovMaxN];
  __shared__ int sfail;
  const int n = g.n6, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  if (tid == 0) sfail = b.st->fail || b.st->bad_input;
  __syncthreads();
  if (sfail) {
    if (tid == 0) fail[0] = 1;
    return;
  }
  const int ld = LDS ? cov_ld(n) : n;
  double* A = LDS ? cov_lds : b.S;
  if (LDS) {
    for (int e = tid; e < n * n; e += kCovFullBlock) A[(e / n) * ld + e % n] = b.S[e];
    __syncthreads();
  }
  if (!cov_factor_invert(A, ld, n, dinv, &sfail)) {
    if (tid == 0) fail[0] = 1;
    return;
  }
  // Sigma[p][q] = sum_{k >= q} X[k][p] X[k][q], p <= q, k ascending
  for (int p = ty; p < n; p += 32)
    for (int q = p + tx; q < n; q += 32) {
      double v = (p == q ? dinv[q] : A[p * ld + q]) * dinv[q];
      for (int k = q + 1; k < n; ++k) v += A[p * ld + k] * A[q * ld + k];
      Sig[(long)p * n + q] = v;
      Sig[(long)q * n + p] = v;
      if (p / 6 == q / 6) {
        double* cb = cam_cov + 36 * (long)(g.nf + p / 6);
        cb[(p % 6) * 6 + q % 6] = v;
        cb[(q % 6) * 6 + p % 6] = v;
      }
    }
  for (int e = tid; e < 36 * g.nf; e += kCovFullBlock) cam_cov[e] = 0.0;  // constant cameras (ceres::Covariance)
}

__device__ __forceinline__ bool cov_inv3(const double* V /* 6 unique */, double* Vi /* 9 */) {
  // V = L L^T (3 x 3 Cholesky), V^-1 = L^-T L^-1
  if (!(V[0] > 0.0)) return false;
  const double l00 = sqrt(V[0]), l10 = V[1] / l00, l20 = V[2] / l00;
  const double d1 = V[3] - l10 * l10;
  if (!(d1 > 0.0)) return false;
  const double l11 = sqrt(d1), l21 = (V[4] - l20 * l10) / l11;
  const double d2 = V[5] - l20 * l20 - l21 * l21;
  if (!(d2 > 0.0)) return false;
  const double l22 = sqrt(d2);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
  Vi[0] = i00 * i00 + i10 * i10 + i20 * i20;
  Vi[1] = Vi[3] = i10 * i11 + i20 * i21;
  Vi[2] = Vi[6] = i20 * i22;
  Vi[4] = i11 * i11 + i21 * i21;
  Vi[5] = Vi[7] = i21 * i22;
  Vi[8] = i22 * i22;
  return true;
}

// Landmark blocks: kCovPtLanes lanes per landmark over its point-sorted slots
// (the plan's CSR by point, p_off / p_obs / p_cam), kCovPtBlock / kCovPtLanes
// landmarks per workgroup.  Lane s takes slots s, s + lanes, ...; a landmark's
// T_a are exchanged through Tbuf (18 doubles per slot, the slot's own place).
// fail[0] is read (set by cov_full_kernel alone), fail[1] written: a V_j not
// positive definite (a landmark without observations has V_j = 0).
constexpr int kCovPtLanes = 16, kCovPtBlock = 256;
template <int OD>
__global__ __launch_bounds__(kCovPtBlock) void cov_points_kernel(Geo g, Bufs b, const double* Sig, double* Tbuf,
                                                                double* pt_cov, int* fail) {
  if (fail[0]) return;  // (uniform: no kernel of this launch writes the word)
  const int lane = threadIdx.x % kCovPtLanes;
  const int j = blockIdx.x * (kCovPtBlock / kCovPtLanes) + threadIdx.x / kCovPtLanes;
  const bool in = j < g.np;
  const int beg = in ? b.p_off[j] : 0, end = in ? b.p_off[j + 1] : 0;
  const int n = g.n6;
  // The pieces are formed again here (repeated work: Wo already holds these W_o bits after the linearisation, and
  // the Schur pass has summed a V_j of its own).  Per-observation V_o exist only in plans with a linearize_kernel
  // launch (the Schur instances that linearise in their phase A keep no obsx), so this is the one form that serves
  // every plan and sums V_j in this kernel's own fixed order.
  double V[6] = {0, 0, 0, 0, 0, 0};
  for (int q = beg + lane; q < end; q += kCovPtLanes) {
    const int o = b.p_obs[q], ci = b.cam_idx[o];
    double X[9], W[18];
    lin_pieces<OD>(g, b, o, b.cams[0] + 6 * ci, b.rot[0] + kRotStride * ci, b.pts[0] + 3 * (long)j, ci >= g.nf, X, W);
    for (int i = 0; i < 6; ++i) V[i] += X[i];
    if (ci >= g.nf)
      for (int i = 0; i < 18; ++i) Tbuf[18 * (long)q + i] = W[i];
  }
  for (int i = 0; i < 6; ++i)
    for (int m = 1; m < kCovPtLanes; m <<= 1) V[i] += __shfl_xor(V[i], m, 64);
  double Vi[9];
  const bool pd = cov_inv3(V, Vi);
  if (in && !pd && lane == 0) fail[1] = 1;
  // T_a = W_a V^-1, in place (this lane's own slots)
  if (pd)
    for (int q = beg + lane; q < end; q += kCovPtLanes) {
      if (b.p_cam[q] < 0) continue;
      double* T = Tbuf + 18 * (long)q;
      for (int a = 0; a < 6; ++a) {
        const double w0 = T[3 * a], w1 = T[3 * a + 1], w2 = T[3 * a + 2];
        for (int c = 0; c < 3; ++c) T[3 * a + c] = w0 * Vi[c] + w1 * Vi[3 + c] + w2 * Vi[6 + c];
      }
    }
  __syncthreads();  // (the other lanes' T_b, through global memory)
  if (!in || !pd) return;
  // acc = sum_a T_a^T (sum_b Sigma[a, b] T_b): lane s the slots a = s, s + lanes, ..., b in slot order
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int qa = beg + lane; qa < end; qa += kCovPtLanes) {
    const int ca = b.p_cam[qa];
    if (ca < 0) continue;
    double M[18];
    for (int i = 0; i < 18; ++i) M[i] = 0.0;
    for (int qb = beg; qb < end; ++qb) {
      const int cb = b.p_cam[qb];
      if (cb < 0) continue;
      const double* Tb = Tbuf + 18 * (long)qb;
      const double* Sab = Sig + (long)(6 * ca) * n + 6 * cb;
      for (int r = 0; r < 6; ++r)
        for (int k = 0; k < 6; ++k) {
          const double s = Sab[(long)r * n + k];
          for (int c = 0; c < 3; ++c) M[3 * r + c] += s * Tb[3 * k + c];
        }
    }
    const double* Ta = Tbuf + 18 * (long)qa;
    int u = 0;
    for (int i = 0; i < 3; ++i)
      for (int c = i; c < 3; ++c, ++u)
        for (int r = 0; r < 6; ++r) acc[u] += Ta[3 * r + i] * M[3 * r + c];
  }
  for (int i = 0; i < 6; ++i)
    for (int m = 1; m < kCovPtLanes; m <<= 1) acc[i] += __shfl_xor(acc[i], m, 64);
  if (lane == 0) {
    double* out = pt_cov + 9 * (long)j;
    out[0] = Vi[0] + acc[0];
    out[1] = out[3] = Vi[1] + acc[1];
    out[2] = out[6] = Vi[2] + acc[2];
    out[4] = Vi[4] + acc[3];
    out[5] = out[7] = Vi[5] + acc[4];
    out[8] = Vi[8] + acc[5];
  }
}

// Device-resident problems: the blocks go to the caller's arrays only when
// every stage succeeded (ok = 0 leaves them untouched).  n_pt = 0 when the
// landmark stage did not run (its fail word is then still clear).
__global__ __launch_bounds__(kBlock) void cov_commit_kernel(const int* fail, const double* cam_src, double* cam_dst,
                                                            long n_cam, const double* pt_src, double* pt_dst, long n_pt,
                                                            int* ok) {
  const bool good = !fail[0] && !fail[1];
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) *ok = good ? 1 : 0;
  if (!good) return;
  if (cam_dst && i < n_cam) cam_dst[i] = cam_src[i];
  if (pt_dst && i < n_pt) pt_dst[i] = pt_src[i];
}

}  // namespace
