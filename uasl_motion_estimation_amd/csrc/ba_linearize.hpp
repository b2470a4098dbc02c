// ba_linearize.hpp — part of ba.hip: the linearisation and the camera
// assembly.  Kernels: linearize_kernel, cam_assemble_kernel, xch_flags_kernel,
// cam_finish_kernel; lin_pieces and cam_assemble_body also run inside
// pt_schur_kernel (ba_schur.hpp).  Reads the plan's layout and rotation tables
// (ba_plan.hpp) and the residuals of ba_residual.hpp.
#pragma once
#include "ba_types.hpp"
#include "ba_reduce.hpp"
#include "ba_residual.hpp"

using namespace ba;

namespace {

// Per observation: corrected residual / Jacobian, cost, and the unscaled
// per-observation normal-equation pieces W_o = Jc^T Jp (6x3), V_o = Jp^T Jp
// (6 unique), g_o = Jp^T r, so the per-point stage only sums.
// Workgroup size by window: one-wave workgroups spread a small window's
// observations over every CU (config 3: 22k observations = 344 workgroups,
// 13.6 -> 11.0 us), 256 threads for large ones (config 4: 100k observations,
// 34.4 us vs 38.6 with one-wave workgroups)
#ifndef ME_LIN_SMALL
#define ME_LIN_SMALL 64  // linearize workgroup for small windows (A/B builds)
#endif
constexpr int kLinSmall = ME_LIN_SMALL, kLinSmallMaxObs = 64 * 512;
__host__ __device__ inline int lin_block(int no) { return no <= kLinSmallMaxObs ? kLinSmall : kBlock; }
// One observation's pieces at the linearisation point: X = V_o (6 unique) |
// g_o (3), W = W_o (6x3, only when `var`: a variable camera), returns the
// observation's cost 0.5 rho0.  The one definition behind linearize_kernel and
// the fused phase A of pt_schur_kernel: the same expressions, the same bits.
template <int OD>
__device__ __forceinline__ double lin_pieces(const Geo& g, const Bufs& b, long o, const double* cam, const double* rot,
                                             const double* pt, bool var, double* X, double* W) {
  double r[4], Jc[24], Jp[12];
  obs_residual_tab<OD>(g, b, o, cam, rot, pt, r, Jc, Jp);
  const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
  double rho0, sc;
  huber(s, &rho0, &sc);
  for (int k = 0; k < 4; ++k) r[k] *= sc;
  for (int k = 0; k < 24; ++k) Jc[k] *= sc;
  for (int k = 0; k < 12; ++k) Jp[k] *= sc;
  X[0] = Jp[0] * Jp[0] + Jp[3] * Jp[3] + Jp[6] * Jp[6] + Jp[9] * Jp[9];
  X[1] = Jp[0] * Jp[1] + Jp[3] * Jp[4] + Jp[6] * Jp[7] + Jp[9] * Jp[10];
  X[2] = Jp[0] * Jp[2] + Jp[3] * Jp[5] + Jp[6] * Jp[8] + Jp[9] * Jp[11];
  X[3] = Jp[1] * Jp[1] + Jp[4] * Jp[4] + Jp[7] * Jp[7] + Jp[10] * Jp[10];
  X[4] = Jp[1] * Jp[2] + Jp[4] * Jp[5] + Jp[7] * Jp[8] + Jp[10] * Jp[11];
  X[5] = Jp[2] * Jp[2] + Jp[5] * Jp[5] + Jp[8] * Jp[8] + Jp[11] * Jp[11];
  for (int a = 0; a < 3; ++a) X[6 + a] = Jp[a] * r[0] + Jp[3 + a] * r[1] + Jp[6 + a] * r[2] + Jp[9 + a] * r[3];
  // (the camera normal-equation pieces are formed by cam_assemble from the
  // same residual and Jacobian: no 216 B per observation through HBM)
  if (var)
    for (int a = 0; a < 6; ++a)
      for (int c = 0; c < 3; ++c)
        W[a * 3 + c] = Jc[a] * Jp[c] + Jc[6 + a] * Jp[3 + c] + Jc[12 + a] * Jp[6 + c] + Jc[18 + a] * Jp[9 + c];
  return 0.5 * rho0;
}

// The separate linearisation launch: the Schur instances that do not
// linearise in their phase A (schur_fused_lin) read its obsx / Wo.
template <int OD, int BLK>
__global__ __launch_bounds__(BLK) void linearize_kernel(Geo g, Bufs b) {
  __shared__ double lds[BLK / 64];
  const State* st = b.st;
  if (st->done || !st->need_lin) return;
  const int o = blockIdx.x * BLK + threadIdx.x;
  double cost = 0;
  if (o < g.no) {
    const int cur = st->cur;
    const int ci = b.cam_idx[o], pi = b.pt_idx[o];
    const long slot = b.pos[o];  // CSR-by-point slot: per-point stages read contiguously
    // (the pieces go straight to their slot of obsx / Wo)
    cost = lin_pieces<OD>(g, b, o, b.cams[cur] + 6 * ci, b.rot[cur] + kRotStride * ci, b.pts[cur] + 3 * pi, ci - g.nf >= 0,
                          b.obsx + slot * kObsxStride, b.Wo + 18 * slot);
  }
  double v[1] = {cost};
  double out[1];
  block_sum<1>(v, out, lds);
  if (threadIdx.x == 0) b.part[R_COST * g.pstride + blockIdx.x] = out[0];
}

// Unscaled U = Jc^T Jc (21 unique) and g = Jc^T r per variable camera, in
// two deterministic stages (cam_assemble_body): a workgroup sums one unit
// (256 slots of one camera, the plan's unit table) into a partial; cam_reduce
// adds the camera's partials in unit order.

// Camera ci: lane u < 27 sums component u of the camera's partials, units
// first .. first + count - 1 (fixed order)
// -> raw U, column norms, raw gradient; unless sharded, the Jacobi scaling
// (iteration 0) and the scaled blocks.  Called by every thread of a block.
__device__ void cam_reduce_body(const Geo& g, const Bufs& b, int sharded, const double* cpart, double* colnorm,
                                double* gc_raw, double* Uraw, int ci, int first, int count) {
  __shared__ double tot[27];
  __shared__ double csl[6];
  const State* st = b.st;
  const int u = threadIdx.x;
  if (u < 27) {
    double sum = 0.0;
    for (int k = 0; k < count; ++k) sum += a_ld<true>(&cpart[27 * ((long)first + k) + u]);  // (written through)
    tot[u] = sum;
    if (u < 21) Uraw[21 * (long)ci + u] = sum;
    else gc_raw[6 * ci + u - 21] = sum;
  }
  __syncthreads();
  if (u < 6) {
    const int d = u * 6 - u * (u - 1) / 2;  // index of (u, u) in the packed upper triangle
    colnorm[6 * ci + u] = tot[d];
    if (!sharded) {
      double* cs = b.csc + 6 * ci;
      if (!st->scaled) cs[u] = g.jacobi ? 1.0 / (1.0 + sqrt(tot[d])) : 1.0;
      csl[u] = cs[u];
    }
  }
  if (sharded) return;
  __syncthreads();
  if (u < 21) {
    int a = 0, r = u;
    while (r >= 6 - a) {
      r -= 6 - a;
      ++a;
    }
    const int c = a + r;
    const double x = tot[u] * csl[a] * csl[c];
    double* U = b.U + 36 * (long)ci;
    U[a * 6 + c] = x;
    U[c * 6 + a] = x;
  } else if (u < 27) {
    b.gcs[6 * ci + u - 21] = tot[u] * csl[u - 21];
  }
}

// Unscaled U = Jc^T Jc (21 unique) and g = Jc^T r per variable camera, in
// two deterministic stages over the camera's observations in c_obs slot
// order (each piece formed here from the observation's residual and
// Jacobian): the workgroup of unit un sums the unit's slots (at most 256,
// one per thread) into a partial; the last of a camera's workgroups to
// finish adds the camera's partials in unit order.  Every workgroup makes
// one pass whatever its camera's share of the observations (a sliding
// window's newest cameras see five times the oldest's), and a unit past the
// plan's unit total (the host launches a bound) returns at once.
// Threads 0 .. kBlock-1 of the block take part (in a wider block the other
// waves have exited: barriers count only live waves).
#ifdef ME_CAM_TS  // timing experiment only: phase split of one unit's assembly workgroup (me_cam_ts_unit; 0 = camera 0's first), s_memtime ticks
__device__ unsigned long long g_cam_ts[8];
__device__ int g_cam_ts_unit;
#define CAM_T(i)                                                                           \
  do {                                                                                     \
    if (un == g_cam_ts_unit && threadIdx.x == 0) {                                         \
      const long long t_ = (long long)__builtin_amdgcn_s_memtime();                        \
      if ((i) > 0) atomicAdd(&g_cam_ts[(i)], (unsigned long long)(t_ - cam_prev_));        \
      else atomicAdd(&g_cam_ts[0], 1ull);                                                  \
      cam_prev_ = t_;                                                                      \
    }                                                                                      \
  } while (0)
#else
#define CAM_T(i) \
  do {           \
  } while (0)
#endif
template <int OD>
__device__ __forceinline__ void cam_assemble_body(const Geo& g, const Bufs& b, double* cpart, int sharded,
                                                  double* colnorm, double* gc_raw, double* Uraw, int un) {
  __shared__ double rows[kBlock / 16 * 27];
  const State* st = b.st;
  // (the unit's entry is requested beside the state words: one round)
  const int4 ue = *(const int4*)(b.cunit + (long)kCuStride * un);  // camera, slot range, the camera's unit count
  const int ufirst = b.cunit[(long)kCuStride * un + CU_FIRST];
  if (st->done || !st->need_lin) return;
  const int ci = ue.x;
  if (ci < 0) return;  // past the plan's unit total
#ifdef ME_CAM_TS
  long long cam_prev_ = 0;
#endif
  CAM_T(0);
  double v[27];
  for (int i = 0; i < 27; ++i) v[i] = 0;
  const int cur = st->cur;
  const int q = ue.y + threadIdx.x;
  if (q < ue.z) {
    // the observation's residual and Jacobian at the linearisation point, as
    // linearize_kernel forms them (same function, same Huber scaling: the same
    // pieces bit for bit), then Jc^T Jc (21) and Jc^T r (6)
    const int o = b.c_obs[q];
    // (the unit's camera: variable camera ci of the window, the same for every
    // slot of the unit, so its parameters and table entry load once per wave)
    const int cam = ci + g.nf, pi = b.pt_idx[o];
    double r[4], Jc[24], Jp[12];
    obs_residual_tab<OD>(g, b, o, b.cams[cur] + 6 * cam, b.rot[cur] + kRotStride * cam, b.pts[cur] + 3 * pi, r, Jc, Jp);
    const double s2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
    double rho0, sc;
    huber(s2, &rho0, &sc);
    for (int kk = 0; kk < 4; ++kk) r[kk] *= sc;
    for (int kk = 0; kk < 24; ++kk) Jc[kk] *= sc;
    int u = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c, ++u)
        v[u] += Jc[a] * Jc[c] + Jc[6 + a] * Jc[6 + c] + Jc[12 + a] * Jc[12 + c] + Jc[18 + a] * Jc[18 + c];
    for (int a = 0; a < 6; ++a) v[21 + a] += Jc[a] * r[0] + Jc[6 + a] * r[1] + Jc[12 + a] * r[2] + Jc[18 + a] * r[3];
  }
  CAM_T(1);
  // the 27 sums: 16-lane row sums by DPP (VALU only), the 16 row sums of the
  // block through LDS, thread u < 27 adds component u's in row order (round 6:
  // 4.2 -> see DESIGN §5.4 us; six dependent lane-shuffle rounds per value before)
#pragma unroll
  for (int u = 0; u < 27; ++u) {
    double x = v[u];
    x += dpp_f64<kDppQuadSwap1>(x);
    x += dpp_f64<kDppQuadSwap2>(x);
    x += dpp_f64<kDppRowHalfMirror>(x);
    x += dpp_f64<kDppRowMirror>(x);
    v[u] = x;
  }
  if ((threadIdx.x & 15) == 0)
#pragma unroll
    for (int u = 0; u < 27; ++u) rows[(threadIdx.x >> 4) * 27 + u] = v[u];
  __syncthreads();
  CAM_T(2);
  if (threadIdx.x < 27) {  // written through for the last of the camera's workgroups (no release per arrival)
    double sum = 0.0;
#pragma unroll
    for (int r = 0; r < kBlock / 16; ++r) sum += rows[r * 27 + threadIdx.x];
    a_st<true>(&cpart[27 * (long)un + threadIdx.x], sum);  // (lanes of wave 0: its vmcnt drain covers them)
  }
  const bool last = last_arrival_wt(b.cnt + ci, (unsigned)ue.w);
  CAM_T(3);
  if (!last) return;
  cam_reduce_body(g, b, sharded, cpart, colnorm, gc_raw, Uraw, ci, ufirst, ue.w);
  CAM_T(4);
#ifdef ME_CAM_TS
  if (un == g_cam_ts_unit && threadIdx.x == 0) atomicAdd(&g_cam_ts[5], 1ull);
#endif
}

// grid: g.ncu units (the host's bound on the plan's unit total)
__global__ __launch_bounds__(kBlock) void cam_assemble_kernel(Geo g, Bufs b, double* cpart, int sharded,
                                                              double* colnorm, double* gc_raw, double* Uraw) {
  // (one instance per model: the mono model's row selection would otherwise
  // keep the stereo path's Jacobian arrays out of registers)
  if (g.od == 4)
    cam_assemble_body<4>(g, b, cpart, sharded, colnorm, gc_raw, Uraw, blockIdx.x);
  else
    cam_assemble_body<2>(g, b, cpart, sharded, colnorm, gc_raw, Uraw, blockIdx.x);
}

// Camera assembly riding in the Schur launch (iterations after the first,
// when the Jacobi scaling is fixed and the two passes are independent).
struct CamArgs {
  double *cpart, *colnorm, *gc_raw, *Uraw;
  int on;
  int ncam;  // leading workgroups of the launch that assemble cameras (g.ncu units, padded to whole rounds of 8 XCDs)
};

// Sharded mode, first linearisation: the rank's input flags (bad index,
// infeasible start) ride behind the column norms in the first exchange, so
// every rank ends the solve alike (each rank only checks its own landmarks).
__global__ void xch_flags_kernel(Geo g, Bufs b, double* colnorm) {
  colnorm[g.n6] = b.st->bad_input ? 1.0 : 0.0;
  colnorm[g.n6 + 1] = b.st->infeasible ? 1.0 : 0.0;
}

// Sharded mode: scaling from the all-reduced column norms, then scale the
// (local) U / g blocks.
__global__ void cam_finish_kernel(Geo g, Bufs b, const double* colnorm, const double* gc_raw, const double* Uraw,
                                  int first) {
  State* st = b.st;
  if (first) {  // (colnorm[n6 ..] = the all-reduced input flags; read before any thread returns)
    const bool bad = colnorm[g.n6] != 0.0, infeasible = colnorm[g.n6 + 1] != 0.0;
    __syncthreads();
    if (bad || infeasible) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->bad_input = bad;
        st->infeasible = infeasible;
        st->done = 1;
        st->termination = 2;
      }
      return;
    }
  }
  if (st->done || !st->need_lin) return;
  const int ci = blockIdx.x * blockDim.x + threadIdx.x;
  if (ci >= g.m) return;
  double* cs = b.csc + 6 * ci;
  if (!st->scaled)
    for (int a = 0; a < 6; ++a) cs[a] = g.jacobi ? 1.0 / (1.0 + sqrt(colnorm[6 * ci + a])) : 1.0;
  const double* Ur = Uraw + 21 * (long)ci;
  double* U = b.U + 36 * (long)ci;
  int u = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c, ++u) {
      const double x = Ur[u] * cs[a] * cs[c];
      U[a * 6 + c] = x;
      U[c * 6 + a] = x;
    }
  for (int a = 0; a < 6; ++a) b.gcs[6 * ci + a] = gc_raw[6 * ci + a] * cs[a];
}

}  // namespace
