// ba_schur.hpp — part of ba.hip: point blocks and Schur complement in one
// pass over the landmarks.  Kernel: pt_schur_kernel (every instance's fused
// linearisation and the camera assembly riding in its launch come from
// ba_linearize.hpp).  Reads linearize_kernel's obsx / Wo unless it linearises
// itself; leaves the partial tiles that ba_assemble.hpp sums.
#pragma once
#include "ba_types.hpp"
#include "ba_reduce.hpp"
#include "ba_linearize.hpp"

using namespace ba;

namespace {

__device__ __forceinline__ bool chol3(const double* A, double* L) {
  double d0 = A[0];
  if (!(d0 > 0)) return false;
  d0 = sqrt(d0);
  const double l10 = A[3] / d0, l20 = A[6] / d0;
  double d1 = A[4] - l10 * l10;
  if (!(d1 > 0)) return false;
  d1 = sqrt(d1);
  const double l21 = (A[7] - l20 * l10) / d1;
  double d2 = A[8] - l20 * l20 - l21 * l21;
  if (!(d2 > 0)) return false;
  d2 = sqrt(d2);
  L[0] = d0; L[1] = 0; L[2] = 0;
  L[3] = l10; L[4] = d1; L[5] = 0;
  L[6] = l20; L[7] = l21; L[8] = d2;
  return true;
}
__device__ __forceinline__ void fwd3(const double* L, const double* b, double* y) {
  y[0] = b[0] / L[0];
  y[1] = (b[1] - L[3] * y[0]) / L[4];
  y[2] = (b[2] - L[6] * y[0] - L[7] * y[1]) / L[8];
}
__device__ __forceinline__ void bwd3(const double* L, const double* y, double* x) {
  x[2] = y[2] / L[8];
  x[1] = (y[1] - L[7] * x[2]) / L[4];
  x[0] = (y[0] - L[3] * x[1] - L[6] * x[2]) / L[0];
}

// Point blocks and Schur complement in one pass over the landmarks.  A
// workgroup (8 waves) takes sub-chunks of P landmarks; per sub-chunk:
//  (A) a group of 32 lanes per landmark, one CSR slot per lane, every load
//      issued in one round: V = sum V_o, g = sum g_o (after a linearisation;
//      Jacobi scaling at iteration 0; projected-gradient max-norm), then
//      V + D/radius -> Cholesky L_p, z_p = L_p^-1 g_p on every lane of the
//      group (butterfly sums leave the totals on all of them: no staging);
//  (B) each lane writes its slot's entries of the landmark's 3 rows of
//      Y = (Dc W Dp) L_p^-T into LDS (duplicate residual blocks of one camera
//      add in CSR order, no atomics), z_p as the extra column n6 (so Y^T Y
//      also yields Y^T z);
//  (C) S partial tiles D(16x16) += A(16x4) B(4x16) on v_mfma_f64_16x16x4f64
//      (A[i][k] = Y[k][16I+i], B[k][j] = Y[k][16J+j]), one wave per tile,
//      accumulated over all the workgroup's sub-chunks in registers.  A K-step
//      of 4 rows is skipped for a tile when the rows' camera band (a track's
//      cameras are contiguous in CSR order) misses the tile's columns.
// Band-sorted runs (plan_order_kernel): a workgroup takes one run of rlen
// landmarks in (first tile, last tile) order -- landmarks with similar camera
// bands together -- and one group of stpw tiles of the run's tile set (the
// pairs of tiles in its band plus the z tile), so a wave holds at most 5
// accumulator tiles and a run stores only its band's tiles (config 5: ~16 MB
// of partials per iteration instead of 97, config 4: 12 instead of 33).
// Partials (run x tile) are summed in fixed run order by s_assemble through
// the per-tile slot lists: deterministic, no atomics.  Operand map of the MFMA: lane l holds
// A[l&15][l>>4] and B[l>>4][l&15]; result register i holds D[(l>>4)+4i][l&15].
// Landmarks per sub-chunk: 32 (96 rows of Y, 16 lanes per landmark) while the
// Y block fits the LDS budget, else 16 (48 rows, 32 lanes per landmark).  Each
// Schur workgroup leaves one set of partial tiles that s_assemble sums, so
// twice the landmarks per workgroup halve that traffic.
constexpr int kSchurPts = 16, kSchurPtsWide = 32, kSchurPtsSmall = 8;
#ifndef ME_SCHUR_NT
#define ME_SCHUR_NT 5
#endif
constexpr int kSchurNtMax = ME_SCHUR_NT;  // accumulator tiles per wave (3..5)
constexpr size_t kSchurLdsCap = 150 * 1024;
constexpr size_t kSchurLinLds = 8 * 9 * 512;  // fused linearisation: one cell of V_o | g_o sums per thread, behind the Y block
__host__ __device__ inline size_t schur_lds_bytes(int P, int Rz) { return 8 * (size_t)3 * P * Rz + 4 * 3 * (size_t)P; }

// Which pt_schur_kernel<OD, NT, 512, PTS> instances linearise in their phase A
// (host and kernel read the same table).  An instance is fused when the
// compiler's resource report keeps it within 256 VGPRs at 512 threads with no
// more scratch than the unfused instance of the same NT
// (profiles/fused_lin_resources.txt); the others keep the linearize_kernel
// launch in front of them.
// Both models alike: 2 and 3 tiles per wave fit with no scratch; 4 tiles keep
// the unfused instance's 20 B with 16 and 32 landmarks per sub-chunk and take
// 28 B with 8; 5 tiles take 64-84 B against 40-56.
#ifndef ME_SCHUR_FUSED_NT
#define ME_SCHUR_FUSED_NT 4  // most tiles per wave of a fused instance; 0: every instance unfused (A/B builds)
#endif
__host__ __device__ constexpr bool schur_fused_lin(int od, int nt, int pts) {
  return (od == 4 || od == 2) && nt <= ME_SCHUR_FUSED_NT && (nt <= 3 || (nt == 4 && pts != kSchurPtsSmall));
}
__host__ __device__ constexpr int schur_nt(int stpw) {  // the instance's tile count for stpw = 8 waves x tiles
  return stpw / 8 <= 2 ? 2 : stpw / 8 <= 3 ? 3 : stpw / 8 <= 4 ? 4 : 5;
}

#ifdef ME_SCHUR_STAMPS  // timing experiment only (tools/drivers.py schur_stamps): workgroup 0's phase times in st->stamps[6..11]
#define SCHUR_T(i)                                                                     \
  do {                                                                                 \
    if (sblk == 0 && threadIdx.x == 0) {                                               \
      const long long tt_ = (long long)__builtin_amdgcn_s_memtime();                   \
      if ((i) > 0) st->stamps[5 + (i)] += tt_ - sch_prev_;                             \
      sch_prev_ = tt_;                                                                 \
    }                                                                                  \
  } while (0)
#else
#define SCHUR_T(i) \
  do {             \
  } while (0)
#endif
template <int OD, int NT, int BLK, int PTS>
__global__ __launch_bounds__(BLK) void pt_schur_kernel(Geo g, Bufs b, Opts o, CamArgs ca) {
  constexpr int SL = BLK / PTS, NW = BLK / 64;  // lanes per landmark, waves
  constexpr bool FL = schur_fused_lin(OD, NT, PTS);  // phase A linearises (no linearize_kernel launch, no obsx)
  extern __shared__ double smem[];
  __shared__ double red[8];
  // camera-assembly blocks of a fused launch come first: dispatched before the
  // Schur runs, their longer chain (slot loop, 27-value reduce, camera reduce)
  // no longer trails the runs (round 6: the launch 14.8 -> see DESIGN §5.4)
  if (ca.on && (int)blockIdx.x < ca.ncam) {
    if (threadIdx.x >= kBlock) return;
    const int q = blockIdx.x;
    if (q >= g.ncu) return;  // (padding to a multiple of 8)
#ifdef ME_EXP_NOCAM  // timing experiment only (wrong results): the launch without its camera work, DESIGN §5.4's yardstick
    return;
#endif
    cam_assemble_body<OD>(g, b, ca.cpart, 0, ca.colnorm, ca.gc_raw, ca.Uraw, q);  // (this instance's model only)
    return;
  }
  const int sblk = (int)blockIdx.x - (ca.on ? ca.ncam : 0);  // this workgroup's index among the Schur runs
  State* st = b.st;
  if (st->done) return;
#ifdef ME_SCHUR_STAMPS
  long long sch_prev_ = 0;
  if (sblk == 0 && threadIdx.x == 0) st->stamps[12] += 1;
#endif
  SCHUR_T(0);
  const int need_lin = st->need_lin, scaled = st->scaled, cur = st->cur;
  const double* obsx = b.obsx;
  const double* Wo = b.Wo;
  const double radius = st->radius;
  // all allowed steps taken: this pass only evaluates the gradient for the
  // closing test (Ceres HandleSuccessfulStep); no Schur complement is needed
  const bool final_pass = st->iterations >= o.max_num_iterations;
  if (sblk == 0 && threadIdx.x == 0) st->final_pass = final_pass;
  const int P = g.spts, Rz = g.Rpad, rows = 3 * P, nks = rows / 4;
  // this workgroup's run and tile group; the run's tile set is [bA, bB] plus the z tile T - 1
  // Workgroups are dealt round-robin over the 8 XCDs: a run's tile groups sit
  // at blocks b, b + 8, ... so they share an XCD's L2 -- the second group's
  // reads of the run's slots (W, obsx; fused linearisation: the observations)
  // hit the lines the first one fetched.
  const int sup = sblk / (8 * g.sgrp), r8 = sblk - sup * 8 * g.sgrp;
  const int run = 8 * sup + (r8 & 7), tgrp = r8 >> 3;
  if (run >= g.nruns) {  // (uniform) padding of the last block of 8 runs
    if (need_lin && threadIdx.x == 0) b.part[R_GMAX_PT * g.pstride + sblk] = 0.0;
    return;
  }
  const int bA = g.sorted ? b.rband[2 * run] : 0, bB = g.sorted ? b.rband[2 * run + 1] : g.T - 1;
  const int nb = bB - bA + 1, ns = nb + (bB < g.T - 1 ? 1 : 0), ntile = ns * (ns + 1) / 2;
  if (tgrp * g.stpw >= ntile) {  // (uniform) the run's tiles are all taken by lower groups
    if (need_lin && threadIdx.x == 0) b.part[R_GMAX_PT * g.pstride + sblk] = 0.0;
    return;
  }
  const bool lead = tgrp == 0;  // the run's first group writes the per-landmark results (the others recompute them)
  double* Y = smem;
  int* band = reinterpret_cast<int*>(Y + (size_t)rows * Rz);  // per landmark: first / last camera column, live
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gi = tid / SL, gl = tid & (SL - 1);
  // Fused linearisation (flin: this instance, a run of one sub-chunk in
  // landmark order), ahead of everything else the workgroup sets up, so that
  // little is live across it.  The run's landmarks are consecutive, so its CSR
  // slots are one range [s0, s1): thread t takes slot s0 + t -- every lane
  // busy, one pass whatever the track lengths -- and forms the slot's pieces
  // (lin_pieces: linearize_kernel's expressions, the same bits).  W_o goes to
  // b.Wo, where phase B and the later launches (pt_step_kernel, a
  // need_lin == 0 pass) read it; V_o | g_o goes into the LDS cell of the lane
  // that owns the slot in phase A (lane (q - beg) mod SL of the landmark's
  // group), its slots q0, q0 + SL, ... added one round after the other: the
  // order of phase A's obsx loop.  b.obsx is neither written nor read.
  // EVERY tile group of the run does so, lead or not: the groups are
  // workgroups of one launch that nothing orders, so a group never reads what
  // another stored.  Each stores the same bits to the same words of b.Wo (a
  // benign overlap) and reads back only what its own threads stored, behind
  // own_stores_visible() and a workgroup barrier: race-free without any order
  // between the groups.
  // The camera of slot q is p_cam[q] + nf (== cam_idx[p_obs[q]]).
  const bool flin = FL && g.flin && need_lin;
  double* vl = reinterpret_cast<double*>(band + 3 * P);  // flin: [BLK][9], lane t's sum of V_o | g_o over its slots
  __shared__ double cwave[NW];                           // per wave: 0.5 rho0 over its threads' slots
  if constexpr (FL) {
    if (flin) {
      const int j0 = run * g.rlen;
      const int s0 = b.p_off[j0], s1 = b.p_off[min(j0 + P, g.np)];
      double cost = 0;
      for (int base = s0; base < s1; base += BLK) {  // (uniform; one batch unless duplicates pile up)
        const int q = base + tid;
        int k = -1, cell = 0;
        double X[9];
        if (q < s1) {
          const int ob = b.p_obs[q], ci = b.p_cam[q];
          const int j = b.pt_idx[ob];
          const int beg = b.p_off[j];
          double xl[3], w[18];
          for (int a = 0; a < 3; ++a) xl[a] = b.pts[cur][3 * (long)j + a];
          const bool var = ci >= 0 && !final_pass;  // (no W_o for a fixed camera, nor for the closing pass)
          cost += lin_pieces<OD>(g, b, ob, b.cams[cur] + 6 * (ci + g.nf), b.rot[cur] + kRotStride * (ci + g.nf), xl, var,
                                 X, w);
          if (var)
            for (int i = 0; i < 18; ++i) b.Wo[18 * (long)q + i] = w[i];
          k = (q - beg) / SL;
          cell = 9 * ((j - j0) * SL + ((q - beg) & (SL - 1)));
        }
        own_stores_visible();  // (before the barrier: the W_o stores of every wave have landed)
        for (int r = 0;; ++r) {  // round r: the owning lanes' r-th slots, up to the batch's largest k (uniform exit)
          if (k == r)
            for (int i = 0; i < 9; ++i) vl[cell + i] = r == 0 ? X[i] : vl[cell + i] + X[i];
          if (!__syncthreads_or(k > r)) break;
        }
      }
      cost = wave_total(cost);
      if (lane == 0) cwave[wave] = cost;  // (read by thread 0 behind the barriers of the sub-chunk loop)
    }
  }
  // this wave's tiles (wave-uniform: scalar registers): canonical index c of
  // the run's tile set (row ka of the set's upper triangle holds ns - ka pairs)
  int tI[NT], tJ[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    int p = tgrp * g.stpw + wave + NW * u, ka = 0;
    if (p >= ntile) p = -1;
    int rem = p < 0 ? 0 : p;
    while (rem >= ns - ka) {
      rem -= ns - ka;
      ++ka;
    }
    const int kb = ka + rem;
    tI[u] = p < 0 ? -1 : (ka < nb ? bA + ka : g.T - 1);
    tJ[u] = p < 0 ? -1 : (kb < nb ? bA + kb : g.T - 1);
  }
  double4_t acc[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
  double gm = 0;
  for (int sc = 0; sc < g.rsub; ++sc) {
    const int pos = run * g.rlen + sc * P + gi;
    const int j = pos < g.np ? (g.sorted ? b.order[pos] : pos) : g.np;
    double* Yp = Y + (size_t)(3 * gi) * Rz;  // this landmark's 3 rows, written by its own lane group only
    for (int i = gl; i < 3 * Rz / 2; i += SL) reinterpret_cast<double2*>(Yp)[i] = double2{0.0, 0.0};
    if (j < g.np) {
      // (A) every load of the landmark and of this lane's first CSR slot in one round
      const int beg = b.p_off[j], end = b.p_off[j + 1];
      const int q0 = beg + gl;
      int ci0 = -1, cprev0 = -1, cnext0 = -2;
      double w0[18], cs0[6], X0[9];
      for (int i = 0; i < 9; ++i) X0[i] = 0.0;
      if (q0 < end) {
        ci0 = b.p_cam[q0];
        if (q0 > beg) cprev0 = b.p_cam[q0 - 1];
        if (q0 + 1 < end) cnext0 = b.p_cam[q0 + 1];  // duplicate test of phase B, requested with the rest
        if (need_lin && !flin)
          for (int i = 0; i < 9; ++i) X0[i] = obsx[(long)q0 * kObsxStride + i];
        if (ci0 >= 0) {
          for (int i = 0; i < 18; ++i) w0[i] = Wo[18 * (long)q0 + i];
          for (int a = 0; a < 6; ++a) cs0[a] = b.csc[6 * ci0 + a];
        }
      }
      double Vs[9], gs[3], pv[3], xv[3];
      if (need_lin) {
        for (int a = 0; a < 3; ++a) xv[a] = b.pts[cur][3 * (long)j + a];
        if (scaled)
          for (int a = 0; a < 3; ++a) pv[a] = b.psc[3 * (long)j + a];
        double V[9];  // V_o (6 unique) | g_o (3)
        if (flin) {
          for (int i = 0; i < 9; ++i) V[i] = q0 < end ? vl[9 * tid + i] : 0.0;  // (this lane's slots, summed ahead of the set-up)
        } else {
          for (int i = 0; i < 9; ++i) V[i] = X0[i];
          for (int q = q0 + SL; q < end; q += SL)
            for (int i = 0; i < 9; ++i) V[i] += obsx[(long)q * kObsxStride + i];
        }
        SCHUR_T(1);  // loads of phase A issued and returned (first use)
      for (int i = 0; i < 9; ++i) V[i] = group_sum<SL>(V[i]);
        if (!scaled) {
          pv[0] = g.jacobi ? 1.0 / (1.0 + sqrt(V[0])) : 1.0;
          pv[1] = g.jacobi ? 1.0 / (1.0 + sqrt(V[3])) : 1.0;
          pv[2] = g.jacobi ? 1.0 / (1.0 + sqrt(V[5])) : 1.0;
        }
        const double p0 = pv[0], p1 = pv[1], p2 = pv[2];
        Vs[0] = V[0] * p0 * p0; Vs[1] = V[1] * p0 * p1; Vs[2] = V[2] * p0 * p2;
        Vs[3] = Vs[1];          Vs[4] = V[3] * p1 * p1; Vs[5] = V[4] * p1 * p2;
        Vs[6] = Vs[2];          Vs[7] = Vs[5];          Vs[8] = V[5] * p2 * p2;
        gs[0] = V[6] * p0;
        gs[1] = V[7] * p1;
        gs[2] = V[8] * p2;
        if (gl == 0 && lead) {
          if (!scaled)
            for (int a = 0; a < 3; ++a) b.psc[3 * (long)j + a] = pv[a];
          for (int i = 0; i < 9; ++i) b.V[9 * (long)j + i] = Vs[i];
          for (int a = 0; a < 3; ++a) b.gps[3 * (long)j + a] = gs[a];
          for (int a = 0; a < 3; ++a) {
            const double xp = fmin(fmax(xv[a] - V[6 + a], g.lo[a]), g.hi[a]);
            gm = fmax(gm, fabs(xv[a] - xp));
          }
        }
      } else {
        for (int i = 0; i < 9; ++i) Vs[i] = b.V[9 * (long)j + i];
        for (int a = 0; a < 3; ++a) {
          gs[a] = b.gps[3 * (long)j + a];
          pv[a] = b.psc[3 * (long)j + a];
        }
      }
      if (!final_pass) {  // (uniform)
      // point block, redundantly on every lane of the group (the sums are group-uniform)
      double A[9], L[9], z[3];
      for (int i = 0; i < 9; ++i) A[i] = Vs[i];
      for (int a = 0; a < 3; ++a) A[4 * a] += fmin(fmax(Vs[4 * a], o.min_diag), o.max_diag) / radius;
      const bool ok = chol3(A, L);
      fwd3(L, gs, z);
      const double rL0 = 1.0 / L[0], rL4 = 1.0 / L[4], rL8 = 1.0 / L[8];
      if (gl == 0) {
        if (!ok) st->fail = 1;
        if (lead) {
          for (int i = 0; i < 9; ++i) b.Lp[9 * (long)j + i] = L[i];
          for (int a = 0; a < 3; ++a) b.zp[3 * (long)j + a] = z[a];
        }
      }
      SCHUR_T(2);  // group sums, point block
      // (B) this lane's slots -> the landmark's rows of Y (first slot of each camera run only;
      // duplicate residual blocks of one camera are summed in CSR order)
      int lo = 1 << 29, hi = -1;
      for (int q = q0; q < end; q += SL) {
        int ci, cp;
        double w[18], cs[6];
        if (q == q0) {
          ci = ci0;
          cp = cprev0;
          if (ci >= 0) {
            for (int i = 0; i < 18; ++i) w[i] = w0[i];
            for (int a = 0; a < 6; ++a) cs[a] = cs0[a];
          }
        } else {
          ci = b.p_cam[q];
          cp = b.p_cam[q - 1];
          if (ci >= 0) {
            for (int i = 0; i < 18; ++i) w[i] = Wo[18 * (long)q + i];
            for (int a = 0; a < 6; ++a) cs[a] = b.csc[6 * ci + a];
          }
        }
        if (ci < 0) continue;
        lo = min(lo, 6 * ci);
        hi = max(hi, 6 * ci + 5);
        if (cp == ci) continue;  // not the first slot of its camera run
        if (q != q0 || cnext0 == ci)  // (the first slot's next camera came with phase A's loads)
          for (int r = q + 1; r < end && b.p_cam[r] == ci; ++r)
            for (int i = 0; i < 18; ++i) w[i] += Wo[18 * (long)r + i];
        for (int a = 0; a < 6; ++a) {
          const int col = 6 * ci + a;
          const double wa[3] = {w[3 * a] * cs[a] * pv[0], w[3 * a + 1] * cs[a] * pv[1], w[3 * a + 2] * cs[a] * pv[2]};
          double y[3];  // L y = wa with the diagonal reciprocals hoisted out of the slot loop
          y[0] = wa[0] * rL0;
          y[1] = (wa[1] - L[3] * y[0]) * rL4;
          y[2] = (wa[2] - L[6] * y[0] - L[7] * y[1]) * rL8;
          for (int k = 0; k < 3; ++k) Yp[(size_t)k * Rz + col] = y[k];
        }
      }
      lo = group_min<SL>(lo);
      hi = group_max<SL>(hi);
      if (gl == 0) {
        for (int k = 0; k < 3; ++k) Yp[(size_t)k * Rz + g.n6] = z[k];
        band[3 * gi] = lo;
        band[3 * gi + 1] = hi;
        band[3 * gi + 2] = 1;  // z_p (column n6, tile T-1) is live for every landmark
      }
      }  // !final_pass
    } else if (gl == 0) {
      band[3 * gi] = 1 << 29;
      band[3 * gi + 1] = -1;
      band[3 * gi + 2] = 0;
    }
    __syncthreads();
    SCHUR_T(3);  // Y rows in LDS (barrier)
    // (C) partial tiles on the matrix cores.  First the band test of every
    // K-step at once (lane ks of each wave tests step ks, one ballot per tile:
    // wave-uniform hit masks in scalar registers), then the steps run with the
    // next step's operands requested before this step's MFMAs -- no LDS round
    // trip between a step's band test and its operands.
    if (!final_pass) {
      unsigned long long hm[NT];
      {
        int lo = 1 << 29, hi = -1, live = 0;
        if (lane < nks) {
          const int pa = (4 * lane) / 3, pb = min((4 * lane + 3) / 3, P - 1);
          lo = min(band[3 * pa], band[3 * pb]);
          hi = max(band[3 * pa + 1], band[3 * pb + 1]);
          live = band[3 * pa + 2] | band[3 * pb + 2];
        }
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const int I = tI[u], J = tJ[u];
          // a tile is touched by these rows iff both its column blocks meet the camera band or the z column
          const bool hitI = (hi >= 16 * I && lo <= 16 * I + 15) || (live && I == g.T - 1);
          const bool hitJ = (hi >= 16 * J && lo <= 16 * J + 15) || (live && J == g.T - 1);
          hm[u] = __ballot(lane < nks && I >= 0 && hitI && hitJ);
        }
      }
      auto operands = [&](int ks, double* a, double* bb) {
        const double* Yr = Y + (size_t)(4 * ks + (lane >> 4)) * Rz + (lane & 15);
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          const bool h = (hm[u] >> ks) & 1ull;
          a[u] = h ? Yr[16 * tI[u]] : 0.0;
          bb[u] = h ? Yr[16 * tJ[u]] : 0.0;
        }
      };
      auto contract = [&](int ks, const double* a, const double* bb) {
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if ((hm[u] >> ks) & 1ull) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bb[u], acc[u], 0, 0, 0);
      };
      double av[NT], bv[NT];
      if constexpr (NT <= 6) {
        // A few tiles per wave: the K-steps unrolled with ping-pong operand
        // registers, every operand read issued unconditionally (clamped tile
        // index) and only the MFMAs skipped by the band masks.  Straight-line
        // LDS reads let each MFMA wait for its own operands only (lgkmcnt(N));
        // conditional reads made the compiler wait for all of them (lgkmcnt(0)
        // before every step's first MFMA: the next step's reads were never
        // overlapped).  Scheduling barriers keep one step of reads in flight.
        constexpr int NKS = 3 * PTS / 4;
        static_assert(NKS % 2 == 0, "K-steps are taken in pairs");
        int cI[NT], cJ[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
          cI[u] = 16 * max(tI[u], 0);
          cJ[u] = 16 * max(tJ[u], 0);
        }
        const double* Y0 = Y + (size_t)(lane >> 4) * Rz + (lane & 15);
        const size_t kstride = 4 * (size_t)Rz;
        auto reads = [&](const double* Yr, double* a, double* bb) {
#pragma unroll
          for (int u = 0; u < NT; ++u) {
            a[u] = Yr[cI[u]];
            bb[u] = Yr[cJ[u]];
          }
        };
        double an[NT], bn[NT];
        reads(Y0, av, bv);
#pragma unroll 1
        for (int ks = 0; ks < NKS; ks += 2) {
          reads(Y0 + (ks + 1) * kstride, an, bn);
          __builtin_amdgcn_sched_barrier(0);
          contract(ks, av, bv);
          __builtin_amdgcn_sched_barrier(0);
          reads(Y0 + min(ks + 2, NKS - 1) * kstride, av, bv);  // (the last pair re-reads a valid row, unused)
          __builtin_amdgcn_sched_barrier(0);
          contract(ks + 1, an, bn);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
        for (int ks = 0; ks < nks; ++ks) {
          operands(ks, av, bv);
          contract(ks, av, bv);
        }
      }
    }
    __syncthreads();
  }
  SCHUR_T(4);  // MFMA contraction (barrier)
  if (need_lin) {
    const double r = block_max(gm, red);
    if (tid == 0) b.part[R_GMAX_PT * g.pstride + sblk] = r;
    if (flin && lead && tid == 0) {  // the run's cost partial: the wave sums in wave order (g.ncost = nruns partials)
      double c = 0;
      for (int w = 0; w < NW; ++w) c += cwave[w];
      b.part[R_COST * g.pstride + run] = c;
    }
  }
  if (final_pass) return;
#pragma unroll
  for (int u = 0; u < NT; ++u) {
    const int p = tgrp * g.stpw + wave + NW * u;
    if (p >= ntile) continue;
    double* dst = b.Spart + ((long)run * g.npairs + p) * 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[((lane >> 4) + 4 * i) * 16 + (lane & 15)] = acc[u][i];
  }
#ifdef ME_SCHUR_STAMPS
  __builtin_amdgcn_s_waitcnt(0);
#endif
  SCHUR_T(5);  // gradient max + partial stores
}

}  // namespace
