// ba_step.hpp — part of ba.hip: point back-substitution, the candidate
// parameters and the LM step decision.  Kernels: pt_step_kernel,
// decide_kernel.  Reads the camera step of ba_cam_solve.hpp and the point
// blocks of ba_schur.hpp.
#pragma once
#include "ba_types.hpp"
#include "ba_reduce.hpp"
#include "ba_residual.hpp"
#include "ba_schur.hpp"

using namespace ba;

namespace {

// Point back-substitution and step evaluation, 16 lanes per point (one
// launch for what were three: per-slot W^T Dc y_c, per-point solve, per-
// observation model change / candidate cost).  The lanes of a point take its
// CSR slots round-robin; the slot sums are reduced across the 16 lanes, every
// lane then solves the point's 3x3 system redundantly (no broadcast), and
// each lane evaluates the model cost change and the candidate cost of its own
// observations.  Partials per workgroup, reduced in fixed order by
// step_finalize (deterministic).
// Step partials -> scal (fixed order).  In single-GPU mode the same workgroup
// then runs the Ceres step handling (decide); in sharded mode the host
// all-reduces scal between step_partials and a decide-only launch.
// R_COUNT of a step whose camera solve hit a hand-off timeout: summed over
// the ranks it stays >= kSpinFlag, so every rank of a sharded solve ends at
// the same iteration with spin_err (ME_ERR_STATE) -- no rank is left waiting
// in a collective the others no longer issue.
constexpr double kSpinFlag = 65536.0;

// The Ceres step handling on a State-like object (the device State itself,
// or the finalizing thread's register copy) and the reduced step scalars.
template <class S>
__device__ __forceinline__ void decide_t(S& st, const double* scal, const Opts& o) {
  st.accepted = 0;
  if (scal[R_COUNT] >= kSpinFlag) {
    st.spin_err = 1;
    st.done = 1;
    st.termination = 2;
    return;
  }
  const double model_change = scal[R_MODEL];
  const bool fail = st.fail || scal[R_COUNT] != 0.0;
  st.fail = 0;  // consumed: the next iteration starts clean
  if (fail || !(model_change > 0.0)) {
    st.invalid_count += 1;
    if (st.invalid_count >= o.max_invalid) {
      st.done = 1;
      st.termination = 2;
      return;
    }
    st.radius = st.radius / st.decrease;
    st.decrease *= 2.0;
    return;
  }
  st.invalid_count = 0;
  const double cand_cost = scal[R_CAND];
  const double step_norm = sqrt(scal[R_STEP2] + st.cam_step2);
  const double x_norm = sqrt(scal[R_XN2] + st.cam_xn2);
  st.cand_cost = cand_cost;
  st.model_change = model_change;
  if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) {
    st.done = 1;
    st.termination = 0;
    return;
  }
  if (fabs(st.x_cost - cand_cost) <= o.function_tolerance * st.x_cost) {
    st.done = 1;
    st.termination = 0;
    return;
  }
  const double q = (st.x_cost - cand_cost) / model_change;
  st.last_q = q;
  if (q > o.min_rel_decrease) {
    st.cur = 1 - st.cur;
    st.x_cost = cand_cost;
    st.successful += 1;
    st.accepted = 1;
    const double t = 2.0 * q - 1.0;
    st.radius = st.radius / fmax(1.0 / 3.0, 1.0 - pow(t, 3.0));
    st.radius = fmin(o.max_radius, st.radius);
    st.decrease = 2.0;
    st.need_lin = 1;
  } else {
    st.radius = st.radius / st.decrease;
    st.decrease *= 2.0;
  }
}

// The end of a solve whose closing linearisation is not queued
// (Opts::close_in_decide), behind decide_t on every one of its returns: the
// iteration-limit test the closing lin_finalize would have run at the head of
// iteration max_num_iterations + 1 (ahead of the minimum-radius test, as
// there).  A solve decide_t itself ended keeps its termination.
template <class S>
__device__ __forceinline__ void close_t(S& st, const Opts& o) {
  if (o.close_in_decide && !st.done && st.iterations >= o.max_num_iterations) {
    st.done = 1;
    st.termination = 1;
  }
}

__device__ void decide(Bufs& b, const Opts& o) {
  decide_t(*b.st, b.scal, o);
  close_t(*b.st, o);
}

// The fields decide_t reads or writes, loaded by the finalizing thread in one
// round before the partial reduce (round 6: the decision's dependent State
// loads were half of the step's finalize tail, ME_STEP_TS)
struct DecideState {
  int cur, need_lin, done, termination, successful, invalid_count, fail, accepted, spin_err;
  int iterations;  // (read only: close_t)
  double radius, decrease, x_cost, cand_cost, model_change, cam_step2, cam_xn2, cam_model, last_q;
  __device__ __forceinline__ void load(const State* st) {
    cur = st->cur; need_lin = st->need_lin; done = st->done; termination = st->termination;
    iterations = st->iterations;
    successful = st->successful; invalid_count = st->invalid_count; fail = st->fail; accepted = st->accepted;
    spin_err = st->spin_err; radius = st->radius; decrease = st->decrease; x_cost = st->x_cost;
    cand_cost = st->cand_cost; model_change = st->model_change; last_q = st->last_q;
    // (written through by this launch's camera workgroup, cam_step_body)
    cam_step2 = a_ld<true>(&st->cam_step2);
    cam_xn2 = a_ld<true>(&st->cam_xn2);
    cam_model = a_ld<true>(&st->cam_model);
  }
  __device__ __forceinline__ void store(State* st) const {
    st->cur = cur; st->need_lin = need_lin; st->done = done; st->termination = termination;
    st->successful = successful; st->invalid_count = invalid_count; st->fail = fail; st->accepted = accepted;
    st->spin_err = spin_err; st->radius = radius; st->decrease = decrease; st->x_cost = x_cost;
    st->cand_cost = cand_cost; st->model_change = model_change; st->last_q = last_q;
  }
};

#ifdef ME_STEP_TS  // timing experiment only: phase split of pt_step workgroup 0 (and of the finalizing workgroup)
__device__ unsigned long long g_step_ts[12];
#define STEP_T(i)                                                                          \
  do {                                                                                     \
    if (blockIdx.x == 0 && threadIdx.x == 0) {                                             \
      const long long t_ = (long long)__builtin_amdgcn_s_memtime();                        \
      if ((i) > 0) atomicAdd(&g_step_ts[(i)], (unsigned long long)(t_ - step_prev_));      \
      else atomicAdd(&g_step_ts[0], 1ull);                                                 \
      step_prev_ = t_;                                                                     \
    }                                                                                      \
  } while (0)
#define STEP_FIN_T(i)                                                                      \
  do {                                                                                     \
    if (threadIdx.x == 0) {                                                                \
      const long long t_ = (long long)__builtin_amdgcn_s_memtime();                        \
      atomicAdd(&g_step_ts[(i)], (unsigned long long)(t_ - fin_prev_));                    \
      fin_prev_ = t_;                                                                      \
    }                                                                                      \
  } while (0)
#else
#define STEP_T(i) \
  do {            \
  } while (0)
#define STEP_FIN_T(i) \
  do {                \
  } while (0)
#endif
__device__ void step_finalize_body(const Geo& g, Bufs b, const Opts& o, int do_decide) {
  __shared__ double rows[1024 / 16 * 4];
  State* st = b.st;
#ifdef ME_STEP_TS
  long long f0 = (long long)__builtin_amdgcn_s_memtime();
#endif
  // the decision's State fields, requested with the partials (one round)
  DecideState ds;
  if (threadIdx.x == 0) ds.load(st);
  double v[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < g.nblk_step; i += blockDim.x) {  // (written through by pt_step's workgroups)
    v[0] += a_ld<true>(&b.part[R_MODEL * g.pstride + i]);
    v[1] += a_ld<true>(&b.part[R_CAND * g.pstride + i]);
    v[2] += a_ld<true>(&b.part[R_STEP2 * g.pstride + i]);
    v[3] += a_ld<true>(&b.part[R_XN2 * g.pstride + i]);
  }
#ifdef ME_STEP_TS
  if (threadIdx.x == 0) {
    const long long t_ = (long long)__builtin_amdgcn_s_memtime();
    atomicAdd(&g_step_ts[8], (unsigned long long)(t_ - f0));
    f0 = t_;
  }
#endif
  // the block's sums: 16-lane row sums by DPP, then the rows in order (VALU and
  // one LDS round; round 6: six lane-shuffle rounds per value before)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    double x = v[u];
    x += dpp_f64<kDppQuadSwap1>(x);
    x += dpp_f64<kDppQuadSwap2>(x);
    x += dpp_f64<kDppRowHalfMirror>(x);
    x += dpp_f64<kDppRowMirror>(x);
    v[u] = x;
  }
  if ((threadIdx.x & 15) == 0)
#pragma unroll
    for (int u = 0; u < 4; ++u) rows[(threadIdx.x >> 4) * 4 + u] = v[u];
  __syncthreads();
#ifdef ME_STEP_TS
  if (threadIdx.x == 0) {
    const long long t_ = (long long)__builtin_amdgcn_s_memtime();
    atomicAdd(&g_step_ts[9], (unsigned long long)(t_ - f0));
    f0 = t_;
  }
#endif
  if (threadIdx.x == 0) {
    double out[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < (int)(blockDim.x >> 4); ++r)
#pragma unroll
      for (int u = 0; u < 4; ++u) out[u] += rows[r * 4 + u];
    double scal[R_COUNT + 1];
    scal[R_MODEL] = out[0] + ds.cam_model;  // (+ this rank's camera part, cam_solve)
    scal[R_CAND] = out[1];
    scal[R_STEP2] = out[2];
    scal[R_XN2] = out[3];
    scal[R_COUNT] = ds.fail ? (ds.spin_err ? kSpinFlag : 1.0) : 0.0;
    for (int k = R_MODEL; k <= R_COUNT; ++k) b.scal[k] = scal[k];
    if (do_decide) {
      decide_t(ds, scal, o);
      close_t(ds, o);
      ds.store(st);
    }
#ifdef ME_STEP_TS
    atomicAdd(&g_step_ts[10], (unsigned long long)((long long)__builtin_amdgcn_s_memtime() - f0));
#endif
  }
}

// (64-thread workgroups measured slower: 17.2 -> 21.6 us at config 3, the
// last arrival then reduces 4x the partials)
// (Measured and dropped, round 4 as in rounds 2-3: the step linearising
// speculatively at its candidate into a second obsx / Wo set, removing the
// linearize launch of every accepted step -- the step went 15.1 -> 28.7 us
// for 9.3 us saved; config 3 BA 0.821 -> 0.894 ms per 10 iterations.)
constexpr int kStepG = 16, kStepBlock = 256, kStepPts = kStepBlock / kStepG;

// Model cost change in the normal-equation form (Ceres computes
// -(J dx).(r + J dx / 2) per residual block; summed over the blocks that is
// -(g.dx + dx^T J^T J dx / 2) with g = J^T r): per point, in the scaled space,
// -(g_p.y_p + y_p^T V_p y_p / 2 + (D_p y_p).sum_q W_q^T (D_c y_c)) -- the last
// sum is the one the point's back-substitution forms anyway -- and per camera
// -(g_c.y_c + y_c^T U_c y_c / 2) (cam_solve).  The same quantity as the
// per-observation form (rounding aside), without the per-observation Jacobian
// traffic (320 B / observation written by linearize and read here before).

// Candidate camera parameter: x + D_c y_c (ys = csc * yc), never contracted
// into an FMA, so the camera workgroup's stored candidate and the point
// workgroups' own copies agree bit for bit.
__device__ __forceinline__ double cam_cand(double x, double ys) {
#pragma clang fp contract(off)
  return x + ys;
}

// The camera workgroup of pt_step (the last one): the candidate cameras and the
// camera part of the step's scalars, |dx_c|^2, |x_c|^2 and the model change
// -(g_c.y_c + y_c^T U_c y_c / 2) in the scaled space.  Round 6: this was the
// camera solve's tail, on its one workgroup's serial path (1.7 us per
// iteration at config 3, tools/drivers.py solve_ts); here it runs beside the
// points.  The scalars are written through: this launch's finalizing workgroup
// reads them (DecideState::load).
__device__ void cam_step_body(const Geo& g, const Bufs& b, int cur, double* lds) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n = g.n6, ncp = 6 * g.nc, f6 = 6 * g.nf;
  const double* x = b.cams[cur];
  double* xc = b.cams[1 - cur];
  double s2 = 0.0, xn2 = 0.0, cm = 0.0;
  for (int i = tid; i < ncp; i += nt) {
    const double xi = x[i];
    if (i < f6) {  // fixed camera
      xc[i] = xi;
      continue;
    }
    const double v = cam_cand(xi, b.csc[i - f6] * b.yc[i - f6]);
    xc[i] = v;
    const double dd = v - xi;
    s2 += dd * dd;
    xn2 += xi * xi;
  }
  for (int r = tid; r < n; r += nt) {
    const double* U = b.U + 36 * (long)(r / 6) + 6 * (r % 6);
    const double* y = b.yc + (r - r % 6);
    const double yr = b.yc[r];
    double uy = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) uy += U[k] * y[k];
    cm += b.gcs[r] * yr + 0.5 * yr * uy;
  }
  double v3[3] = {s2, xn2, -cm}, out[3];
  block_sum<3>(v3, out, lds);
  if (tid == 0) {
    a_st<true>(&b.st->cam_step2, out[0]);
    a_st<true>(&b.st->cam_xn2, out[1]);
    a_st<true>(&b.st->cam_model, out[2]);
  }
}

// The candidates' rotation table, rot[1 - cur] beside cams[1 - cur], which the
// next launches read if the step is accepted (a rejected step leaves cur and
// rot[cur] alone).  The thread of camera c forms the candidate rotation itself
// (cam_cand: the bits cam_step_body stored), so it waits for no store; a fixed
// camera's entry is copied.  The camera workgroup runs this AFTER its arrival
// (pt_step_kernel), with the `cur` it read before: the chain (sqrt, sin, cos,
// ten divisions) then runs beside the point workgroups still at work and the
// finalizing workgroup, which read neither table, and nothing it reads
// (cams[cur], csc, yc) is written by them.  Ahead of the arrival it lengthened
// the launch by 0.5 us (profiles/rot_tables_kernel_stats.txt).
__device__ void rot_step_body(const Geo& g, const Bufs& b, int cur) {
  const double* x = b.cams[cur];
  const double* rx = b.rot[cur];
  double* rc = b.rot[1 - cur];
  for (int c = threadIdx.x; c < g.nc; c += blockDim.x) {
    if (c < g.nf) {
      for (int k = 0; k < kRotStride; ++k) rc[kRotStride * c + k] = rx[kRotStride * c + k];
      continue;
    }
    double aa[3];
    for (int a = 0; a < 3; ++a) {
      const int i = 6 * (c - g.nf) + 3 + a;
      aa[a] = cam_cand(x[6 * c + 3 + a], b.csc[i] * b.yc[i]);
    }
    rot_entry(aa, rc + kRotStride * c);
  }
}

// Grid: g.nblk_step point workgroups + the camera workgroup (cam_step_body,
// then rot_step_body behind its arrival; not in the last iteration of a solve
// that queues no closing linearisation, Opts::close_in_decide).
template <int OD>
__global__ __launch_bounds__(kStepBlock) void pt_step_kernel(Geo g, Bufs b, Opts o, int do_decide) {
  __shared__ double lds[16];
  const State* st = b.st;
  // the camera solve's roster, re-armed for the next iteration's solve (every
  // workgroup of the solve launch, late joiners included, has finished)
  if (blockIdx.x == 0 && threadIdx.x < 2) b.roster[threadIdx.x] = 0u;
  if (st->done) return;
#ifdef ME_STEP_TS
  long long step_prev_ = 0, fin_prev_ = 0;
#endif
  // (the camera workgroup: a failed solve wrote no step, so no candidate and no
  // table; read here, before the arrival -- the finalizing workgroup's decide
  // flips cur and clears fail)
  const bool cam_wg = (int)blockIdx.x == g.nblk_step && !st->fail;
  const int cam_cur = st->cur;
  // (the last iteration of a solve without a closing linearisation: nothing reads the candidates' table)
  const bool rot_wg = cam_wg && !(o.close_in_decide && st->iterations >= o.max_num_iterations);
  if ((int)blockIdx.x == g.nblk_step) {
    // (thread 0's scalar stores drain before its arrival, last_arrival_wt)
    if (cam_wg) cam_step_body(g, b, cam_cur, lds);
  } else {
  STEP_T(0);
  const int gl = threadIdx.x & (kStepG - 1);
  const int j = blockIdx.x * kStepPts + (threadIdx.x / kStepG);
  double mc = 0, cc = 0, s2 = 0, xn2 = 0;
  if (j < g.np && !st->fail) {  // uniform within a 16-lane group
    // Every load of the point and of this lane's first CSR slot, and the
    // second slot's but W, is requested in three dependent rounds (point data
    // + offsets | slot: camera, obs index, W | camera step / scales,
    // observation, candidate camera) before any arithmetic; further slots
    // (points with more than 32 observations) load in the loops.  The slot's
    // camera is p_cam + nf (plan_segsort_kernel writes p_cam[q] =
    // cam_idx[p_obs[q]] - nf), so the candidate camera does not wait for a
    // cam_idx read.
    const int cur = st->cur;
    const double* Wo = b.Wo;
    double psv[3], gpv[3], Lv[9], xv[3], Vv[9];
    for (int a = 0; a < 3; ++a) {
      psv[a] = b.psc[3 * (long)j + a];
      gpv[a] = b.gps[3 * (long)j + a];
      xv[a] = b.pts[cur][3 * (long)j + a];
    }
    for (int i = 0; i < 9; ++i) {
      Lv[i] = b.Lp[9 * (long)j + i];
      Vv[i] = b.V[9 * (long)j + i];
    }
    const int beg = b.p_off[j], end = b.p_off[j + 1];
    const int q0 = beg + gl;
    const bool has0 = q0 < end;
    int ci0 = -1, o0 = 0;
    double W0[18];
    if (has0) {
      ci0 = b.p_cam[q0];
      o0 = b.p_obs[q0];
      for (int i = 0; i < 18; ++i) W0[i] = Wo[18 * (long)q0 + i];  // (unused for a fixed camera)
    }
    // the lane's second slot (tracks of 17 .. 32 observations: 13.5 % of the
    // config-3 window's, in 93 % of its workgroups) is requested in the same
    // rounds, all but its W: loop (3)'s second pass waits for no load of its
    // own and loop (1)'s only for W, already addressed.  (W too costs 36
    // registers and the second wave per SIMD: config 4 +2.7 us)
    const int q1 = q0 + kStepG;
    const bool has1 = q1 < end;
    int ci1 = -1, o1 = 0;
    if (has1) {
      ci1 = b.p_cam[q1];
      o1 = b.p_obs[q1];
    }
    // candidate cameras x + D_c y_c formed here from the current ones (the
    // camera workgroup stores the same values, cam_cand; not read back)
    const double* cams_x = b.cams[cur];
    double ys0[6], f0[4];
    int cam0 = 0, right0 = 0;
    if (has0) {
      if (ci0 >= 0)
        for (int a = 0; a < 6; ++a) ys0[a] = b.csc[6 * ci0 + a] * b.yc[6 * ci0 + a];
      cam0 = ci0 + g.nf;
      for (int k = 0; k < OD; ++k) f0[k] = b.obs[(long)OD * o0 + k];
      if (OD == 2) right0 = b.cam_id[o0] != 0;
    }
    double ys1[6], f1[4];
    int cam1 = 0, right1 = 0;
    if (has1) {
      if (ci1 >= 0)
        for (int a = 0; a < 6; ++a) ys1[a] = b.csc[6 * ci1 + a] * b.yc[6 * ci1 + a];
      cam1 = ci1 + g.nf;
      for (int k = 0; k < OD; ++k) f1[k] = b.obs[(long)OD * o1 + k];
      if (OD == 2) right1 = b.cam_id[o1] != 0;
    }
    double cv0[6], cv1[6];
    if (has0)
      for (int a = 0; a < 6; ++a) {
        const double xa = cams_x[6 * cam0 + a];
        cv0[a] = ci0 >= 0 ? cam_cand(xa, ys0[a]) : xa;
      }
    if (has1)
      for (int a = 0; a < 6; ++a) {
        const double xa = cams_x[6 * cam1 + a];
        cv1[a] = ci1 >= 0 ? cam_cand(xa, ys1[a]) : xa;
      }
    STEP_T(1);  // (the first round of loads issued; returns at first use below)
    // (1) sum over the point's slots of W_q^T (Dc y_c)
    double t[3] = {0.0, 0.0, 0.0};
    for (int q = q0; q < end; q += kStepG) {
      const bool first = q == q0, second = q == q1;
      const int ci = first ? ci0 : second ? ci1 : b.p_cam[q];
      if (ci < 0) continue;
      double ys[6], W[18];
      if (first) {
        for (int a = 0; a < 6; ++a) ys[a] = ys0[a];
        for (int i = 0; i < 18; ++i) W[i] = W0[i];
      } else if (second) {
        for (int a = 0; a < 6; ++a) ys[a] = ys1[a];
        for (int i = 0; i < 18; ++i) W[i] = Wo[18 * (long)q + i];
      } else {
        for (int a = 0; a < 6; ++a) ys[a] = b.csc[6 * ci + a] * b.yc[6 * ci + a];
        for (int i = 0; i < 18; ++i) W[i] = Wo[18 * (long)q + i];
      }
      for (int c = 0; c < 3; ++c) {
        double s = 0;
        for (int a = 0; a < 6; ++a) s += W[a * 3 + c] * ys[a];
        t[c] += s;
      }
    }
    for (int c = 0; c < 3; ++c) t[c] = group_sum<kStepG>(t[c]);
    STEP_T(2);  // slot sums (loads of the first slot returned)
    // (2) point step y_p = -(V + D/r)^-1 (g_p + sum) in the scaled space, candidate point
    double rhs[3];
    for (int c = 0; c < 3; ++c) rhs[c] = -gpv[c] - t[c] * psv[c];
    double u[3], yp[3];
    fwd3(Lv, rhs, u);
    bwd3(Lv, u, yp);
    double d[3], xc[3];
    for (int a = 0; a < 3; ++a) {
      d[a] = yp[a] * psv[a];
      xc[a] = fmin(fmax(xv[a] + d[a], g.lo[a]), g.hi[a]);
    }
    if (gl == 0) {
      double gy = 0.0, yvy = 0.0, cross = 0.0;
      for (int a = 0; a < 3; ++a) {
        b.dp[3 * (long)j + a] = d[a];
        b.pts[1 - cur][3 * (long)j + a] = xc[a];
        const double dd = xc[a] - xv[a];
        s2 += dd * dd;
        xn2 += xv[a] * xv[a];
        gy += gpv[a] * yp[a];
        cross += d[a] * t[a];
        double vy = 0.0;
        for (int c = 0; c < 3; ++c) vy += Vv[3 * a + c] * yp[c];
        yvy += yp[a] * vy;
      }
      mc = -(gy + 0.5 * yvy + cross);
    }
    STEP_T(3);  // point solve, candidate point
    // (3) candidate cost of the point's observations
    for (int q = q0; q < end; q += kStepG) {
      const bool first = q == q0, second = q == q1;
      double cv[6], f[4];
      int right = 0;
      if (first) {
        for (int a = 0; a < 6; ++a) cv[a] = cv0[a];
        for (int k = 0; k < OD; ++k) f[k] = f0[k];
        right = right0;
      } else if (second) {
        for (int a = 0; a < 6; ++a) cv[a] = cv1[a];
        for (int k = 0; k < OD; ++k) f[k] = f1[k];
        right = right1;
      } else {
        const int o = b.p_obs[q];
        const int ci = b.p_cam[q], cam = ci + g.nf;
        for (int a = 0; a < 6; ++a) {
          const double xa = cams_x[6 * cam + a];
          cv[a] = ci >= 0 ? cam_cand(xa, b.csc[6 * ci + a] * b.yc[6 * ci + a]) : xa;
        }
        for (int k = 0; k < OD; ++k) f[k] = b.obs[(long)OD * o + k];
        if (OD == 2) right = b.cam_id[o] != 0;
      }
      double r[4];
      if (OD == 4)
        stereo_residual<false>(g, cv, nullptr, xc, f, r, nullptr, nullptr);
      else
        mono_residual<false>(g, cv, nullptr, xc, f, right, r, nullptr, nullptr);
      const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3];
      double rho0, sc;
      huber(s, &rho0, &sc);
      cc += 0.5 * rho0;
    }
  }
  STEP_T(4);  // candidate costs
  double v4[4] = {mc, cc, s2, xn2}, out[4];
  block_sum<4>(v4, out, lds);
  if (threadIdx.x == 0) {
    a_st<true>(&b.part[R_MODEL * g.pstride + blockIdx.x], out[0]);
    a_st<true>(&b.part[R_CAND * g.pstride + blockIdx.x], out[1]);
    a_st<true>(&b.part[R_STEP2 * g.pstride + blockIdx.x], out[2]);
    a_st<true>(&b.part[R_XN2 * g.pstride + blockIdx.x], out[3]);
  }
  STEP_T(5);  // block sum + partial stores
  }  // (point workgroups)
  // the last workgroup to finish (of either kind) reduces the partials
  // (step_finalize) and, single-GPU, runs the Ceres step handling
  if (!last_arrival_wt(b.cnt + g.m, gridDim.x)) {
    if (rot_wg) rot_step_body(g, b, cam_cur);
    return;
  }
#ifdef ME_STEP_TS
  if (threadIdx.x == 0) fin_prev_ = (long long)__builtin_amdgcn_s_memtime();
#endif
  step_finalize_body(g, b, o, do_decide);
  STEP_FIN_T(6);  // the finalizing workgroup: partial reduce + decide
#ifdef ME_STEP_TS
  if (threadIdx.x == 0) atomicAdd(&g_step_ts[7], 1ull);
#endif
  if (rot_wg) rot_step_body(g, b, cam_cur);  // (the camera workgroup arrived last: the table behind the step's decision)
}

__global__ void decide_kernel(Geo g, Bufs b, Opts o) {
  if (threadIdx.x != 0) return;
  if (b.st->done) return;
  decide(b, o);
}

}  // namespace
