// ba_cam_solve.hpp — part of ba.hip: the camera solve, a dense blocked
// Cholesky of [S + D; -b^T] in its three forms (LDS, global memory, global
// memory with trailing-update workers) with the fused assemblers.  Kernel:
// cam_solve_kernel.  Reads the system assembled by ba_assemble.hpp (or
// assembles it in the same launch); leaves the camera step y_c for ba_step.hpp.
#pragma once
#include "me_internal.hpp"
#include "ba_types.hpp"
#include "me_device.hpp"
#include "roster.hpp"
#include "solve_diag.hpp"
#include "ba_reduce.hpp"
#include "ba_assemble.hpp"

using namespace ba;

namespace {

// One workgroup: S (assembled by s_assemble_kernel, all-reduced in sharded
// mode) + LM diagonal, blocked right-looking Cholesky with 16x16 blocks.
// The right-hand side rides along as an extra row [-b^T | 1] below S, so the
// factorisation also yields z = L^-1 (-b) (no separate forward solve).
// Per block column J:
//  * diagonal block (wave 0): L_JJ and X_J = L_JJ^-1 together, lane = (row,
//    4-column group), pivots by readlane, row broadcast by quad DPP;
//  * panel L_IJ = A_IJ X_J^T on v_mfma_f64_16x16x4f64, one wave per block row;
//  * trailing update A_IK -= L_IJ L_KJ^T on the matrix cores.
// Then the backward solve L^T y = z in wave 0 with the block inverses.
// The matrix is padded to N = 16 Ts >= n + 1 with an identity block.
#ifndef ME_SOLVE_BLOCK
#define ME_SOLVE_BLOCK 512
#endif
constexpr int kSolveBlock = ME_SOLVE_BLOCK;
constexpr int kLoadBatch = 32;

#ifdef ME_SOLVE_TS  // timing experiment only (tools/drivers.py solve_ts): wall-clock phases of cam_solve, 100 MHz ticks
// [1] lin_finalize, [2] assembly wait, [3] load, [4] factorisation, [5] backward
// solve, [6] candidate / cost tail, [8] last assembler exit - wg 0 entry,
// [9] first assembler entry - wg 0 entry, [10] s_memtime ticks of [1..6], [15] calls
// SOLVE_START / SOLVE_STAMP: s_memtime ticks of the phased loop's phases in
// State::stamps (me_debug_read): [0] the barrier behind the load, [1] diagonal,
// [2] panel, [3] trailing, [5] backward solve, [15] calls
#define SOLVE_STAMP(i)                                                               \
  do {                                                                               \
    if (tid == 0) st->stamps[(i)] += (long long)__builtin_amdgcn_s_memtime();        \
  } while (0)
#define SOLVE_START(i)                                                               \
  do {                                                                               \
    if (tid == 0) st->stamps[(i)] -= (long long)__builtin_amdgcn_s_memtime();        \
  } while (0)
__device__ long long g_solve_ts[24];
__device__ unsigned long long g_asm_first = ~0ull, g_asm_last = 0ull;
#define STS_DECL long long sts_prev_ = 0, sts_t0_ = 0, sts_c0_ = 0
#define STS_BEGIN()                                                        \
  do {                                                                     \
    if (threadIdx.x == 0) {                                                \
      sts_t0_ = sts_prev_ = (long long)__builtin_amdgcn_s_memrealtime();   \
      sts_c0_ = (long long)__builtin_amdgcn_s_memtime();                   \
    }                                                                      \
  } while (0)
#define STS(k)                                                             \
  do {                                                                     \
    if (threadIdx.x == 0) {                                                \
      const long long t_ = (long long)__builtin_amdgcn_s_memrealtime();    \
      atomicAdd((unsigned long long*)&g_solve_ts[(k)], (unsigned long long)(t_ - sts_prev_)); \
      sts_prev_ = t_;                                                      \
    }                                                                      \
  } while (0)
#define STS_END()                                                          \
  do {                                                                     \
    if (threadIdx.x == 0) {                                                \
      atomicAdd((unsigned long long*)&g_solve_ts[10],                      \
                (unsigned long long)((long long)__builtin_amdgcn_s_memtime() - sts_c0_)); \
      atomicAdd((unsigned long long*)&g_solve_ts[15], 1ull);               \
    }                                                                      \
  } while (0)
#define STS_ASM()                                                          \
  do {                                                                     \
    if (threadIdx.x == 0) {                                                \
      const unsigned long long a_ = atomicExch(&g_asm_last, 0ull);         \
      const unsigned long long f_ = atomicExch(&g_asm_first, ~0ull);       \
      if (a_) {                                                            \
        atomicAdd((unsigned long long*)&g_solve_ts[8], (unsigned long long)((long long)a_ - sts_t0_)); \
        atomicAdd((unsigned long long*)&g_solve_ts[9], (unsigned long long)((long long)f_ - sts_t0_)); \
      }                                                                    \
    }                                                                      \
  } while (0)
#else
#define SOLVE_STAMP(i) do {} while (0)
#define SOLVE_START(i) do {} while (0)
#define STS_DECL
#define STS_BEGIN() do {} while (0)
#define STS(k) do {} while (0)
#define STS_END() do {} while (0)
#define STS_ASM() do {} while (0)
#endif

// dynamic LDS: X (Ts x 256) | z/y (N) | row exchange (256) | A (N x ld, when it fits)
constexpr int kXchDoubles = 192;  // per buffer: the one-wave diagonal factor's LDS scratch (ME_DIAG_GATHER 0)
constexpr int kDiagLd = 17;  // staged diagonal block (global-memory form): 16 x 17 doubles
__host__ __device__ inline size_t solve_small_doubles(int Ts) {
  return 256 * (size_t)Ts + 16 * (size_t)Ts + 2 * (size_t)kXchDoubles + 16 * kDiagLd;
}
__host__ __device__ inline size_t solve_a_doubles(int Ts) { return (size_t)(16 * Ts) * solve_ld(Ts); }

// Global-memory form (windows whose [S; -b^T] does not fit the LDS, config 4
// and 5): block 0 factors the diagonal blocks and panels as below, and the
// trailing update of each block step is spread over the further workgroups
// of the same launch that joined its roster (roster.hpp: block 0 never waits
// for a workgroup that was not dispatched; with none, it updates the tiles
// itself).  Hand-offs through b.ssync (zeroed by
// s_assemble before every solve): block 0 publishes step J (epoch J + 1)
// once the panel of J is stored (every thread: agent-scope release fence,
// barrier, release store); a worker waits for the epoch (acquire, barrier),
// updates its tiles of step J and counts itself done (fence, barrier,
// release add); block 0 waits for all workers before the next diagonal
// block.  Every spin is also bounded (a safety net: every partner waited on
// is resident): a missing partner ends the solve as a failed step, never a
// hang.
constexpr unsigned kSolveTerm = 0x40000000u;  // epoch: stop (block 0 failed)
// Hand-off form (MI355X_MICROARCH.md, inter-workgroup visibility, Valid forms
// row 1): every store of A is write-through (sc1), every storing wave drains
// (vmcnt 0) before the workgroup barrier, ONE lane then stores the epoch / adds
// to the counter (agent-scope atomic), the consumer polls with an sc1 load and
// reads A only with sc1 loads after its barrier -- no release fence (an L2
// write-back) and no acquire (an L1 invalidate) per hand-off.
constexpr long kSolveSpin = 1L << 21;         // bounded waits (~0.5 s with s_sleep)
// (cam_solve_kernel's `flags` bits: kFlag*, me_internal.hpp -- scale.hip and mi.hip read the ctx's word too)
#ifndef ME_SOLVE_IMG
#define ME_SOLVE_IMG 1  // non-fused assembly writes the solver's image (0: S | b | diag U, loaded by the solve)
#endif
constexpr int kSolveMwMinTs = 16;             // block steps from which the trailing workers are used

template <bool SC1>
__device__ void trailing_tiles(double* A, int ld, int Ts, int J, int first, int stride, int lane) {
  const int j0 = 16 * J;
  const int rem = Ts - J - 1;
  const int npairs = rem * (rem + 1) / 2;
  for (int p = first; p < npairs; p += stride) {
    int I = 0, q = p;
    while (q > I) {
      q -= I + 1;
      ++I;
    }
    const int i0 = 16 * (J + 1 + I), k0 = 16 * (J + 1 + q);
    double av[4], bv[4];
    double4_t acc;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int cc = j0 + 4 * s + (lane >> 4);
      av[s] = -a_ld<SC1>(&A[(long)(i0 + (lane & 15)) * ld + cc]);
      bv[s] = a_ld<SC1>(&A[(long)(k0 + (lane & 15)) * ld + cc]);
      acc[s] = a_ld<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) a_st<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)], acc[s]);
  }
}

// Trailing tiles of block step J split for the lookahead of the one-workgroup
// solve: `col` = the tiles of column J + 1 only (they feed the next diagonal
// block), else every other tile (the deferred part, overlapped with the next
// diagonal block).  Tiles are dealt round-robin over (first, stride).
template <bool SC1>
__device__ void trailing_split(double* A, int ld, int Ts, int J, bool col, int first, int stride, int lane) {
  const int rem = Ts - J - 1;
  const int cnt = col ? rem : rem * (rem - 1) / 2;
  const int j0 = 16 * J;
  for (int p = first; p < cnt; p += stride) {
    int I, q;
    if (col) {
      I = p;
      q = 0;
    } else {  // p = I (I - 1) / 2 + q - 1, 1 <= q <= I
      I = 1;
      q = p;
      while (q >= I) {
        q -= I;
        ++I;
      }
      ++q;
    }
    const int i0 = 16 * (J + 1 + I), k0 = 16 * (J + 1 + q);
    double av[4], bv[4];
    double4_t acc;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int cc = j0 + 4 * s + (lane >> 4);
      av[s] = -a_ld<SC1>(&A[(long)(i0 + (lane & 15)) * ld + cc]);
      bv[s] = a_ld<SC1>(&A[(long)(k0 + (lane & 15)) * ld + cc]);
      acc[s] = a_ld<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) a_st<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)], acc[s]);
  }
}

// One trailing tile of block step J: A_IK -= L_IJ L_KJ^T (16 x 16, v_mfma_f64_16x16x4f64).
template <bool SC1>
__device__ __forceinline__ void trailing_tile(double* A, int ld, int J, int I, int K, int lane) {
  const int j0 = 16 * J, i0 = 16 * I, k0 = 16 * K;
  double av[4], bv[4];
  double4_t acc;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cc = j0 + 4 * s + (lane >> 4);
    av[s] = -a_ld<SC1>(&A[(long)(i0 + (lane & 15)) * ld + cc]);
    bv[s] = a_ld<SC1>(&A[(long)(k0 + (lane & 15)) * ld + cc]);
    acc[s] = a_ld<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
  for (int s = 0; s < 4; ++s) a_st<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + k0 + (lane & 15)], acc[s]);
}

// The same update of one tile, the result left in the MFMA accumulator (lane
// l holds A_IK[(l >> 4) + 4 s][l & 15] in element s: the layout the one-wave
// diagonal factorisation takes its block in) instead of stored.
// (Diagonal tile, K = I: both MFMA operands come from the same panel tile.)
template <bool SC1 = false>
__device__ __forceinline__ double4_t trailing_diag_acc(const double* A, int ld, int J, int I, int lane) {
  const int j0 = 16 * J, i0 = 16 * I;
  double av[4], bv[4];
  double4_t acc;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int cc = j0 + 4 * s + (lane >> 4);
    bv[s] = a_ld<SC1>(&A[(long)(i0 + (lane & 15)) * ld + cc]);
    av[s] = -bv[s];
    acc[s] = a_ld<SC1>(&A[(long)(i0 + (lane >> 4) + 4 * s) * ld + i0 + (lane & 15)]);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
  return acc;
}

// A bounded cross-workgroup wait of the camera solve timed out (a partner
// not co-resident): me_ba_* returns ME_ERR_STATE.  One GPU: the solve ends
// here.  Sharded: the rank must keep issuing the same collectives
// as its peers, so it only fails its steps -- st->fail reaches every rank
// through the step exchange (R_COUNT), the camera solve keeps failing while
// spin_err is set, and every rank ends alike after max_invalid rejected steps
// (decide, on exchanged values).
__device__ __forceinline__ void spin_timeout(const Bufs& b) {
  State* st = b.st;
  st->spin_err = 1;
  st->fail = 1;
  if (!b.xch) {
    st->done = 1;
    st->termination = 2;
  }
}

// Workers of the multi-workgroup solve.  Tile (I, K), 1 <= K <= I < Ts, is
// owned by one wave of one worker for the whole solve (linear index
// (I-1) I / 2 + K - 1, dealt round-robin over the workers' waves), so its
// successive updates are ordered by that wave's program order.  Per block step
// J (after block 0 publishes the panel of J): the tiles of column J + 1 below
// the diagonal and the diagonal tile (J + 2, J + 2) first -- block 0 needs
// them for the panel of J + 1 and the diagonal block J + 2 -- then the worker
// signals, then its other tiles.  The diagonal tile (J + 1, J + 1) is left to
// block 0, which applies step J to it in registers and factors it while the
// workers update column J + 1.
//
// The workers join the solve's roster (roster.hpp) first; block 0 closes it
// and the tiles are dealt over the P workers that joined (worker p, wave w:
// slot p nw + w), so block 0 never waits for a worker that was not
// dispatched.  Which wave updates a tile does not change its operations:
// the results are the same for any P.
__device__ void cam_solve_worker(const Geo& g, const Bufs& b, int nworkers) {
  __shared__ unsigned sep;
  __shared__ int s_pid, s_np;
  const State* st = b.st;
  if (st->done) return;  // block 0 returns for the same reason (before its close)
  if (threadIdx.x == 0) {
    // (no last-joiner close: the workers depend on block 0, which may not be
    // dispatched yet; without its count within kAbandonTicks they close the
    // roster empty and leave, and block 0 works alone)
    int pid = me_roster::join<me_roster_dev>(b.roster, 0u), np = 0;
    if (pid >= 0) {
      np = me_roster::count_or_abandon<me_roster_dev>(b.roster);
      if (np < 0) {  // a first closer that never published (not reachable: it is running)
        b.st->spin_err = 1;
        atomicOr(&b.st->pad[0], 1);  // spin site: worker roster count
        pid = -1;
      } else if (pid >= np) {
        pid = -1;  // the roster was abandoned (np = 0): block 0 updates every tile
      }
    }
    s_pid = pid;
    s_np = np;
  }
  __syncthreads();
  if (s_pid < 0) return;  // dispatched after the close: the joined workers own every tile
  if (st->fail || b.scal[R_COUNT] != 0.0) return;  // block 0 skips the factorisation for the same reasons
  const int Ts = g.Ts, ld = solve_ld(Ts);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int slot0 = s_pid * nw + wave, nslots = s_np * nw;
  const int ntiles = (Ts - 1) * Ts / 2;
  for (int J = 0; J + 1 < Ts; ++J) {
    if (tid == 0) {
      unsigned e = 0;
      long k = 0;
      for (; k < kSolveSpin; ++k) {
        e = __hip_atomic_load(b.ssync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (e >= (unsigned)(J + 1)) break;
        __builtin_amdgcn_s_sleep(2);
      }
      sep = k == kSolveSpin ? kSolveTerm : e;
      if (k == kSolveSpin) {  // block 0 never published the step: the solve ends in error
        b.st->spin_err = 1;
        atomicOr(&b.st->pad[0], 2);  // spin site: worker step poll
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads behind the poll
    __syncthreads();
    if (sep >= kSolveTerm) return;
    for (int pass = 0; pass < 2; ++pass) {
      for (int t = slot0; t < ntiles; t += nslots) {
        int I = 1, r = t;
        while (r >= I) {  // t = (I-1) I / 2 + (K-1)
          r -= I;
          ++I;
        }
        const int K = r + 1;
        // pass 0: column J + 1 below the diagonal tile, and the diagonal tile
        // (J + 2, J + 2); pass 1: the rest.  Tile (J + 1, J + 1) is block 0's
        // (it applies step J to it in registers before factoring it).
        const bool col = K == J + 1 && I > J + 1, nd = I == J + 2 && K == J + 2;
        if (pass == 0 ? (col || nd) : (K > J + 1 && !nd)) trailing_tile<true>(b.Abuf, ld, J, I, K, lane);
      }
      if (pass == 0) {
        drain_and_barrier();
        if (tid == 0) __hip_atomic_fetch_add(b.ssync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// Diagonal block Jd of the LDS-resident system on one wave, from its updated
// values in the accumulator layout (lane l, register r: row (l >> 4) + 4 r,
// column l & 15); false on a non-positive pivot.
__device__ __forceinline__ bool diag_factor_wave(double* A, int ld, double* X, double* xch, int n, int Jd,
                                                 double4_t A4, int lane) {
  const int jd0 = 16 * Jd;
  double* Ablk = A + (long)jd0 * ld + jd0;
  double* XJw = X + 256 * Jd;
  const int q = lane >> 4, c = lane & 15;
  bool ok = true;
  double4_t Y4;
#pragma unroll
  for (int r = 0; r < 4; ++r) Y4[r] = (q + 4 * r == c) ? 1.0 : 0.0;
  diag_round_mfma<0>(A4, Y4, q, c, n - jd0, ok, Ablk, ld, XJw, xch);
  diag_round_mfma<1>(A4, Y4, q, c, n - jd0, ok, Ablk, ld, XJw, xch);
  diag_round_mfma<2>(A4, Y4, q, c, n - jd0, ok, Ablk, ld, XJw, xch);
  diag_round_mfma<3>(A4, Y4, q, c, n - jd0, ok, Ablk, ld, XJw, xch);
  return ok;
}
__device__ __forceinline__ double4_t diag_load_wave(const double* A, int ld, int Jd, int lane) {
  const double* Ablk = A + (long)(16 * Jd) * ld + 16 * Jd;
  double4_t A4;
#pragma unroll
  for (int r = 0; r < 4; ++r) A4[r] = Ablk[((lane >> 4) + 4 * r) * ld + (lane & 15)];
  return A4;
}

// y = sum_m X[m][t] u_m over the 16 lanes of this lane's 16-lane row (lane m
// of the row holds u_m; lane t reads column t of X): DPP row broadcasts, in m
// order.
// (four partial sums over m mod 4, then (y0 + y1) + (y2 + y3): a 4-deep chain)
template <int M>
__device__ __forceinline__ void row_dot16_acc(double u, const double* X, int t, double (&y)[4]) {
  if constexpr (M < 16) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(u), 0x150 + M, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(u), 0x150 + M, 0xf, 0xf, false);
    y[M & 3] = fma(X[M * 16 + t], __hiloint2double(hi, lo), y[M & 3]);
    row_dot16_acc<M + 1>(u, X, t, y);
  }
}
__device__ __forceinline__ double row_dot16(double u, const double* X, int t) {
  double y[4] = {0.0, 0.0, 0.0, 0.0};
  row_dot16_acc<0>(u, X, t, y);
  return (y[0] + y[1]) + (y[2] + y[3]);
}

// kMode: 0 = [S; -b^T] in LDS, one workgroup; 1 = in global memory, one workgroup;
// 2 = in global memory, trailing updates on `nworkers` more workgroups (sc1 hand-offs)
template <int kMode>
// Fused assembly (nasm > 0; single GPU, modes 0 and 1): workgroups 1..nasm
// assemble S | b | diag(U) from the Schur partials (s_assemble_body, written
// through) and count themselves done on b.cnt[g.m + 3]; workgroup 0 runs the
// linearisation bookkeeping (lin_finalize) and, unless the solve has ended,
// waits for the count (bounded), re-arms it and reads S with sc1 loads.  One
// launch per LM iteration fewer than s_assemble_kernel + cam_solve_kernel.
__global__ __launch_bounds__(kSolveBlock) void cam_solve_kernel(Geo g, Bufs b, Opts o, int flags, int nworkers, int nasm,
                                                                const double* gc_raw, unsigned asm_gen) {
  extern __shared__ double smem[];
  __shared__ double red[64];
  __shared__ int sfail;
  constexpr bool kLds = kMode == 0, kSc1 = kMode == 2;
  // lookahead: the trailing update of step J outside column J + 1 overlaps the
  // next diagonal block (config 3: 44.2 -> 42.0 us).  Measured and dropped:
  // the panel fused with the column-(J+1) update in one phase (transposed
  // panel tiles as MFMA operands, no barrier between; 43.8 us) and a one-wave
  // backward solve without workgroup barriers (unchanged).
  // Also measured and dropped (git history keeps the code):
  // the panel tile kept in registers for the diagonal update, E = L^-T
  // accumulated by the workers, a one-wave backward solve, block 0 factored
  // beside the LDS copy, a four-wave diagonal factor.
  constexpr bool kLook = kMode != 2;
  // LDS-resident system: wave 0 alone on the critical path (see below)
  constexpr bool kPipe = kLds;
  __shared__ unsigned pflag, pdone;
  if (kMode == 2 && blockIdx.x > 0) {
    cam_solve_worker(g, b, nworkers);
    return;
  }
  unsigned* asm_cnt = b.cnt + g.m + 3;
  if (kMode != 2 && nasm > 0 && blockIdx.x > 0) {
#ifdef ME_SOLVE_TS
    if (threadIdx.x == 0) atomicMin(&g_asm_first, (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
    // Unit u = blockIdx.x - 1, claimed first (s_assemble_body `claim`): block
    // 0 takes the units nobody claimed once it has waited kCloseTicks for them
    // (an assembler held back behind other work, another process's kernels or
    // a CU mask), so it never waits for a workgroup that was not dispatched;
    // a late assembler finds its unit claimed and stores nothing.
    const int u = blockIdx.x - 1;
    // (sharded: the assemblers unpack the all-reduced exchange instead of summing partials)
    const bool mine = s_assemble_body<kSolveBlock, true>(g, b, u, 0, b.xch ? SA_UNPACK : SA_SUM,
                                                         kLds || ME_SOLVE_IMG ? b.Abuf : nullptr, &o,
                                                         b.asm_claim + u, asm_gen);
    drain_and_barrier();  // every wave's written-through stores have left
#ifdef ME_SOLVE_TS
    if (threadIdx.x == 0) atomicMax(&g_asm_last, (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
    if (mine && threadIdx.x == 0) __hip_atomic_fetch_add(asm_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  State* st = b.st;
  const bool fused = kMode != 2 && nasm > 0;
  STS_DECL;
  STS_BEGIN();
  __shared__ int s_steal;
  if (fused) {
    lin_finalize_body(g, b, o, gc_raw, red);
    STS(1);
    if (threadIdx.x == 0) {
      const int live = !st->done;
      // (what s_assemble's first block writes in the unfused form; read by decide)
      b.scal[R_COUNT] = (st->fail || (b.xch && b.xch[xo_fail(g)] != 0.0)) ? 1.0 : 0.0;
      // the assemblers' units: wait kCloseTicks for them, then claim and do
      // every unit still unclaimed here (normally none)
      s_steal = 0;
      if (live) {
        const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
        const long long lim = (flags & kFlagRosterNow) ? 0 : me_roster::kCloseTicks;
        while (__hip_atomic_load(asm_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)nasm) {
          if ((long long)__builtin_amdgcn_s_memrealtime() - t0 >= lim) {
            s_steal = 1;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
    }
    __syncthreads();
    if (s_steal) {
      __shared__ int s_taken;
      for (int u = 0; u < nasm; ++u) {
        // one decision for the whole workgroup (thread 0's load, through LDS):
        // per-wave loads could see an assembler's claim land between them, and
        // waves that skipped the unit would then meet the others' barriers
        // inside s_assemble_body at the wrong place (round 6: the count never
        // completed -- an intermittent hand-off timeout with another process on
        // the GPU)
        if (threadIdx.x == 0)
          s_taken = __hip_atomic_load(b.asm_claim + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= asm_gen;
        __syncthreads();
        const bool taken = s_taken != 0;
        __syncthreads();  // s_taken is rewritten for the next unit
        if (taken) continue;
        const bool mine = s_assemble_body<kSolveBlock, true>(g, b, u, 0, b.xch ? SA_UNPACK : SA_SUM,
                                                             kLds || ME_SOLVE_IMG ? b.Abuf : nullptr, &o,
                                                             b.asm_claim + u, asm_gen);
        drain_and_barrier();
        if (mine && threadIdx.x == 0) __hip_atomic_fetch_add(asm_cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (threadIdx.x == 0) {
      const int live = !st->done;
      long k = (flags & kFlagAsmTimeout) ? kSolveSpin : 0;  // (test hook: a forced timeout on this ctx)
      if (live && (s_steal || k)) {  // (all counted in the first wait: nothing left to wait for)
        for (; k < kSolveSpin; ++k) {
          if (__hip_atomic_load(asm_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)nasm) break;
          __builtin_amdgcn_s_sleep(1);
        }
      }
      if (live) {
        if (k == kSolveSpin) {
          // a unit never counted (not reachable: every claimed unit's owner is
          // running; kept as a safety net and for the test hook): the solve ends
          // in error (a late count may still come, so the counter is not
          // re-armed: the next plan clears it)
          spin_timeout(b);
          atomicOr(&b.st->pad[0], 4);  // spin site: fused assemblers' count
        } else {
          __hip_atomic_store(asm_cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next iteration
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads behind the poll
    __syncthreads();
    STS(2);
    STS_ASM();
    STS(11);
  }
  const int n = g.n6, Ts = g.Ts, N = 16 * Ts;
  const int ld = solve_ld(Ts);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  double* X = smem;
  double* u = X + 256 * (size_t)Ts;
  double* xch = u + N;  // diagonal-block exchange (2 x kXchDoubles)
  double* A = kLds ? xch + 2 * kXchDoubles : b.Abuf;
  // flags, radius and the whole lower block triangle of [S; -b^T] are
  // requested together: one round of global latency instead of a chain
  const int done = st->done;
  const int fail_in = st->fail || st->spin_err || (fused ? (b.xch && b.xch[xo_fail(g)] != 0.0) : b.scal[R_COUNT] != 0.0) ||
                      (flags & kFlagSolveFail);  // (test hook: a forced solve failure)
  const double radius = st->radius;
  // [S + D; -b^T]: every load of a batch is issued from a computed index
  // before the first use, so a batch costs one round of global latency.
  // (Per-element branches with the use inside them made the compiler wait on
  // every load: the load phase took 15.2 of the 45 us launch at config 3 and
  // 100 of 265 us at config 5, tools/drivers.py solve_ts.)  S | b | diag(U) are one
  // allocation (plan), so every element is an index off b.S.  The LM diagonal
  // (Ceres: clamp(diag(U)) / radius) goes through LDS (u, free until the
  // backward solve), loaded beside the first batch.  Loads are coherent (sc1):
  // the system is written through by this launch's assemblers, or by the
  // previous launch.
  const int CC = (N + 63) >> 6, RT = (N + nw - 1) / nw, NQ = RT * CC;
  const double* S0 = b.S;
  const int nn = n * n;
  // the image of [S + D; -b^T] in Abuf: written by s_assemble_kernel (non-fused), or by this launch's
  // assemblers (fused; written through)
  const bool img_ready = (flags & kFlagImg) != 0 || (fused && (kLds || ME_SOLVE_IMG));
  // LDS-DMA chunks of the image: all, or (pipelined form) the ones holding block row 0 first
  const int dma_bytes = N * ld * 8, dma_chunks = (dma_bytes + 1023) >> 10;
  const int dma_first = kPipe ? min(dma_chunks, (16 * ld * 8 + 1023) >> 10) : dma_chunks;
  auto dma_chunk = [&](int k) {
    const int off = (k << 10) + 16 * lane;
    if (off < dma_bytes)
      __builtin_amdgcn_global_load_lds((const void*)((const char*)b.Abuf + off),
                                       (__attribute__((address_space(3))) void*)((char*)A + (k << 10)), 16, 0,
                                       16 /* sc1 */);
  };
  if (!kLds && img_ready) {
    // the working matrix is Abuf itself: nothing to load.  (Fused: the
    // assemblers' written-through stores bypassed this XCD's L2, which may
    // still hold lines of Abuf from the previous launch's factorisation: an
    // agent-scope acquire invalidates them before the first plain load.)
    if (fused) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  } else if (kLds && img_ready) {
    // the assemblers wrote the solver's image (s_assemble_body img): N x ld
    // doubles, copied by LDS-DMA, 1 KiB per wave-instruction (lane-linear),
    // coherent reads (sc1); the barrier below retires them (vmcnt).  Only the
    // chunks of block row 0 here: the pipelined factorisation (kPipe) has
    // waves 1.. copy the rest while wave 0 factors diagonal block 0.
    if (!done)
      for (int k = wave; k < dma_first; k += nw) dma_chunk(k);
  } else
  for (int q0 = 0; q0 < NQ; q0 += kLoadBatch) {
    double xv[kLoadBatch];
    const int tb = q0 / CC, ub = q0 - tb * CC;  // (t, uu) of the batch's first element, stepped below
    int t = tb, uu = ub;
#pragma unroll
    for (int k = 0; k < kLoadBatch; ++k) {
      const int q = q0 + k;
      const int r = wave + nw * t, c = lane + 64 * uu;
      if (++uu == CC) {
        uu = 0;
        ++t;
      }
      // element class, branch-free: S (r, c < n), b as row n, b as column n
      // of the last diagonal block (it must stay symmetric); others load S[0]
      const bool in = q < NQ && r < N && c < n && (c >> 4) <= (r >> 4);
      const bool colb = q < NQ && c == n && r < n && (r >> 4) == (n >> 4);
      const int ix = in ? (r < n ? r * n + c : (r == n ? nn + c : 0)) : (colb ? nn + r : 0);
      xv[k] = a_ld<true>(S0 + ix);
    }
    if (q0 == 0) {
      STS(12);
      for (int r = tid; r < n; r += nt) u[r] = fmin(fmax(a_ld<true>(S0 + nn + n + r), o.min_diag), o.max_diag) / radius;
      __syncthreads();
      STS(13);
    }
    if (done) return;
    t = tb;
    uu = ub;
#pragma unroll
    for (int k = 0; k < kLoadBatch; ++k) {
      const int q = q0 + k;
      const int r = wave + nw * t, c = lane + 64 * uu;
      if (++uu == CC) {
        uu = 0;
        ++t;
      }
      const bool in = q < NQ && r < N && c < n && (c >> 4) <= (r >> 4);
      const bool colb = q < NQ && c == n && r < n && (r >> 4) == (n >> 4);
      double v = (in && r < n) ? xv[k] : ((in && r == n) || colb) ? -xv[k] : 0.0;
      if (in && r < n && r == c) v += u[r];
      if (q < NQ && r < N && c < N && (c >> 4) <= (r >> 4)) a_st<kSc1>(&A[r * ld + c], (r == c && r >= n) ? 1.0 : v);
    }
  }
  if (done) return;
  // trailing-update workers: close their roster (roster.hpp; at once when the
  // solve fails here anyway) -- the tiles are dealt over those that joined,
  // none of them: block 0 updates them itself (the phased loop)
  __shared__ int s_nwk;
  if (tid == 0) {
    sfail = fail_in;
    pflag = 0u;
    pdone = 0u;
    if (kMode == 2 && nworkers > 0)
      s_nwk = (int)me_roster::close<me_roster_dev>(b.roster, (unsigned)nworkers,
                                                   fail_in || (flags & kFlagRosterNow) ? 0 : me_roster::kCloseTicks);
  }
#ifdef ME_SOLVE_TS
  if (tid == 0) st->stamps[15] += 1;
#endif
  SOLVE_START(0);
  __syncthreads();
  STS(3);
  if (sfail) {
    if (tid == 0) st->fail = 1;
    return;
  }
  SOLVE_STAMP(0);
  if constexpr (kPipe) {
    // Wave 0 walks the critical path alone: per block step J it forms the
    // panel tile L_{J+1,J} = A_{J+1,J} X_J^T, publishes it (LDS flag), applies
    // step J to the diagonal tile (J+1, J+1) and factors diagonal block J+1 --
    // no workgroup barrier between.  Meanwhile the workers (waves other than
    // 0 and its SIMD sibling 4) form the other panel tiles of J, update
    // column J + 1 below the diagonal tile (after the flag), and, once every
    // worker's panel tiles are stored (LDS counter), the rest of step J's
    // trailing tiles.  One barrier per step joins both.  Same operations on
    // the same operands as the phased loop below: identical results.
    const bool worker = wave != 0 && !(nw > 4 && wave == 4);
    const int nwk = nw - 1 - (nw > 4 ? 1 : 0);
    const int widx = wave - 1 - (nw > 4 && wave > 4 ? 1 : 0);
    // diagonal block Jd from its (updated) values in the accumulator layout
    auto diag_factor = [&](int Jd, double4_t A4) {
      if (!diag_factor_wave(A, ld, X, xch, n, Jd, A4, lane)) sfail = 1;  // benign race: every writer stores 1
    };
    auto panel_tile = [&](int J, int I) {  // L_IJ = A_IJ X_J^T on the matrix cores
      const int j0 = 16 * J, i0 = 16 * I;
      const double* XJ = X + 256 * J;
      double av[4], bv[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        av[s4] = A[(long)(i0 + (lane & 15)) * ld + j0 + 4 * s4 + (lane >> 4)];
        bv[s4] = XJ[(lane & 15) * 16 + 4 * s4 + (lane >> 4)];
      }
      double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], bv[s4], acc, 0, 0, 0);
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) A[(long)(i0 + (lane >> 4) + 4 * q4) * ld + j0 + (lane & 15)] = acc[q4];
    };
    auto lds_wait = [&](volatile unsigned* f, unsigned want) {
      long k = 0;
      for (; k < kSolveSpin && *f < want; ++k) __builtin_amdgcn_s_sleep(1);
      if (k == kSolveSpin) {
        sfail = 1;
        st->spin_err = 1;
        atomicOr(&st->pad[0], 8);  // spin site: LDS-form step flags (pflag / pdone)
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    if (wave == 0) {
      diag_factor(0, diag_load_wave(A, ld, 0, lane));
    } else if (img_ready && nw > 1) {
      // the rest of the image, beside wave 0's block 0 (its rows are in LDS:
      // the barrier above retired their chunks); retired before the barrier
      for (int k = dma_first + wave - 1; k < dma_chunks; k += nw - 1) dma_chunk(k);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    STS(19);
    __syncthreads();
    for (int J = 0; J + 1 < Ts; ++J) {
      if (sfail) break;
      STS(18);
      if (wave == 0) {
        // step J on the diagonal tile, handed to the factorisation in registers
        // (its updated values are read by no one else: the factorisation
        // overwrites the lower triangle with L, the upper one is never read)
        panel_tile(J, J + 1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) pflag = (unsigned)(J + 1);
        solve_wave_sync();  // the panel tile just stored is an operand
        STS(16);
        diag_factor(J + 1, trailing_diag_acc(A, ld, J, J + 1, lane));
        STS(17);
      } else if (worker) {
        for (int I = J + 2 + widx; I < Ts; I += nwk) panel_tile(J, I);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) atomicAdd(&pdone, 1u);
        lds_wait(&pflag, (unsigned)(J + 1));
        for (int I = J + 2 + widx; I < Ts; I += nwk) trailing_tile<false>(A, ld, J, I, J + 1, lane);
        lds_wait(&pdone, (unsigned)(nwk * (J + 1)));
        trailing_split<false>(A, ld, Ts, J, false, widx, nwk, lane);  // tiles (I, K), J + 2 <= K <= I
      }
      __syncthreads();
    }
  } else if (kMode == 2 && nworkers > 0 && s_nwk > 0) {
    // Global-memory form with trailing workers (config 5), pipelined like the
    // LDS form: per block step J, wave 0 applies step J - 1 to the diagonal
    // tile (J, J) in registers (the workers left it out) and factors it, while
    // thread 64 waits for the workers' column-J count (their first pass of step
    // J - 1: column J below the diagonal and the diagonal tile (J + 1, J + 1)).
    // Then every wave forms the panel of J, and block 0 publishes step J and
    // goes on to the next diagonal tile without waiting for the workers: their
    // round trip overlaps the next diagonal block.  Same operations on the same
    // operands as the phased loop below: identical results.  (Measured and
    // dropped: wave 0 forming its panel tile transposed in registers and going
    // on without the panel barrier, the other waves publishing through an LDS
    // counter, and LDS-only barriers -- 144 vs 134 us per config-5 solve: the
    // workers' round trip, not wave 0, sets the step.)
    const int c = lane & 15, q = lane >> 4;
    double* Lblk = xch + 2 * kXchDoubles;
    for (int J = 0; J < Ts; ++J) {
      const int j0 = 16 * J;
      double* Ablk = A + (long)j0 * ld + j0;
      if (wave == 0) {
        double4_t A4, Y4;
        if (J > 0) {
          A4 = trailing_diag_acc<true>(A, ld, J - 1, J, lane);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) A4[r] = a_ld<true>(&Ablk[(q + 4 * r) * ld + c]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Y4[r] = (q + 4 * r == c) ? 1.0 : 0.0;
        bool ok = true;
        double* XJw = X + 256 * J;
        diag_round_mfma<0>(A4, Y4, q, c, n - j0, ok, Lblk, kDiagLd, XJw, xch);
        diag_round_mfma<1>(A4, Y4, q, c, n - j0, ok, Lblk, kDiagLd, XJw, xch);
        diag_round_mfma<2>(A4, Y4, q, c, n - j0, ok, Lblk, kDiagLd, XJw, xch);
        diag_round_mfma<3>(A4, Y4, q, c, n - j0, ok, Lblk, kDiagLd, XJw, xch);
        solve_wave_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (c <= q + 4 * r) a_st<true>(&Ablk[(q + 4 * r) * ld + c], Lblk[(q + 4 * r) * kDiagLd + c]);
        if (!ok) sfail = 1;  // benign race: every writer stores 1
        STS(16);
      } else if (tid == 64 && J > 0 && J + 1 < Ts) {
        const unsigned want = (unsigned)s_nwk * (unsigned)J;
        long k = 0;
        for (; k < kSolveSpin; ++k) {
          if (__hip_atomic_load(b.ssync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) break;
          __builtin_amdgcn_s_sleep(1);
        }
        if (k == kSolveSpin) {  // a worker not co-resident (narrow CU mask, busy CUs): the solve ends in error
          sfail = 1;
          st->spin_err = 1;
          atomicOr(&st->pad[0], 16);  // spin site: workers' step count
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads behind the poll
      __syncthreads();
      STS(17);
      if (sfail || J + 1 == Ts) break;
      // panel of J on the matrix cores: L_IJ = A_IJ X_J^T
      const double* XJ = X + 256 * J;
      for (int I = J + 1 + wave; I < Ts; I += nw) {
        const int i0 = 16 * I;
        double av[4], bv[4];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          av[s4] = a_ld<true>(&A[(long)(i0 + (lane & 15)) * ld + j0 + 4 * s4 + (lane >> 4)]);
          bv[s4] = XJ[(lane & 15) * 16 + 4 * s4 + (lane >> 4)];
        }
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4], bv[s4], acc, 0, 0, 0);
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) a_st<true>(&A[(long)(i0 + (lane >> 4) + 4 * q4) * ld + j0 + (lane & 15)], acc[q4]);
      }
      STS(18);
      drain_and_barrier();  // the panel's (and diagonal copy-back's) sc1 stores have left
      if (tid == 0) __hip_atomic_store(b.ssync, (unsigned)(J + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      STS(19);
    }
  } else
  for (int J = 0; J < Ts; ++J) {
    const int j0 = 16 * J;
    SOLVE_START(1);
    // (a) diagonal block + its inverse (wave 0; every wave joins the barrier)
    {
      const int c = lane & 15;
      double* Ablk = A + (long)j0 * ld + j0;
      // global-memory form: the rounds write the block's L into LDS (a round's
      // barrier would otherwise wait for its global stores), copied back after
      double* Lblk = kLds ? Ablk : xch + 2 * kXchDoubles;
      const int lld = kLds ? ld : kDiagLd;
      bool ok = true;
      double* XJw = X + 256 * J;
      {
        // lookahead: the trailing tiles of step J - 1 outside column J run on
        // waves 1-3 and 5-7 while wave 0 factors this block (wave 4 shares
        // wave 0's SIMD and stays out of its way)
        const bool sib = nw > 4 && wave == 4;  // wave 0's SIMD sibling
        if (kLook && J > 0 && wave != 0 && !sib)
          trailing_split<kSc1>(A, ld, Ts, J - 1, false, wave - 1 - (nw > 4 && wave > 4), nw - 1 - (nw > 4), lane);
        if (wave == 0) {
          const int q = lane >> 4;
          double4_t A4, Y4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            A4[r] = a_ld<kSc1>(&Ablk[(q + 4 * r) * ld + c]);
            Y4[r] = (q + 4 * r == c) ? 1.0 : 0.0;
          }
          diag_round_mfma<0>(A4, Y4, q, c, n - j0, ok, Lblk, lld, XJw, xch);
          diag_round_mfma<1>(A4, Y4, q, c, n - j0, ok, Lblk, lld, XJw, xch);
          diag_round_mfma<2>(A4, Y4, q, c, n - j0, ok, Lblk, lld, XJw, xch);
          diag_round_mfma<3>(A4, Y4, q, c, n - j0, ok, Lblk, lld, XJw, xch);
          if (!kLds) {
            solve_wave_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (c <= q + 4 * r) a_st<kSc1>(&Ablk[(q + 4 * r) * ld + c], Lblk[(q + 4 * r) * kDiagLd + c]);
          }
          if (!ok) sfail = 1;  // benign race: every writer stores 1
        }
      }
    }
    __syncthreads();
    SOLVE_STAMP(1);
    if (sfail) break;
    SOLVE_START(2);
    // (b) panel on the matrix cores: L_IJ = A_IJ X_J^T
    {
      const double* XJ = X + 256 * J;
      for (int I = J + 1 + wave; I < Ts; I += nw) {
        const int i0 = 16 * I;
        double av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          av[s] = a_ld<kSc1>(&A[(long)(i0 + (lane & 15)) * ld + j0 + 4 * s + (lane >> 4)]);
          bv[s] = XJ[(lane & 15) * 16 + 4 * s + (lane >> 4)];
        }
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) a_st<kSc1>(&A[(long)(i0 + (lane >> 4) + 4 * q) * ld + j0 + (lane & 15)], acc[q]);
      }
      __syncthreads();
    }
    SOLVE_STAMP(2);
    SOLVE_START(3);
    // (c) trailing update on the matrix cores: A_IK -= L_IJ L_KJ^T, J < K <= I
    {
      if (kLook)
        trailing_split<kSc1>(A, ld, Ts, J, true, wave, nw, lane);  // column J + 1 now, the rest with the next block
      else
        trailing_tiles<kSc1>(A, ld, Ts, J, wave, nw, lane);
      __syncthreads();
    }
    SOLVE_STAMP(3);
  }
  STS(4);
  if (sfail) {
    if (tid == 0) {
      st->fail = 1;
      if (st->spin_err) spin_timeout(b);  // not a numerical failure: me_ba_* returns an error
      if (kMode == 2 && nworkers > 0) __hip_atomic_store(b.ssync, kSolveTerm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  SOLVE_START(5);
  // backward solve L^T y = z (z = row n of L), block by block.
  // One column per thread (N <= 512): lane cc keeps u[cc] in a register and
  // walks the blocks K from the last down to its own; wave w owns blocks
  // 4w .. 4w + 3 (its 16-lane rows).  Per block K the owning row finalises
  // y_K = X_K^T u_K (its lanes' u by DPP row broadcasts), publishes y_K in
  // LDS and bumps an LDS flag; every lane of a lower block then subtracts
  // L_K^T y_K from its u (the previous form's sums in the same order).  No
  // workgroup barrier on the chain: a wave waits only for the blocks of other
  // waves, and the lanes' L entries of the next block are requested one block
  // ahead (global forms: a memory round trip per block otherwise).
  const int Jlast = (n - 1) >> 4;
  // Global forms only: in the LDS form the two-barrier loop below is faster
  // (config 3: 3.7 vs 5.3 us); at W = 50 this one is (17.4 vs 19.9 us).
  if (!kLds && N <= nt) {
    if (tid == 0) pflag = 0u;
    __syncthreads();
    const int cc = tid, myJ = cc >> 4, t = cc & 15;
    double acc = (cc < n && myJ <= Jlast) ? a_ld<kSc1>(&A[(long)n * ld + cc]) : 0.0;
    // the L entries of the next block in flight
    constexpr int kPf = 1;  // (3 blocks ahead measured slower: 20.3 vs 17.4 us at W = 50)
    double lpf[kPf][16];
    auto fetchL = [&](int K, double* dst) {
      if (K >= 0 && myJ < K) {
#pragma unroll
        for (int m = 0; m < 16; ++m) dst[m] = a_ld<kSc1>(&A[(long)(16 * K + m) * ld + cc]);
      }
    };
#pragma unroll
    for (int d = 0; d < kPf; ++d) fetchL(Jlast - d, lpf[d]);
    for (int K = Jlast; K >= 4 * wave; --K) {  // (wave-uniform)
      double lk[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) lk[m] = lpf[0][m];
#pragma unroll
      for (int d = 0; d + 1 < kPf; ++d)
#pragma unroll
        for (int m = 0; m < 16; ++m) lpf[d][m] = lpf[d + 1][m];
      fetchL(K - kPf, lpf[kPf - 1]);
      const unsigned want = (unsigned)(Jlast - K + 1);
      if ((K >> 2) == wave) {
        if (myJ == K) {
          double y = row_dot16(acc, X + 256 * K, t);
          y = 16 * K + t < n ? y : 0.0;
          u[16 * K + t] = y;
          acc = y;
        }
        solve_wave_sync();  // y_K in LDS for this wave's lanes
        if (lane == 0) *(volatile unsigned*)&pflag = want;
      } else {
        long k = 0;
        for (; k < kSolveSpin && *(volatile unsigned*)&pflag < want; ++k) __builtin_amdgcn_s_sleep(1);
        if (k == kSolveSpin) {
          sfail = 1;
          st->spin_err = 1;
          atomicOr(&st->pad[0], 32);  // spin site: backward-solve block flags
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
      if (myJ < K) {
        double yk[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) yk[m] = u[16 * K + m];
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int m = 0; m < 16; m += 2) {
          a0 = fma(lk[m], yk[m], a0);
          a1 = fma(lk[m + 1], yk[m + 1], a1);
        }
        acc -= a0 + a1;
      }
    }
    __syncthreads();
  } else {
  // (LDS form, and N > 512: wave 0 forms y_J = X_J^T z_J and every wave
  // updates the entries above the block, two barriers per block)
  for (int c = tid; c < N; c += nt) u[c] = c < n ? a_ld<kSc1>(&A[(long)n * ld + c]) : 0.0;
  __syncthreads();
  for (int J = Jlast; J >= 0; --J) {
    const int j0 = 16 * J;
    if (wave == 0) {
      const double* XJ = X + 256 * J;
      const int t = lane >> 2, gq = lane & 3;
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < 4; ++m) s += XJ[(4 * gq + m) * 16 + t] * u[j0 + 4 * gq + m];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      solve_wave_sync();
      if (gq == 0) u[j0 + t] = j0 + t < n ? s : 0.0;
    }
    __syncthreads();
    if (j0 > 0) {
      double yj[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) yj[m] = u[j0 + m];
      for (int cc = tid; cc < j0; cc += nt) {
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int m = 0; m < 16; m += 2) {
          a0 = fma(a_ld<kSc1>(&A[(long)(j0 + m) * ld + cc]), yj[m], a0);
          a1 = fma(a_ld<kSc1>(&A[(long)(j0 + m + 1) * ld + cc]), yj[m + 1], a1);
        }
        u[cc] -= a0 + a1;
      }
    }
    __syncthreads();
  }
  }
  SOLVE_STAMP(5);
  STS(5);
  // the scaled camera step; the candidate cameras and the camera part of the
  // model cost change are pt_step's camera workgroup (cam_step_body), beside
  // the points -- off this launch's serial tail
  for (int r = tid; r < n; r += nt) b.yc[r] = u[r];
  STS(6);
  STS_END();
}

}  // namespace
