// ba_assemble.hpp — part of ba.hip: the close of a linearisation and the
// assembly of the reduced camera system.  Kernels: lin_finalize_kernel,
// s_assemble_kernel; lin_finalize_body, xch_tail_body and s_assemble_body also
// run inside cam_solve_kernel (ba_cam_solve.hpp).  Reads pt_schur_kernel's
// partial tiles and the camera blocks of ba_linearize.hpp.
#pragma once
#include "ba_types.hpp"
#include "roster.hpp"
#include "ba_reduce.hpp"

using namespace ba;

namespace {

// Linearisation bookkeeping + iteration start: reduce the cost / gradient
// partials (fixed order), Ceres gradient-tolerance test (IterationZero /
// HandleSuccessfulStep), max-iteration and min-radius tests.
// The cost partials are summed by the first kFinBlock threads in the same
// order whatever the block size (256 in s_assemble_kernel, 512 inside the
// camera-solve launch): the same x_cost bits either way.  Sharded (b.xch):
// cost, camera gradient and the per-rank gradient max-norms come from the
// all-reduced exchange.
constexpr int kFinBlock = 256;
__device__ void lin_finalize_body(const Geo& g, const Bufs& b, const Opts& o, const double* gc_raw,
                                  double* lds /* 16 */) {
  State* st = b.st;
  if (st->done) return;
  if (st->need_lin) {
    const bool x = b.xch != nullptr;
    const int t = threadIdx.x;
    const bool in = t < kFinBlock;
    double c = 0, m = 0;
    if (!x && in) {
      for (int i = t; i < g.ncost; i += kFinBlock) c += b.part[R_COST * g.pstride + i];
      for (int i = t; i < g.ksplit; i += kFinBlock) m = fmax(m, b.part[R_GMAX_PT * g.pstride + i]);
    }
    const double* gcv = x ? b.xch + xo_gc(g) : gc_raw;
    if (in)
      for (int i = t; i < g.n6; i += kFinBlock) m = fmax(m, fabs(gcv[i]));
    if (x && in)
      for (int i = t; i < g.xslots; i += kFinBlock) m = fmax(m, b.xch[xo_gmax(g) + i]);
    double v[1] = {c}, out[1];
    block_sum<1>(v, out, lds, kFinBlock / 64);
    const double mm = block_max(m, lds + 8);
    if (threadIdx.x == 0) {
      st->x_cost = x ? b.xch[xo_cost(g)] : out[0];
      const double gm = mm;
      if (!st->scaled) {
        st->initial_cost = st->x_cost;
        st->scaled = 1;
      }
      st->need_lin = 0;
      if (gm <= o.gradient_tolerance) {
        st->done = 1;
        st->termination = 0;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0 || st->done) return;
  if (st->iterations >= o.max_num_iterations) {
    st->done = 1;
    st->termination = 1;
    return;
  }
  if (st->radius <= o.min_radius) {
    st->done = 1;
    st->termination = 0;
    return;
  }
  st->iterations += 1;
}

__global__ __launch_bounds__(kFinBlock) void lin_finalize_kernel(Geo g, Bufs b, Opts o, const double* gc_raw) {
  __shared__ double lds[16];
  lin_finalize_body(g, b, o, gc_raw, lds);
}

// Sharded mode: this rank's linearisation scalars into the exchange tail --
// cost (fixed-order sum of the linearize partials), failure flag, gradient
// max-norm in this rank's slot (0 in the others), raw camera gradient.
__device__ void xch_tail_body(const Geo& g, const Bufs& b, const double* gc_raw, double* lds /* 16 */) {
  const State* st = b.st;
  double c = 0, m = 0;
  if (st->need_lin) {
    for (int i = threadIdx.x; i < g.ncost; i += kFinBlock) c += b.part[R_COST * g.pstride + i];
    for (int i = threadIdx.x; i < g.ksplit; i += kFinBlock) m = fmax(m, b.part[R_GMAX_PT * g.pstride + i]);
  }
  double* x = b.xch;
  for (int i = threadIdx.x; i < g.n6; i += kFinBlock) x[xo_gc(g) + i] = gc_raw[i];
  for (int i = threadIdx.x; i < g.xslots; i += kFinBlock)
    if (i != g.xrank) x[xo_gmax(g) + i] = 0.0;
  double v[1] = {c}, out[1];
  block_sum<1>(v, out, lds);
  const double mm = block_max(m, lds + 8);
  if (threadIdx.x == 0) {
    x[xo_cost(g)] = out[0];
    x[xo_fail(g)] = st->fail ? 1.0 : 0.0;
    x[xo_gmax(g) + g.xrank] = mm;
  }
}

// S = U - sum over the Schur runs' partial tiles, b = g - Y^T z, diag(U)
// (sharded mode: the local pieces, no LM diagonal).  256 threads = 32
// elements x 8 partial groups: group k sums entries k, k + 8, ... of the
// tile's slot list (the runs covering the tile, in run order), then the 8
// group sums are added in order (deterministic).  The threads walk
// the partial tiles in their own layout (the upper block triangle, tile pair
// p = (I <= J), row-major 16 x 16), so consecutive threads read consecutive
// doubles of every partial; the sums land in the lower block triangle of S
// (transposed for I < J; the diagonal tiles as they are), the column n6 of
// the tiles in b.  `full` also writes the upper block triangle (reduced-system
// / covariance read-back); the camera solve reads only the lower one.
constexpr int kSaElems = 32, kSaGroups = kBlock / kSaElems;
// The grid's last workgroup runs the linearisation bookkeeping of
// lin_finalize_kernel instead (one launch less per iteration): the assembly
// blocks do not read what it writes, and the camera solve that follows
// reads both.
// Assembly of elements blk * EL .. blk * EL + EL - 1 by NTH = 8 EL threads
// (8 partial groups of EL elements).  No early return: the fused form's
// workgroup signals after every thread's stores have drained.  SC1: stores
// written through for a consumer workgroup of the same launch.
// mode (sharded runs): SA_PACK sums this rank's partials and U
// into the exchange buffer in the tile layout (element idx of [S | b] at
// xch[idx], diag(U) in the tail) instead of S; SA_UNPACK reads the all-reduced
// exchange (no partials, no U) and stores S / b / diag(U) exactly as SA_SUM.
__host__ __device__ inline int solve_ld(int Ts) { return ((16 * Ts + 31) / 32) * 32 + 2; }  // == 2 mod 32
enum { SA_SUM = 0, SA_PACK = 1, SA_UNPACK = 2 };
// img (fused camera solve, LDS form): instead of S | b | diag(U), the
// assembly writes the solver's image of [S + D; -b^T] itself -- the lower
// block triangle of the N x ld padded matrix the factorisation runs on (the
// LM diagonal clamp(diag U) / radius added, row n = -b^T, the last diagonal
// block symmetric, identity padding), written through -- so the solve copies
// it into LDS with a few LDS-DMA instructions instead of an element-wise load
// (whose one-time code dominated the launch, tools/drivers.py solve_ts).
//
// claim (fused assembly): the unit is first claimed for launch generation
// `gen` (atomic max on its claim word, issued before the loads, its result
// read only before the stores); a unit another workgroup claimed first is
// left to it -- no stores, and the function returns false.
template <int NTH, bool SC1>
__device__ bool s_assemble_body(const Geo& g, const Bufs& b, int blk, int full, int mode = SA_SUM,
                                double* img = nullptr, const Opts* o = nullptr, unsigned* claim = nullptr,
                                unsigned gen = 0) {
  constexpr int EL = NTH / kSaGroups;
  __shared__ double part[kSaGroups][EL];
  __shared__ int s_claimed;
  unsigned claim_old = 0;
  if (claim && threadIdx.x == 0) claim_old = me_roster_dev::fetch_max(claim, gen);  // (roster.hpp CLAIM, split)
  const State* st = b.st;
  const bool live = !(st->done || st->final_pass);  // final pass: no step follows, S is not needed
  const int n = g.n6;
  const int e = threadIdx.x % EL, grp = threadIdx.x / EL;
  const int idx = blk * EL + e;
  int gr = -1, gc = -1;  // position in the (padded) system [S | b]
  bool diag = false;
  if (idx < g.npairs * 256) {
    int p = idx >> 8, I = 0;
    while (p >= g.T - I) {  // tile pair p -> (I, J): row I holds T - I pairs
      p -= g.T - I;
      ++I;
    }
    const int J = I + p;
    diag = I == J;
    gr = 16 * I + ((idx >> 4) & 15);
    gc = 16 * J + (idx & 15);
  }
  // S entries (gr, gc < n) and the right-hand side (gc == n); the padding is skipped
  const bool use = live && gr >= 0 && gr < n && gc <= n;
  const bool fail = st->fail || (mode == SA_UNPACK && b.xch[xo_fail(g)] != 0.0);  // (unpack: any rank's failure)
  double acc = 0.0;
  if (use && !fail && mode != SA_UNPACK) {
    // the partials of the runs covering this tile (run order): entries grp,
    // grp + 8, ... added in order; their loads issued 8 at a time
    // (independent addresses: one memory latency per batch, not per add)
#ifndef ME_SA_BATCH
#define ME_SA_BATCH 16
#endif
    if (g.sorted) {
      // whole lists (padded with -1 at plan time): no wait for the tile's count
      // before the list loads -- two rounds of latency (list, partials) per batch
      const int cnt = g.nruns;
      const int* tl = b.tl + (long)(idx >> 8) * g.nruns;
      const double* src = b.Spart + (idx & 255);
      for (int q0 = grp; q0 < cnt; q0 += ME_SA_BATCH * kSaGroups) {
        int sl[ME_SA_BATCH];
#pragma unroll
        for (int k = 0; k < ME_SA_BATCH; ++k) {
          const int q = q0 + k * kSaGroups;
          sl[k] = q < cnt ? tl[q] : -1;
        }
        double v[ME_SA_BATCH];
#pragma unroll
        for (int k = 0; k < ME_SA_BATCH; ++k) v[k] = sl[k] >= 0 ? src[(long)sl[k] * 256] : 0.0;
#pragma unroll
        for (int k = 0; k < ME_SA_BATCH; ++k)
          if (sl[k] >= 0) acc += v[k];
      }
    } else {  // every run holds every tile, at slot run * npairs + tile
      const double* src = b.Spart + idx;
      const long stride = (long)g.npairs * 256;
      for (int q0 = grp; q0 < g.nruns; q0 += ME_SA_BATCH * kSaGroups) {
        double v[ME_SA_BATCH];
#pragma unroll
        for (int k = 0; k < ME_SA_BATCH; ++k) {
          const int q = q0 + k * kSaGroups;
          v[k] = q < g.nruns ? src[q * stride] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < ME_SA_BATCH; ++k)
          if (q0 + k * kSaGroups < g.nruns) acc += v[k];
      }
    }
  }
  part[grp][e] = acc;
  if (claim && threadIdx.x == 0) s_claimed = claim_old < gen;
  __syncthreads();
  if (claim && !s_claimed) return false;
  if (img != nullptr) {
    // every element of the tile pair when live (padding included): the image
    // is complete without any other writer
    if (grp == 0 && live && gr >= 0) {
      const int ld = solve_ld(g.Ts);
      double sum = 0.0;
      if (mode == SA_UNPACK) {
        sum = b.xch[idx];
      } else {
#pragma unroll
        for (int k = 0; k < kSaGroups; ++k) sum += part[k][e];
      }
      double v;
      if (gr < n && gc < n) {
        if (mode == SA_UNPACK) {
          v = fail ? 0.0 : sum;
        } else {
          v = 0;
          if (gr / 6 == gc / 6) v = b.U[36 * (gr / 6) + (gr % 6) * 6 + (gc % 6)];
          v = fail ? 0.0 : v - sum;
        }
        if (gr == gc) {
          const double du = mode == SA_UNPACK ? b.xch[xo_diag(g) + gr] : b.U[36 * (gr / 6) + (gr % 6) * 7];
          v += fmin(fmax(du, o->min_diag), o->max_diag) / b.st->radius;
        }
      } else if ((gr < n && gc == n) || (gr == n && gc < n)) {
        const int r = gr < n ? gr : gc;  // (the (n, c) partial equals the (c, n) one bit for bit: Y^T Y)
        v = -(fail ? 0.0 : mode == SA_UNPACK ? sum : b.gcs[r] - sum);
      } else {
        v = gr == gc ? 1.0 : 0.0;  // (n, n) and the padding: identity
      }
      a_st<SC1>(&img[diag ? (long)gr * ld + gc : (long)gc * ld + gr], v);
    }
    return true;
  }
  if (grp == 0 && use) {
    double sum = 0.0;
    if (mode == SA_UNPACK) {
      sum = b.xch[idx];
    } else {
#pragma unroll
      for (int k = 0; k < kSaGroups; ++k) sum += part[k][e];
    }
    if (gc < n) {
      double v = 0;
      if (mode == SA_UNPACK) {
        v = fail ? 0.0 : sum;
      } else {
        if (gr / 6 == gc / 6) v = b.U[36 * (gr / 6) + (gr % 6) * 6 + (gc % 6)];  // U blocks are symmetric
        v = fail ? 0.0 : v - sum;
      }
      if (mode == SA_PACK) {
        b.xch[idx] = v;
      } else if (diag) {
        a_st<SC1>(&b.S[(long)gr * n + gc], v);
      } else {
        a_st<SC1>(&b.S[(long)gc * n + gr], v);
        if (full) b.S[(long)gr * n + gc] = v;
      }
    } else {
      const double bv = fail ? 0.0 : mode == SA_UNPACK ? sum : b.gcs[gr] - sum;
      const double du = mode == SA_UNPACK ? b.xch[xo_diag(g) + gr] : b.U[36 * (gr / 6) + (gr % 6) * 7];
      if (mode == SA_PACK) {
        b.xch[idx] = bv;
        b.xch[xo_diag(g) + gr] = du;
      } else {
        a_st<SC1>(&b.bvec[gr], bv);
        a_st<SC1>(&b.diagU[gr], du);
      }
    }
  } else if (mode == SA_PACK && grp == 0 && idx < g.npairs * 256) {
    b.xch[idx] = 0.0;  // padding (and a finished solve): defined values in the exchange
  }
  return true;
}

// mode SA_PACK (sharded, before the exchange): the last workgroup writes the
// exchange tail instead of finalizing; SA_UNPACK (sharded, after it, when
// the camera solve does not unpack itself): as SA_SUM from the exchange.
__global__ __launch_bounds__(kBlock) void s_assemble_kernel(Geo g, Bufs b, Opts o, const double* gc_raw, int full,
                                                            int mode, double* img = nullptr) {
  static_assert(kBlock == kFinBlock, "the finalize block runs with the assembly block size");
  if (blockIdx.x == gridDim.x - 1) {
    __shared__ double lds[16];
    if (mode == SA_PACK) {
      xch_tail_body(g, b, gc_raw, lds);
      return;
    }
    if (threadIdx.x < 2) b.ssync[threadIdx.x] = 0u;  // the camera solve that follows starts its steps at 0
    lin_finalize_body(g, b, o, gc_raw, lds);
    return;
  }
  if (mode != SA_PACK && blockIdx.x == 0 && threadIdx.x == 0 && !(b.st->done || b.st->final_pass))
    b.scal[R_COUNT] = (b.st->fail || (mode == SA_UNPACK && b.xch[xo_fail(g)] != 0.0)) ? 1.0 : 0.0;
  s_assemble_body<kBlock, false>(g, b, blockIdx.x, full, mode, img, &o);
}

}  // namespace
