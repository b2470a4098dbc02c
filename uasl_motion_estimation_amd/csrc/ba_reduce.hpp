// ba_reduce.hpp — part of ba.hip: the reductions and hand-off helpers shared
// by the BA kernels.  Defines no kernel: lane-group, wave and workgroup
// reductions (dpp_*, group_sum/min/max, wave_total, block_sum, block_max), the
// written-through hand-off (a_ld / a_st, drain_and_barrier, last_arrival_wt)
// and own_stores_visible.  Reads no other part.
#pragma once
#include "me_device.hpp"

namespace {

// Reductions over aligned groups of W lanes, every lane ending with the same
// bits: each level combines a lane's value with one from the sibling block
// (the blocks are uniform after the previous level, and a + b == b + a
// exactly).  Within a 16-lane row the partners come from DPP (quad permutes,
// row half-mirror, row mirror: a VALU move each); only the 16- and 32-lane
// levels go through the LDS crossbar (ds_bpermute).  (Round 3 used an xor
// butterfly of lane shuffles for every level.)
#ifndef ME_GROUP_DPP
#define ME_GROUP_DPP 1
#endif
template <int Ctrl>
__device__ __forceinline__ int dpp_i32(int x) {
  return __builtin_amdgcn_mov_dpp(x, Ctrl, 0xf, 0xf, false);
}
template <int Ctrl>
__device__ __forceinline__ double dpp_f64(double x) {
  return __hiloint2double(dpp_i32<Ctrl>(__double2hiint(x)), dpp_i32<Ctrl>(__double2loint(x)));
}
constexpr int kDppQuadSwap1 = 0xB1, kDppQuadSwap2 = 0x4E, kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;
template <int W>
__device__ __forceinline__ double group_sum(double x) {
  if (!ME_GROUP_DPP) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, W);
    return x;
  }
  if (W >= 2) x += dpp_f64<kDppQuadSwap1>(x);
  if (W >= 4) x += dpp_f64<kDppQuadSwap2>(x);
  if (W >= 8) x += dpp_f64<kDppRowHalfMirror>(x);
  if (W >= 16) x += dpp_f64<kDppRowMirror>(x);
  if (W >= 32) x += __shfl_xor(x, 16, W);
  if (W >= 64) x += __shfl_xor(x, 32, W);
  return x;
}

template <int W>
__device__ __forceinline__ int group_min(int x) {
  if (W >= 2) x = min(x, dpp_i32<kDppQuadSwap1>(x));
  if (W >= 4) x = min(x, dpp_i32<kDppQuadSwap2>(x));
  if (W >= 8) x = min(x, dpp_i32<kDppRowHalfMirror>(x));
  if (W >= 16) x = min(x, dpp_i32<kDppRowMirror>(x));
  if (W >= 32) x = min(x, __shfl_xor(x, 16, W));
  if (W >= 64) x = min(x, __shfl_xor(x, 32, W));
  return x;
}
template <int W>
__device__ __forceinline__ int group_max(int x) {
  if (W >= 2) x = max(x, dpp_i32<kDppQuadSwap1>(x));
  if (W >= 4) x = max(x, dpp_i32<kDppQuadSwap2>(x));
  if (W >= 8) x = max(x, dpp_i32<kDppRowHalfMirror>(x));
  if (W >= 16) x = max(x, dpp_i32<kDppRowMirror>(x));
  if (W >= 32) x = max(x, __shfl_xor(x, 16, W));
  if (W >= 64) x = max(x, __shfl_xor(x, 32, W));
  return x;
}

// The wave's sum in every lane, VALU only: the 16-lane row sums by DPP
// (quad swaps, half mirror, mirror), then the four row sums by readlane,
// added in row order (round 6: six dependent ds_bpermute rounds per value
// before -- 3.2k of the step finalize's 7.8k ticks, ME_STEP_TS).
__device__ __forceinline__ double wave_total(double x) {
  x += dpp_f64<kDppQuadSwap1>(x);
  x += dpp_f64<kDppQuadSwap2>(x);
  x += dpp_f64<kDppRowHalfMirror>(x);
  x += dpp_f64<kDppRowMirror>(x);
  auto row = [&](int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                            __builtin_amdgcn_readlane(__double2loint(x), l));
  };
  return ((row(0) + row(16)) + row(32)) + row(48);
}

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* out, double* lds /* nw*NV */, int nw_active = 0) {
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = wave_total(v[i]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) lds[wave * NV + i] = v[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = nw_active ? nw_active : (blockDim.x + 63) >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double s = 0;
      for (int w = 0; w < nw; ++w) s += lds[w * NV + i];
      out[i] = s;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ double block_max(double v, double* lds) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double r = 0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    r = lds[0];
    for (int w = 1; w < nw; ++w) r = fmax(r, lds[w]);
  }
  __syncthreads();
  return r;
}

// Written-through hand-off helpers (see "Hand-off form" at the camera solve).
template <bool SC1>
__device__ __forceinline__ double a_ld(const double* p) {
  if (!SC1) return *p;
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), ME_HO_LD,
                                                      __HIP_MEMORY_SCOPE_AGENT));
}
template <bool SC1>
__device__ __forceinline__ void a_st(double* p, double v) {
  if (!SC1) {
    *p = v;
    return;
  }
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v),
                     ME_HO_ST, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_and_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave, before the barrier
  __syncthreads();
}

// Before a lane reads back W_o words that lanes of its own wave stored earlier
// in program order (fused linearisation): the wave's stores have reached the
// memory its loads read (workgroup scope: one vector-memory wait, no cache
// maintenance), and the loads are not moved ahead of it.
__device__ __forceinline__ void own_stores_visible() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The last workgroup to arrive on a counter, with a written-through hand-off
// (the form of the camera solve's workers): thread 0 stored the workgroup's
// partials with sc1 stores, drains them before a relaxed arrival, and the last
// reads them with sc1 loads -- no L2 write-back (release) per arrival and no
// invalidate (acquire).  The last one re-arms the counter for the next launch.
__device__ __forceinline__ bool last_arrival_wt(unsigned* cnt, unsigned expected) {
  __shared__ int slast;
  __syncthreads();
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned k = __hip_atomic_fetch_add(cnt, 1u, ME_HO_RMW, __HIP_MEMORY_SCOPE_AGENT);
    slast = k == expected - 1;
    if (slast) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return slast != 0;
}

}  // namespace
