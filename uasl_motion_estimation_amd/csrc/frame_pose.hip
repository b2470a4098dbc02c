// frame_pose.hip — pose-only refinement of a pushed frame against the last
// keyframe (include/me_hip.h, section A12j; the numpy restatement is
// frame_pose.frame_pose_ref).
//
// iters launches of fpose_iter_kernel and one of fpose_final_kernel on the ctx
// stream, each a grid of ceil(n / 256) workgroups, one wave per chunk of 64
// features, a lane per feature.  The lanes' 27 terms are staged in LDS, a lane
// per sum walks the chunk's 64 staged terms in index order, and the wave
// writes its partial to scratch.  The workgroup that takes the last ticket of
// an integer counter adds the partials in chunk order, solves and writes the
// pose for the next launch.  The final pass counts with integer atomics, and
// its last workgroup writes info and zeroes the tickets and counters for the
// next call.  Nobody waits for anybody: no launch needs its grid co-resident.
// (Everything in one launch of one workgroup, gate_finish_kernel's shape, was
// measured slower: 122.4 us against 69.9 us per call at 2000 features,
// DESIGN.md 5.15.)
// FP64 throughout, + - * / sqrt only, every sum in the header's order; the
// library is built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include "gate_math.hpp"
#include "me_internal.hpp"

namespace {

using namespace me_gate;  // cross3, project, gn_update

constexpr int kBlock = 256;  // threads of every kernel here
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 64;   // feature indices per partial of the ordered sums
constexpr int kSums = 27;    // 21 (upper triangle of H) + 6 (b)
constexpr int kMaxIters = 16;

// The call's block in ctx-owned memory: all zero between calls but for pose
struct FpWork {
  uint32_t ticket;
  int nu0;             // usable features, counted by the first iteration's launch
  int nu, nact, ninl;  // the final pass's counts
  int steps, stop, pad;
  double pose[12];     // R row-major, t: written by each iteration's last workgroup
};
static_assert(sizeof(FpWork) == 128, "FpWork layout");

struct FpArgs {
  const float* ref_uv;
  const float* ref_xr;
  const float* cur_uv;
  const uint8_t* alive;
  int n;
  double f, cx, cy, fb;  // fb = f * baseline
  double min_disp, huber, g2;  // g2 = gate_max * gate_max
  int iters, min_inliers;
  const unsigned char* start;  // an info block, or NULL
  double* part;                // kSums per chunk
  FpWork* work;
  float* err_out;
  unsigned char* info;
};

template <class T>
__device__ __forceinline__ T ld_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entry i of the start pose (step 3)
__device__ __forceinline__ double start_pose(const FpArgs& g, int i) {
  if (g.start && ((const int32_t*)g.start)[4] == 1) return ((const double*)(g.start + 32))[i];
  return (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
}

// Steps 1 and 2: usable, and then P and the current position as doubles
__device__ __forceinline__ bool load_feature(const FpArgs& g, int k, double* P, double& u1, double& v1) {
  const float fu0 = g.ref_uv[2 * (size_t)k], fv0 = g.ref_uv[2 * (size_t)k + 1], fx0 = g.ref_xr[k];
  const float fu1 = g.cur_uv[2 * (size_t)k], fv1 = g.cur_uv[2 * (size_t)k + 1];
  const double d0 = (double)fu0 - (double)fx0;
  if (!(g.alive[k] != 0 && isfinite(fu1) && isfinite(fv1) && d0 >= g.min_disp)) return false;
  const double Z = g.fb / d0;
  P[0] = ((double)fu0 - g.cx) * Z / g.f;
  P[1] = ((double)fv0 - g.cy) * Z / g.f;
  P[2] = Z;
  u1 = (double)fu1;
  v1 = (double)fv1;
  return true;
}

// Y, the two residuals and e2 of a usable feature under (R, t); returns act
__device__ __forceinline__ bool residual(const FpArgs& g, const double* R, const double* t, const double* P, double u1,
                                         double v1, double* Y, double* r, double& e2) {
  double uh, vh;
  project(R, t, P, g, Y, uh, vh);
  r[0] = uh - u1;
  r[1] = vh - v1;
  e2 = r[0] * r[0] + r[1] * r[1];
  return Y[2] > 0.0;
}

// Feature k's 27 terms of step 4 under (R, t): +0.0 each where k is out of range or not act
__device__ __forceinline__ void feature_terms(const FpArgs& g, int k, const double* R, const double* t, double* term) {
  for (int s = 0; s < kSums; ++s) term[s] = 0.0;
  if (k >= g.n) return;
  double P[3], u1, v1, Y[3], r[2], e2;
  if (!load_feature(g, k, P, u1, v1)) return;
  if (!residual(g, R, t, P, u1, v1, Y, r, e2)) return;
  const double e = sqrt(e2);
  const double w = e <= g.huber ? 1.0 : g.huber / e;
  const double a = g.f / Y[2], q = Y[2] * Y[2];
  const double gr[2][3] = {{a, 0.0, -(g.f * Y[0]) / q}, {0.0, a, -(g.f * Y[1]) / q}};
  double J[2][6];
  for (int m = 0; m < 2; ++m) {
    cross3(Y, gr[m], J[m]);
    for (int i = 0; i < 3; ++i) J[m][3 + i] = gr[m][i];
  }
  int s = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) term[s++] = w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]);
  for (int i = 0; i < 6; ++i) term[s++] = w * (J[0][i] * r[0] + J[1][i] * r[1]);
}

// The final pass of feature k < n: bit 0 usable, bit 1 act, bit 2 inlier; err_out written
__device__ __forceinline__ int final_feature(const FpArgs& g, int k, const double* R, const double* t) {
  double P[3], u1, v1, Y[3], r[2], e2;
  float err = INFINITY;
  int bits = 0;
  if (load_feature(g, k, P, u1, v1)) {
    bits = 1;
    if (residual(g, R, t, P, u1, v1, Y, r, e2)) {
      bits |= 2;
      err = (float)sqrt(e2);
      if (e2 <= g.g2) bits |= 4;
    }
  }
  if (g.err_out) g.err_out[k] = err;
  return bits;
}

__device__ __forceinline__ void write_info(const FpArgs& g, int nu, int nact, int ninl, int steps, const double* pose) {
  int32_t* iw = (int32_t*)g.info;
  iw[0] = nu;
  iw[1] = nact;
  iw[2] = ninl;
  iw[3] = steps;
  iw[4] = (steps == g.iters && ninl >= g.min_inliers) ? 1 : 0;
  iw[5] = iw[6] = iw[7] = 0;
  double* dw = (double*)(g.info + 32);
  for (int i = 0; i < 12; ++i) dw[i] = pose[i];
}

// A wave's chunk: the lanes' terms staged in LDS, then lane s < kSums adds row s in index order from +0.0
__device__ __forceinline__ double chunk_sum(double (*stage)[kChunk + 1], const double* term, int lane) {
  for (int s = 0; s < kSums; ++s) stage[s][lane] = term[s];
  __syncthreads();
  double acc = 0.0;
  if (lane < kSums) {
    for (int j0 = 0; j0 < kChunk; j0 += 16) {  // (16 reads in flight, then their adds in index order)
      double v[16];
      for (int j = 0; j < 16; ++j) v[j] = stage[lane][j0 + j];
      for (int j = 0; j < 16; ++j) acc = acc + v[j];
    }
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void fpose_iter_kernel(FpArgs g, int it) {
  __shared__ double s_stage[kWaves][kSums][kChunk + 1];  // (+1: a lane per sum reads its row without bank conflicts)
  __shared__ double s_tot[kSums];
  __shared__ double s_pose[12];
  __shared__ int s_last;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  FpWork* w = g.work;
  if (it > 0 && w->stop) return;  // (uniform: written by an earlier launch)
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = it == 0 ? start_pose(g, i) : w->pose[i];
  for (int i = 0; i < 3; ++i) t[i] = it == 0 ? start_pose(g, 9 + i) : w->pose[9 + i];
  const int nchunks = (g.n + kChunk - 1) / kChunk;
  const int chunk = blockIdx.x * kWaves + wv;
  const int k = chunk * kChunk + lane;
  double term[kSums];
  feature_terms(g, k, R, t, term);
  const double acc = chunk_sum(s_stage[wv], term, lane);
  if (chunk < nchunks && lane < kSums) g.part[(size_t)chunk * kSums + lane] = acc;
  if (it == 0) {  // the usable features, once per call
    double P[3], u1, v1;
    const bool usable = k < g.n && load_feature(g, k, P, u1, v1);
    const int c = __popcll(__ballot(usable));
    if (lane == 0 && c) __hip_atomic_fetch_add(&w->nu0, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the ticket: every wave's partial and count are out before its workgroup arrives
  __threadfence();
  __syncthreads();
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(&w->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;  // (uniform)
  __threadfence();
  if (tid < kSums) {
    double tot = 0.0;
    int c = 0;
    for (; c + 8 <= nchunks; c += 8) {  // (8 loads in flight, then their adds in chunk order)
      double v[8];
      for (int j = 0; j < 8; ++j) v[j] = ld_agent(&g.part[(size_t)(c + j) * kSums + tid]);
      for (int j = 0; j < 8; ++j) tot = tot + v[j];
    }
    for (; c < nchunks; ++c) tot = tot + ld_agent(&g.part[(size_t)c * kSums + tid]);
    s_tot[tid] = tot;
  }
  if (tid == 0) {
    for (int i = 0; i < 9; ++i) s_pose[i] = R[i];
    for (int i = 0; i < 3; ++i) s_pose[9 + i] = t[i];
  }
  __syncthreads();
  if (tid == 0) {
    if (it == 0 && ld_agent(&w->nu0) < 3) {
      w->stop = 1;  // fewer than 3 usable features: no step at all
    } else if (gn_update(s_tot, s_pose)) {
      w->steps = it + 1;
    } else {
      w->stop = 1;
    }
    for (int i = 0; i < 12; ++i) w->pose[i] = s_pose[i];
    w->ticket = 0;
  }
}

__global__ __launch_bounds__(kBlock) void fpose_final_kernel(FpArgs g) {
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  FpWork* w = g.work;
  double pose[12];
  for (int i = 0; i < 12; ++i) pose[i] = g.iters == 0 ? start_pose(g, i) : w->pose[i];
  const int k = blockIdx.x * kBlock + tid;
  const int bits = k < g.n ? final_feature(g, k, pose, pose + 9) : 0;
  const int cu = __popcll(__ballot((bits & 1) != 0)), ca = __popcll(__ballot((bits & 2) != 0)),
            ci = __popcll(__ballot((bits & 4) != 0));
  if (lane == 0) {
    if (cu) __hip_atomic_fetch_add(&w->nu, cu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ca) __hip_atomic_fetch_add(&w->nact, ca, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ci) __hip_atomic_fetch_add(&w->ninl, ci, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence();
  __syncthreads();  // (every thread has read the start pose by now: info may be that block)
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(&w->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!s_last || tid != 0) return;
  __threadfence();
  write_info(g, ld_agent(&w->nu), ld_agent(&w->nact), ld_agent(&w->ninl), w->steps, pose);
  w->ticket = 0;  // the block is zero again for the next call
  w->nu0 = 0;
  w->nu = 0;
  w->nact = 0;
  w->ninl = 0;
  w->steps = 0;
  w->stop = 0;
}

}  // namespace

extern "C" void me_frame_pose_default_params(me_frame_pose_params* p) {
  if (!p) return;
  p->huber = 1.0;
  p->gate_max = 2.0;
  p->min_disp = 0.5;
  p->iters = 6;
  p->min_inliers = 6;
}

// The parameter checks the entry point and me_vo_loop_set_frame_pose share: NULL on success, else the
// message, which names the argument.
const char* me_frame_pose_check(const me_frame_pose_params* p) {
  if (!p) return "null params";
  if (!(std::isfinite(p->huber) && p->huber > 0.0)) return "huber must be finite and > 0";
  if (!(std::isfinite(p->gate_max) && p->gate_max > 0.0)) return "gate_max must be finite and > 0";
  if (!(std::isfinite(p->min_disp) && p->min_disp > 0.0)) return "min_disp must be finite and > 0";
  if (p->iters < 0 || p->iters > kMaxIters) return "iters must be in 0 .. 16";
  if (p->min_inliers < 3) return "min_inliers must be >= 3";
  return nullptr;
}

extern "C" int me_frame_pose(me_ctx* c, const float* ref_uv, const float* ref_xr, const float* cur_uv,
                             const uint8_t* alive, int n, double f, double cx, double cy, double baseline,
                             const me_frame_pose_params* p, const void* start, float* err_out, void* info) {
  me_range range_("me_frame_pose");
  if (!c) return ME_ERR_INVALID;
  if (const char* why = me_frame_pose_check(p)) return me_set_error(c, ME_ERR_INVALID, "me_frame_pose: %s", why);
  ME_CHECK(c, n >= 0 && n <= (1 << 24), "me_frame_pose: n must be in 0 .. 2^24");
  ME_CHECK(c, n == 0 || ref_uv, "me_frame_pose: null ref_uv");
  ME_CHECK(c, n == 0 || ref_xr, "me_frame_pose: null ref_xr");
  ME_CHECK(c, n == 0 || cur_uv, "me_frame_pose: null cur_uv");
  ME_CHECK(c, n == 0 || alive, "me_frame_pose: null alive");
  ME_CHECK(c, std::isfinite(f) && f > 0.0, "me_frame_pose: f must be finite and > 0");
  ME_CHECK(c, std::isfinite(baseline) && baseline > 0.0, "me_frame_pose: baseline must be finite and > 0");
  ME_CHECK(c, std::isfinite(cx) && std::isfinite(cy), "me_frame_pose: cx and cy must be finite");
  ME_CHECK(c, info != nullptr, "me_frame_pose: null info");
  ME_CHECK(c, ((uintptr_t)info & 7) == 0, "me_frame_pose: info must be 8-byte aligned");
  ME_CHECK(c, ((uintptr_t)start & 7) == 0, "me_frame_pose: start must be 8-byte aligned");
  ME_HIP(c, hipSetDevice(c->device));
  const size_t nchunks = ((size_t)n + kChunk - 1) / kChunk;
  void* part;
  ME_TRY(me_scratch(c, SLOT_FPOSE, 8 * kSums * nchunks + 8, &part));
  FpArgs g{};
  g.ref_uv = ref_uv;
  g.ref_xr = ref_xr;
  g.cur_uv = cur_uv;
  g.alive = alive;
  g.n = n;
  g.f = f;
  g.cx = cx;
  g.cy = cy;
  g.fb = f * baseline;
  g.min_disp = p->min_disp;
  g.huber = p->huber;
  g.g2 = p->gate_max * p->gate_max;
  g.iters = p->iters;
  g.min_inliers = p->min_inliers;
  g.start = (const unsigned char*)start;
  g.part = (double*)part;
  g.err_out = err_out;
  g.info = (unsigned char*)info;
  // the ctx's own block, of a fixed size: allocated on first use.  The final kernel zeroes it for the next
  // call; a block that is new, or whose last call failed between its launches, is zeroed here instead.
  void* work;
  ME_TRY(me_scratch(c, SLOT_FPOSE_WORK, sizeof(FpWork), &work));
  g.work = (FpWork*)work;
  if (!c->fpose_armed) ME_HIP(c, hipMemsetAsync(work, 0, sizeof(FpWork), c->stream));
  c->fpose_armed = false;
  const unsigned grid = n > 0 ? (unsigned)((n + kBlock - 1) / kBlock) : 1u;
  for (int it = 0; it < (n > 0 ? p->iters : 0); ++it) {
    {
      me_ktimer tm(c, ME_KT_FRAMEPOSE);
      hipLaunchKernelGGL(fpose_iter_kernel, dim3(grid), dim3(kBlock), 0, c->stream, g, it);
    }
    ME_TRY(me_check_launch(c, "fpose_iter_kernel"));
  }
  if (n == 0) g.iters = 0;  // (no iteration launch ran: the final kernel takes the start pose)
  {
    me_ktimer tm(c, ME_KT_FRAMEPOSE);
    hipLaunchKernelGGL(fpose_final_kernel, dim3(grid), dim3(kBlock), 0, c->stream, g);
  }
  ME_TRY(me_check_launch(c, "fpose_final_kernel"));
  c->fpose_armed = true;
  return ME_OK;
}
