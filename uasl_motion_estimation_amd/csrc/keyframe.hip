// keyframe.hip — keyframe selection between the VO loop's keyframes
// (include/me_hip.h, section A12i; the numpy restatement is
// keyframe.kf_update_ref).
//
// One launch of one workgroup on the ctx stream folds a tracker result into
// the carried state and takes the keyframe decision:
//  1. every thread strides over the features: the alive test, cur_uv and the
//     alive byte updated in place, the 64-bit pattern of d2 (a non-negative
//     double: monotone as an unsigned integer) kept in LDS for the first kCache
//     features and formed again from cur_uv / ref_uv for the others;
//  2. the lower median of the alive d2 by a radix select over those patterns:
//     eight passes, most significant byte first, each a 256-bin LDS histogram
//     (integer LDS atomics) of the keys that share the prefix found so far,
//     then wave 0 scans the bins (a lane per four bins, shuffles) and picks the
//     bin the remaining rank falls in;
//  3. thread 0 forms the flags and writes the info block.
// Counts are integers and the selected value is an order statistic, so nothing
// depends on the order in which lanes or waves arrive.  FP64 + - * only; the
// library is built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include "me_internal.hpp"

namespace {

constexpr int kBlock = 256;   // threads of the one workgroup (= histogram bins)
constexpr int kCache = 2048;  // features whose d2 pattern is kept in LDS (16 KiB)
constexpr unsigned long long kDead = ~0ull;  // a feature that is not alive (no d2 of finite positions has this pattern)

struct KfArgs {
  const float* ref_uv;
  float* cur_uv;
  uint8_t* alive;
  const float* new_uv;
  const uint8_t* status;
  int n;
  float margin, wlim, hlim;  // wlim = (float)width - margin, hlim likewise
  int gap, max_gap, min_tracked_pct;
  double thr2;  // min_parallax * min_parallax
  unsigned char* info;
};

__device__ __forceinline__ unsigned long long d2_key(float u, float v, const float* ref) {
  const double dx = (double)u - (double)ref[0];
  const double dy = (double)v - (double)ref[1];
  const double d2 = (dx * dx) + (dy * dy);
  return (unsigned long long)__double_as_longlong(d2);
}

__global__ __launch_bounds__(kBlock) void kf_update_kernel(KfArgs g) {
  __shared__ unsigned long long s_key[kCache];
  __shared__ int s_hist[kBlock];
  __shared__ int s_m, s_bin, s_rank;
  const int tid = threadIdx.x, n = g.n;
  if (tid == 0) s_m = 0;
  s_hist[tid] = 0;
  __syncthreads();
  // 1. the update and the keys; feature k belongs to thread k % kBlock in every loop below
  int mine = 0;
  for (int k = tid; k < n; k += kBlock) {
    const float u = g.new_uv[2 * (size_t)k], v = g.new_uv[2 * (size_t)k + 1];
    const bool a = g.alive[k] != 0 && g.status[k] == 1 && isfinite(u) && isfinite(v) && u >= g.margin && u < g.wlim &&
                   v >= g.margin && v < g.hlim;
    if (a) {
      g.cur_uv[2 * (size_t)k] = u;
      g.cur_uv[2 * (size_t)k + 1] = v;
      ++mine;
    }
    g.alive[k] = a ? 1 : 0;
    if (k < kCache) s_key[k] = a ? d2_key(u, v, g.ref_uv + 2 * (size_t)k) : kDead;
  }
  if (mine) atomicAdd(&s_m, mine);
  __syncthreads();
  const int m = s_m;
  const int rank = (m - 1) >> 1;  // (-1 when nothing is alive)
  // 2. radix select of the element of that rank
  unsigned long long prefix = 0;
  if (m > 0) {  // (uniform)
    int want = rank;
    for (int p = 7; p >= 0; --p) {
      const int shift = 8 * p;
      const unsigned long long hi = p == 7 ? 0ull : ~0ull << (shift + 8);
      for (int k = tid; k < n; k += kBlock) {
        unsigned long long key;
        if (k < kCache) {
          key = s_key[k];
        } else {  // (this thread's own stores above: same thread, same index)
          key = g.alive[k] ? d2_key(g.cur_uv[2 * (size_t)k], g.cur_uv[2 * (size_t)k + 1], g.ref_uv + 2 * (size_t)k) : kDead;
        }
        if (key != kDead && (key & hi) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
      }
      __syncthreads();
      if (tid < 64) {  // wave 0: lane l owns bins 4 l .. 4 l + 3
        int c[4];
        for (int j = 0; j < 4; ++j) c[j] = s_hist[4 * tid + j];
        const int own = (c[0] + c[1]) + (c[2] + c[3]);
        int incl = own;
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d, 64);
          if (tid >= d) incl += up;
        }
        int before = incl - own;
        if (want >= before && want < incl) {  // (exactly one lane: the bins hold want + 1 keys or more)
          int j = 0;
          while (want >= before + c[j]) {
            before += c[j];
            ++j;
          }
          s_bin = 4 * tid + j;
          s_rank = want - before;
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)s_bin << shift;
      want = s_rank;
      s_hist[tid] = 0;
      __syncthreads();
    }
  }
  // 3. the decision
  if (tid == 0) {
    const double med2 = m > 0 ? __longlong_as_double((long long)prefix) : 0.0;
    int flags = 0;
    if (n == 0 || 100 * (long long)m < (long long)g.min_tracked_pct * (long long)n) flags |= 1;
    if (g.thr2 > 0.0 && med2 >= g.thr2) flags |= 2;  // (min_parallax = 0: the rule is off)
    if (g.gap >= g.max_gap) flags |= 4;
    int32_t* iw = (int32_t*)g.info;
    iw[0] = n;
    iw[1] = m;
    iw[2] = rank;
    iw[3] = flags;
    double* dw = (double*)(g.info + 16);
    dw[0] = med2;
    dw[1] = 0.0;
  }
}

}  // namespace

extern "C" void me_kf_default_params(me_kf_params* p) {
  if (!p) return;
  p->min_parallax = 12.0;
  p->min_tracked_pct = 60;
  p->max_gap = 10;
}

// The parameter checks the entry point and me_vo_loop_set_keyframe_select share: NULL on success, else the
// message, which names the argument.
const char* me_kf_check(const me_kf_params* p) {
  if (!p) return "null params";
  if (!(std::isfinite(p->min_parallax) && p->min_parallax >= 0.0)) return "min_parallax must be finite and >= 0";
  if (p->min_tracked_pct < 0 || p->min_tracked_pct > 100) return "min_tracked_pct must be in 0 .. 100";
  if (p->max_gap < 1) return "max_gap must be >= 1";
  return nullptr;
}

extern "C" int me_kf_update(me_ctx* c, const float* ref_uv, float* cur_uv, uint8_t* alive, const float* new_uv,
                            const uint8_t* status, int n, int width, int height, float margin, int gap,
                            const me_kf_params* p, void* info) {
  me_range range_("me_kf_update");
  if (!c) return ME_ERR_INVALID;
  if (const char* why = me_kf_check(p)) return me_set_error(c, ME_ERR_INVALID, "me_kf_update: %s", why);
  ME_CHECK(c, gap >= 1, "me_kf_update: gap must be >= 1");
  ME_CHECK(c, n >= 0, "me_kf_update: n must be >= 0");
  ME_CHECK(c, n == 0 || (ref_uv && cur_uv && alive && new_uv && status), "me_kf_update: null feature array");
  ME_CHECK(c, info != nullptr, "me_kf_update: null info");
  ME_CHECK(c, ((uintptr_t)info & 7) == 0, "me_kf_update: info must be 8-byte aligned");
  ME_CHECK(c, width >= 1 && height >= 1, "me_kf_update: width / height must be >= 1");
  ME_CHECK(c, std::isfinite(margin) && margin >= 0.0f, "me_kf_update: margin must be finite and >= 0");
  ME_HIP(c, hipSetDevice(c->device));
  KfArgs g{};
  g.ref_uv = ref_uv;
  g.cur_uv = cur_uv;
  g.alive = alive;
  g.new_uv = new_uv;
  g.status = status;
  g.n = n;
  g.margin = margin;
  g.wlim = (float)width - margin;
  g.hlim = (float)height - margin;
  g.gap = gap;
  g.max_gap = p->max_gap;
  g.min_tracked_pct = p->min_tracked_pct;
  g.thr2 = p->min_parallax * p->min_parallax;
  g.info = (unsigned char*)info;
  {
    me_ktimer tm(c, ME_KT_KEYFRAME);
    hipLaunchKernelGGL(kf_update_kernel, dim3(1), dim3(kBlock), 0, c->stream, g);
  }
  return me_check_launch(c, "kf_update_kernel");
}
