// tonemap.hip — 16-bit ingest: a 16 -> 8-bit tone map on the device
// (build-defined and integer-only; no reference: it restates no OpenCV function
// and parity is unpinned).
//
// The definition is stated in me_hip.h (section A12g) and restated in numpy in
// uasl_motion_estimation_amd/tonemap.py (tonemap_ref), the checker.  The window
// needs two order statistics of the frame, not its 65 536-bin histogram: a
// two-level radix select finds them, and its results are by construction those
// of the full histogram.  Three kernels:
//  * tonemap_select_kernel<0>, the coarse pass: 256-bin histograms of the high
//    byte.  Every wave owns kCopies histograms in LDS (257 words apart, one per
//    value of the lane's low bits: clahe_table_kernel's answer to images whose
//    lanes meet on a few words), a thread takes 8 pixels at a time (one aligned
//    16-byte load; elements before a row's first aligned address and at its
//    ragged end) and adds a run of equal bins once with its length.  The
//    workgroup's non-zero sums go to a global table with integer atomic adds.
//    The workgroup that arrives last on the pass's ticket scans the table,
//    finds the high bytes B_lo / B_hi holding ranks k_lo and N - k_hi and the
//    ranks left inside them, and re-arms table and ticket.
//  * tonemap_select_kernel<1>, the fine pass: the same over the low byte of the
//    pixels whose high byte is B_lo or B_hi (two tables; one when B_lo == B_hi).
//    The last arrival finds lo and hi, does steps 2-4 of the definition on one
//    thread, updates the state, publishes lo_u, hi_u, span and 1.0f / span, and
//    re-arms.
//  * tonemap_apply_kernel: the same walk; 8 pixels per 16-byte load, one 8-byte
//    store where the destination's address allows, bytes otherwise.  q / span
//    is a float estimate put right by the remainder: exact for every span in
//    1..65535 and every q < 2^24.
// Nobody waits for anybody: tickets only.  Every cross-workgroup sum is an
// integer add, so nothing depends on scheduling.  Stride padding is neither
// read as pixels nor written.
#include <algorithm>
#include <climits>
#include "me_internal.hpp"

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kUnit = 8;    // pixels a thread takes at a time: one 16-byte load
constexpr int kCopies = 4;  // histograms per wave and table, chosen by the lane's low bits
constexpr int kHistStride = 257;  // words between two histograms: an odd stride puts the copies of a bin in
                                  // different LDS banks
constexpr int kHists = kWaves * kCopies;
constexpr int kTable = kHists * kHistStride;  // words of one table's copies
constexpr int kUnitsPerBlock = 512;  // units a workgroup aims at (two per thread)
constexpr int kMaxBlocks = 1024;     // and the most workgroups a pass launches

// the words of a state's (or the ctx's stateless) device block
enum : int {
  W_COARSE = 0,      // 256: the coarse table
  W_FINE = 256,      // 2 x 256: the fine tables of B_lo and B_hi
  W_TICKET = 768,    // 2: one per pass
  W_SEL = 770,       // B_lo, B_hi, rank left in B_lo (0-based), rank left in B_hi (1-based)
  W_WIN = 776,       // lo_u, hi_u, span, bits of 1.0f / span
  W_STATE = 780,     // lo_q8, hi_q8, frames
  W_COUNT = 784
};

struct WalkArgs {
  int w, h, stride;  // stride in elements
  int upr;           // units per row: (w + 7) / 8 + 1 (the first one holds the elements before the aligned address)
  int rows;          // rows per workgroup
  float rupr;        // 1.0f / upr
};

// n / den for n below 2^24: a float estimate, off by one at the most, put right by the remainder.
__device__ __forceinline__ uint32_t div_small(uint32_t n, uint32_t den, float rden) {
  uint32_t q = (uint32_t)((float)n * rden);
  const int32_t r = (int32_t)(n - q * den);
  if (r < 0)
    --q;
  else if ((uint32_t)r >= den)
    ++q;
  return q;
}

__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Unit q of the workgroup's rows: the row, the first column x0 (may be negative: the elements before the row's
// first 16-byte aligned address make the first unit) and the columns [xa, xb) that are pixels.  False past the end.
__device__ __forceinline__ bool unit_of(const WalkArgs& g, const uint16_t* src, int q, int& y, int& x0, int& xa,
                                        int& xb, const uint16_t*& row) {
  const int r = g.rows == 1 ? 0 : (int)div_small((uint32_t)q, (uint32_t)g.upr, g.rupr);
  y = blockIdx.x * g.rows + r;
  if (y >= g.h) return false;
  const int u = q - r * g.upr;
  row = src + (long)y * g.stride;
  const int head = (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1;  // elements
  x0 = head + kUnit * (u - 1);
  xa = max(x0, 0);
  xb = min(x0 + kUnit, g.w);
  return true;
}

// Inclusive scan of one value per thread over threads 0..255 (the other threads keep the barriers company).
__device__ __forceinline__ uint32_t scan256(uint32_t c, uint32_t* red /* kWaves words */) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(c, off, 64);
    if (lane >= off) c += t;
  }
  __syncthreads();  // (red may still be read from the scan before)
  if (lane == 63) red[wv] = c;
  __syncthreads();
  for (int k = 0; k < wv; ++k) c += red[k];
  return c;
}

struct SelectArgs {
  uint32_t n, k_lo, t_hi;  // pixels, rank of lo (0-based), N - k_hi (1-based)
  int min_span, alpha_q8, stateless;
};

// kPass 0: coarse (high byte), 1: fine (low byte of the pixels in B_lo / B_hi)
template <int kPass>
__global__ __launch_bounds__(kBlock) void tonemap_select_kernel(const uint16_t* __restrict__ src, WalkArgs g,
                                                                SelectArgs s, uint32_t* work) {
  __shared__ uint32_t hist[(kPass ? 2 : 1) * kTable];
  __shared__ uint32_t red[kWaves];
  __shared__ int flag[3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int k = tid; k < (kPass ? 2 : 1) * kTable; k += kBlock) hist[k] = 0;
  // (written by the coarse pass's last workgroup in the launch before: plain loads)
  const uint32_t b_lo = kPass ? work[W_SEL + 0] : 0u, b_hi = kPass ? work[W_SEL + 1] : 0u;
  __syncthreads();

  // 1. the histogram(s) of the workgroup's rows
  uint32_t* mine = hist + (wv * kCopies + (lane & (kCopies - 1))) * kHistStride;
  constexpr uint32_t kNone = 0xffffffffu;
  auto bin = [&](uint32_t v) -> uint32_t {
    if (!kPass) return v >> 8;
    const uint32_t hb = v >> 8;
    return hb == b_lo ? (v & 255u) : (hb == b_hi ? (uint32_t)kTable + (v & 255u) : kNone);
  };
  const int units = g.upr * g.rows;
  for (int q = tid; q < units; q += kBlock) {
    int y, x0, xa, xb;
    const uint16_t* row;
    if (!unit_of(g, src, q, y, x0, xa, xb, row)) break;  // (rows past the image: every later unit as well)
    if (xb - xa < kUnit) {  // a row's unaligned head or ragged end: element by element
      for (int x = xa; x < xb; ++x) {
        const uint32_t b = bin(row[x]);
        if (b != kNone) atomicAdd(&mine[b], 1u);
      }
      continue;
    }
    const uint4 wd = *reinterpret_cast<const uint4*>(row + x0);  // (16-byte aligned by construction)
    const uint32_t wds[4] = {wd.x, wd.y, wd.z, wd.w};
    // a run of one bin adds once with its length
    uint32_t cur = bin(wds[0] & 0xffffu), cnt = 0;
#pragma unroll
    for (int i = 0; i < kUnit; ++i) {
      const uint32_t b = bin((wds[i >> 1] >> (16 * (i & 1))) & 0xffffu);
      if (b != cur) {
        if (cur != kNone) atomicAdd(&mine[cur], cnt);
        cur = b;
        cnt = 0;
      }
      ++cnt;
    }
    if (cur != kNone) atomicAdd(&mine[cur], cnt);
  }
  __syncthreads();

  // 2. the workgroup's sums to the global table(s): integer adds
  uint32_t* tab = work + (kPass ? W_FINE : W_COARSE);
  for (int t = 0; t < (kPass ? 2 : 1); ++t) {
    uint32_t c = 0;
    for (int k = 0; k < kHists; ++k) c += hist[t * kTable + k * kHistStride + tid];
    if (c) __hip_atomic_fetch_add(&tab[t * 256 + tid], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // 3. the ticket: whoever arrives last goes on, everybody else is done.  Every wave drains its own adds
  // first (vmcnt is per wave and the barrier waits for no counter): an add still in flight at the arrival
  // could miss the last workgroup's scan and land in the re-armed table instead
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    flag[0] = __hip_atomic_fetch_add(&work[W_TICKET + kPass], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
              gridDim.x - 1;
  __syncthreads();
  if (!flag[0]) return;

  if (!kPass) {
    // 4a. the high bytes that hold the two ranks, and the ranks left inside them
    const uint32_t hv = ld_agent(&tab[tid]);
    const uint32_t c = scan256(hv, red);
    if (hv != 0 && c > s.k_lo && c - hv <= s.k_lo) {
      work[W_SEL + 0] = (uint32_t)tid;
      work[W_SEL + 2] = s.k_lo - (c - hv);
    }
    if (hv != 0 && c >= s.t_hi && c - hv < s.t_hi) {
      work[W_SEL + 1] = (uint32_t)tid;
      work[W_SEL + 3] = s.t_hi - (c - hv);
    }
    tab[tid] = 0;  // re-armed for the next call (this launch's end publishes it)
    if (tid == 0) work[W_TICKET + 0] = 0;
    return;
  }
  // 4b. lo and hi inside their high bytes
  const uint32_t r_lo = work[W_SEL + 2], r_hi = work[W_SEL + 3];
  const uint32_t ha = ld_agent(&tab[tid]);
  const uint32_t hb = b_lo == b_hi ? ha : ld_agent(&tab[256 + tid]);
  const uint32_t ca = scan256(ha, red);
  const uint32_t cb = scan256(hb, red);
  if (ha != 0 && ca > r_lo && ca - ha <= r_lo) flag[1] = (int)((b_lo << 8) | (uint32_t)tid);
  if (hb != 0 && cb >= r_hi && cb - hb < r_hi) flag[2] = (int)((b_hi << 8) | (uint32_t)tid);
  tab[tid] = 0;
  tab[256 + tid] = 0;
  __syncthreads();
  if (tid != 0) return;
  work[W_TICKET + 1] = 0;
  // steps 2 - 4 of the definition
  int lo = flag[1], hi = flag[2];
  const int sp = hi - lo;
  if (sp < s.min_span) {
    lo -= (s.min_span - sp) / 2;
    if (lo < 0) lo = 0;
    hi = lo + s.min_span;
    if (hi > 65535) {
      hi = 65535;
      lo = 65535 - s.min_span;
    }
  }
  int* st = reinterpret_cast<int*>(work + W_STATE);
  long long lo_q8 = (long long)lo << 8, hi_q8 = (long long)hi << 8;
  if (!s.stateless) {
    const int frames = st[2];
    if (frames != 0) {
      const long long pl = st[0], ph = st[1];
      lo_q8 = pl + (((lo_q8 - pl) * s.alpha_q8) >> 8);
      hi_q8 = ph + (((hi_q8 - ph) * s.alpha_q8) >> 8);
    }
    st[0] = (int)lo_q8;
    st[1] = (int)hi_q8;
    st[2] = frames == INT_MAX ? INT_MAX : frames + 1;
  }
  const int lo_u = (int)(lo_q8 >> 8), hi_u = (int)((hi_q8 + 255) >> 8);
  const int span = max(1, hi_u - lo_u);
  work[W_WIN + 0] = (uint32_t)lo_u;
  work[W_WIN + 1] = (uint32_t)hi_u;
  work[W_WIN + 2] = (uint32_t)span;
  work[W_WIN + 3] = __float_as_uint(1.0f / (float)span);
}

__device__ __forceinline__ uint32_t map_pixel(uint32_t v, uint32_t lo_u, uint32_t hi_u, uint32_t span, float rspan) {
  if (v < lo_u) return 0u;
  const uint32_t q = (min(v, hi_u) - lo_u) * 255u + (span >> 1);  // below 2^24
  return min(255u, div_small(q, span, rspan));
}

__global__ __launch_bounds__(kBlock) void tonemap_apply_kernel(const uint16_t* __restrict__ src, WalkArgs g,
                                                               const uint32_t* __restrict__ work,
                                                               uint8_t* __restrict__ dst, int dst_stride) {
  // (written by the fine pass's last workgroup in the launch before: plain loads)
  const uint32_t lo_u = work[W_WIN + 0], hi_u = work[W_WIN + 1], span = work[W_WIN + 2];
  const float rspan = __uint_as_float(work[W_WIN + 3]);
  const int units = g.upr * g.rows;
  for (int q = threadIdx.x; q < units; q += kBlock) {
    int y, x0, xa, xb;
    const uint16_t* row;
    if (!unit_of(g, src, q, y, x0, xa, xb, row)) break;
    uint8_t* o = dst + (long)y * dst_stride;
    if (xb - xa < kUnit) {
      for (int x = xa; x < xb; ++x) o[x] = (uint8_t)map_pixel(row[x], lo_u, hi_u, span, rspan);
      continue;
    }
    const uint4 wd = *reinterpret_cast<const uint4*>(row + x0);
    const uint32_t wds[4] = {wd.x, wd.y, wd.z, wd.w};
    uint32_t out[kUnit];
#pragma unroll
    for (int i = 0; i < kUnit; ++i)
      out[i] = map_pixel((wds[i >> 1] >> (16 * (i & 1))) & 0xffffu, lo_u, hi_u, span, rspan);
    o += x0;
    if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
      uint2 pk;
      pk.x = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
      pk.y = out[4] | (out[5] << 8) | (out[6] << 16) | (out[7] << 24);
      *reinterpret_cast<uint2*>(o) = pk;
    } else {
#pragma unroll
      for (int i = 0; i < kUnit; ++i) o[i] = (uint8_t)out[i];
    }
  }
}

// Rows per workgroup and the grid of the walk the three kernels share.
WalkArgs walk_of(int width, int height, int stride, unsigned* blocks) {
  WalkArgs g;
  g.w = width;
  g.h = height;
  g.stride = stride;
  g.upr = (width + kUnit - 1) / kUnit + 1;
  g.rows = std::max(std::max(1, kUnitsPerBlock / g.upr), (height + kMaxBlocks - 1) / kMaxBlocks);
  g.rows = std::min(g.rows, height);
  g.rupr = 1.0f / (float)g.upr;
  *blocks = (unsigned)((height + g.rows - 1) / g.rows);
  return g;
}

}  // namespace

struct me_tonemap_state {
  me_ctx* ctx = nullptr;
  uint32_t* work = nullptr;  // W_COUNT words of device memory
  bool armed = false;        // tables and tickets are zero: set by a call whose launches all went out
};

extern "C" void me_tonemap_default_params(me_tonemap_params* p) {
  if (!p) return;
  p->lo_ppm = 1000;
  p->hi_ppm = 1000;
  p->min_span = 256;
  p->alpha_q8 = 64;
}

// The parameter checks every entry point shares (me_vo_loop_set_tonemap as well): NULL on success, else the
// message, which names the argument.
const char* me_tonemap_check(const me_tonemap_params* p) {
  if (!p) return "null params";
  if (p->lo_ppm < 0) return "lo_ppm must be >= 0";
  if (p->hi_ppm < 0) return "hi_ppm must be >= 0";
  if ((long)p->lo_ppm + (long)p->hi_ppm >= 1000000L) return "lo_ppm + hi_ppm must be < 10^6";
  if (p->min_span < 1 || p->min_span > 65535) return "min_span must be in 1 .. 65535";
  if (p->alpha_q8 < 1 || p->alpha_q8 > 256) return "alpha_q8 must be in 1 .. 256";
  return nullptr;
}

extern "C" int me_tonemap_state_create(me_ctx* c, me_tonemap_state** st) {
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, st != nullptr, "me_tonemap_state_create: null st");
  *st = nullptr;
  ME_HIP(c, hipSetDevice(c->device));
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, W_COUNT * sizeof(uint32_t));
  if (e != hipSuccess)
    return me_set_error(c, ME_ERR_NOMEM, "me_tonemap_state_create: hipMalloc failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(p, 0, W_COUNT * sizeof(uint32_t), c->stream);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return me_set_error(c, ME_ERR_HIP, "me_tonemap_state_create: hipMemsetAsync failed: %s", hipGetErrorString(e));
  }
  me_tonemap_state* s = new me_tonemap_state;
  s->ctx = c;
  s->work = (uint32_t*)p;
  s->armed = true;
  *st = s;
  return ME_OK;
}

extern "C" int me_tonemap_state_destroy(me_tonemap_state* st) {
  if (!st) return ME_OK;
  me_ctx* c = st->ctx;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(st->work);
  delete st;
  return ME_OK;
}

extern "C" int me_tonemap_state_reset(me_tonemap_state* st) {
  if (!st) return ME_ERR_INVALID;
  me_ctx* c = st->ctx;
  ME_HIP(c, hipSetDevice(c->device));
  ME_HIP(c, hipMemsetAsync(st->work + W_STATE + 2, 0, sizeof(uint32_t), c->stream));
  return ME_OK;
}

extern "C" int me_tonemap_state_read(me_tonemap_state* st, int32_t out[3]) {
  if (!st) return ME_ERR_INVALID;
  me_ctx* c = st->ctx;
  ME_CHECK(c, out != nullptr, "me_tonemap_state_read: null out");
  ME_HIP(c, hipSetDevice(c->device));
  ME_HIP(c, hipMemcpyAsync(out, st->work + W_STATE, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  return ME_OK;
}

extern "C" int me_tonemap16(me_ctx* c, me_mem mem, const uint16_t* src, int width, int height, int src_stride,
                            uint8_t* dst, int dst_stride, const me_tonemap_params* p, me_tonemap_state* state) {
  me_range range_("me_tonemap16");
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, src != nullptr, "me_tonemap16: null src");
  ME_CHECK(c, dst != nullptr, "me_tonemap16: null dst");
  if (const char* why = me_tonemap_check(p)) return me_set_error(c, ME_ERR_INVALID, "me_tonemap16: %s", why);
  ME_CHECK(c, width >= 1, "me_tonemap16: width must be >= 1");
  ME_CHECK(c, height >= 1, "me_tonemap16: height must be >= 1");
  ME_CHECK(c, src_stride >= width, "me_tonemap16: src_stride must be >= width");
  ME_CHECK(c, dst_stride >= width, "me_tonemap16: dst_stride must be >= width");
  ME_CHECK(c, (long)src_stride * height < (1L << 30), "me_tonemap16: src_stride * height must be < 2^30");
  ME_CHECK(c, (long)dst_stride * height < (1L << 30), "me_tonemap16: dst_stride * height must be < 2^30");
  ME_CHECK(c, state == nullptr || state->ctx == c, "me_tonemap16: state belongs to another ctx");
  ME_CHECK(c, (reinterpret_cast<uintptr_t>(src) & 1) == 0, "me_tonemap16: src must be 2-byte aligned");
  ME_HIP(c, hipSetDevice(c->device));
  const long long n = (long long)width * height;
  SelectArgs s;
  s.n = (uint32_t)n;
  s.k_lo = (uint32_t)((long long)p->lo_ppm * n / 1000000LL);
  s.t_hi = (uint32_t)(n - (long long)p->hi_ppm * n / 1000000LL);
  s.min_span = p->min_span;
  s.alpha_q8 = p->alpha_q8;
  s.stateless = state == nullptr;
  uint32_t* work;
  bool* armed;
  if (state) {
    work = state->work;
    armed = &state->armed;
  } else {
    // the ctx's own block, of a fixed size: allocated on first use
    void* base;
    ME_TRY(me_scratch(c, SLOT_TONEMAP_WORK, W_COUNT * sizeof(uint32_t), &base));
    work = (uint32_t*)base;
    armed = &c->tonemap_armed;
  }
  // The select kernels zero tables and tickets for the next call.  A block that is new, or whose last call
  // failed between its launches, is zeroed here instead (the state words stay): a failure heals itself.
  if (!*armed) ME_HIP(c, hipMemsetAsync(work, 0, W_STATE * sizeof(uint32_t), c->stream));
  *armed = false;
  const size_t src_elems = (size_t)src_stride * (height - 1) + width;
  const size_t dst_bytes = (size_t)dst_stride * (height - 1) + width;
  const uint16_t* dsrc = src;
  uint8_t* ddst = dst;
  if (mem == ME_HOST) {
    // one slot: src | dst, each part 16-byte aligned
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    void* base;
    ME_TRY(me_scratch(c, SLOT_TONEMAP, up(2 * src_elems) + up(dst_bytes), &base));
    ME_HIP(c, hipMemcpyAsync(base, src, 2 * src_elems, hipMemcpyHostToDevice, c->stream));
    dsrc = (const uint16_t*)base;
    ddst = (uint8_t*)base + up(2 * src_elems);
  }
  unsigned blocks;
  const WalkArgs g = walk_of(width, height, src_stride, &blocks);
  {
    me_ktimer t(c, ME_KT_TONEMAP);
    hipLaunchKernelGGL(tonemap_select_kernel<0>, dim3(blocks), dim3(kBlock), 0, c->stream, dsrc, g, s, work);
  }
  ME_TRY(me_check_launch(c, "tonemap_select_kernel<0>"));
  {
    me_ktimer t(c, ME_KT_TONEMAP);
    hipLaunchKernelGGL(tonemap_select_kernel<1>, dim3(blocks), dim3(kBlock), 0, c->stream, dsrc, g, s, work);
  }
  ME_TRY(me_check_launch(c, "tonemap_select_kernel<1>"));
  {
    me_ktimer t(c, ME_KT_TONEMAP);
    hipLaunchKernelGGL(tonemap_apply_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, dsrc, g,
                       (const uint32_t*)work, ddst, dst_stride);
  }
  ME_TRY(me_check_launch(c, "tonemap_apply_kernel"));
  *armed = true;
  if (mem == ME_HOST) {
    // row by row: the caller's stride padding keeps its bytes
    ME_HIP(c, hipMemcpy2DAsync(dst, dst_stride, ddst, dst_stride, width, height, hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipStreamSynchronize(c->stream));
  }
  return ME_OK;
}
