// clahe.hip — contrast-limited adaptive histogram equalisation on the device
// (build-defined and integer-only; no reference: OpenCV's float CLAHE is not
// restated and parity with it is unpinned).
//
// The definition is stated in me_hip.h (section A12e) and restated in numpy in
// uasl_motion_estimation_amd/equalise.py (clahe_ref), the checker.  Two kernels
// (DESIGN.md 5.10 has the measurements behind the choices):
//  * clahe_table_kernel: one workgroup of 16 waves per tile.
//    1. every wave owns kCopies 256-bin histograms in LDS (64 KB in all; 257
//       words apart, so that the copies of a value sit in different banks), one
//       per value of the lane's low bits, and walks the tile's rows in units
//       of 16 columns: one 16-byte load where the unit lies inside the image
//       and the tile, bytes with the reflect-101 index otherwise.  Counts are
//       integers (ds_add_u32): the result cannot depend on arrival order.  A
//       run of equal pixels inside a unit adds once with its length.  Copies
//       and runs are the answer to the low-contrast image, on which the lanes
//       of a wave meet on a few LDS words and are served one after the other;
//       -DME_CLAHE_NO_RUNS builds the kernel with one add per pixel;
//    2. threads 0..255 sum the copies of their bin; the excess over the clip
//       limit is reduced with shuffles and four LDS words; clip, redistribute,
//       scan (shuffles inside the wave, the wave totals through LDS), and 256
//       LUT bytes leave.
//  * clahe_apply_kernel<kRows>: remap_q5_kernel's shape, 64 pixels wide, four
//    horizontally adjacent pixels per thread in each of kRows rows 16 apart
//    (4 rows on large images, 1 on small ones: me_clahe chooses).
//    1. the thread's pixels are loaded first (one dword per row where the row
//       holds all four, bytes at the ragged right edge);
//    2. the tables the workgroup's pixels can blend -- at most 3 x 3 when the
//       tiles are no smaller than the workgroup's pixels -- are staged in LDS
//       as words; a workgroup that touches more than 9 tables (small images
//       with many tiles) gathers from global memory instead; the choice
//       depends on blockIdx alone.  -DME_CLAHE_NO_STAGE builds the kernel with
//       the global gathers only;
//    3. i0 / i1 / fx by one division and three increments, j0 / j1 / fy once
//       per row; divisions are a float estimate put right by the remainder
//       (exact); the blend is the definition's sum with the four weights
//       multiplied out, in the 24-bit multiplier (exact: every factor < 2^24);
//    4. one dword store where the row's address allows, bytes otherwise.
//    A thread reads its pixels before it writes them and nobody else reads
//    them: dst == src works.
// Stride padding is neither read as pixels nor written.
#include <algorithm>
#include <cmath>
#include "me_internal.hpp"

namespace {

constexpr int kTableBlock = 1024, kTableWaves = kTableBlock / 64;
constexpr int kUnit = 16;  // pixels a thread of the table kernel takes at a time
constexpr int kCopies = 4;  // histograms per wave, chosen by the lane's low bits
constexpr int kHistStride = 257;  // words between two histograms: an odd stride puts the copies of a value in
                                  // different LDS banks
constexpr int kHists = kTableWaves * kCopies;
constexpr int kTW = 64, kRowStep = 16, kBlock = 256, kPix = 4;
constexpr int kStageTables = 9;  // tables the apply kernel stages in LDS: up to 3 x 3, what a tile of an image with
                                 // tiles of 64 x 16 pixels and more touches
constexpr int kMaxTiles = 16;
constexpr long kMaxArea = 1L << 20;
static_assert(kBlock == (kTW / kPix) * kRowStep, "one thread per four pixels of a row");

__device__ __forceinline__ int reflect101(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

// n / den where the quotient is small (at most 2^20, n below 2^24; or at most 256, n below 2^31): a float
// estimate, off by one at the most, put right by the remainder.  rden = 1.0f / den from the host.
__device__ __forceinline__ uint32_t div_small(uint32_t n, uint32_t den, float rden) {
  uint32_t q = (uint32_t)((float)n * rden);
  const int32_t r = (int32_t)(n - __umul24(q, den));
  if (r < 0)
    --q;
  else if ((uint32_t)r >= den)
    ++q;
  return q;
}

__global__ __launch_bounds__(kTableBlock) void clahe_table_kernel(const uint8_t* __restrict__ src, int w, int h,
                                                                  int stride, int tw, int th, uint32_t lim,
                                                                  float rupr, uint8_t* __restrict__ lut) {
  __shared__ uint32_t hist[kHists * kHistStride];
  __shared__ uint32_t red[8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x_lo = blockIdx.x * tw, y_lo = blockIdx.y * th;
  const uint32_t area = (uint32_t)tw * (uint32_t)th;

  for (int k = tid; k < kHists * kHistStride; k += kTableBlock) hist[k] = 0;
  __syncthreads();

  // 1. the histogram of the thread's share of the tile, in units of kUnit columns of a row
  uint32_t* mine = hist + (wv * kCopies + (lane & (kCopies - 1))) * kHistStride;
  const int upr = (tw + kUnit - 1) / kUnit;
  const int units = upr * th;
  // columns below x_in can be read as they lie: inside the image, no mirror
  const int x_hi = x_lo + tw, x_in = min(x_hi, w);
  for (int q = tid; q < units; q += kTableBlock) {
    const int r = (int)div_small((uint32_t)q, (uint32_t)upr, rupr), u = q - r * upr;
    const int x = x_lo + kUnit * u;
    const uint8_t* row = src + (long)reflect101(y_lo + r, h) * stride;
    if (x + kUnit - 1 >= x_in) {  // the tile's ragged or mirrored end: pixel by pixel
      for (int i = 0; i < kUnit; ++i)
        if (x + i < x_hi) atomicAdd(&mine[row[reflect101(x + i, w)]], 1u);
      continue;
    }
    uint32_t wd[kUnit / 4];
    __builtin_memcpy(wd, row + x, kUnit);  // (one 16-byte load; global memory takes it at any alignment)
#ifndef ME_CLAHE_NO_RUNS
    // runs of one value add once with their length: on the low-contrast image, whose lanes meet on a few LDS
    // words and are served one after the other, that is a fraction of the adds; on noise it changes nothing
    uint32_t cur = wd[0] & 255u, cnt = 0;
#pragma unroll
    for (int i = 0; i < kUnit; ++i) {
      const uint32_t v = (wd[i >> 2] >> (8 * (i & 3))) & 255u;
      if (v != cur) {
        atomicAdd(&mine[cur], cnt);
        cur = v;
        cnt = 0;
      }
      ++cnt;
    }
    atomicAdd(&mine[cur], cnt);
#else
#pragma unroll
    for (int i = 0; i < kUnit; ++i) atomicAdd(&mine[(wd[i >> 2] >> (8 * (i & 3))) & 255u], 1u);
#endif
  }
  __syncthreads();

  // 2. bins on threads 0..255 (waves 0..3); the other waves only keep the barriers company
  const bool bin = tid < 256;
  uint32_t c = 0;
  if (bin)
    for (int k = 0; k < kHists; ++k) c += hist[k * kHistStride + tid];
  uint32_t ex = c > lim ? c - lim : 0u;
  for (int off = 32; off > 0; off >>= 1) ex += __shfl_xor(ex, off, 64);
  if (bin && lane == 0) red[wv] = ex;
  __syncthreads();
  const uint32_t excess = red[0] + red[1] + red[2] + red[3];
  c = min(c, lim) + excess / 256u;
  const uint32_t rem = excess % 256u;
  if (rem > 0) {
    const uint32_t step = max(256u / rem, 1u);
    if ((uint32_t)tid % step == 0 && (uint32_t)tid / step < rem) c += 1;
  }
  // inclusive scan of the 256 counts
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(c, off, 64);
    if (lane >= off) c += t;
  }
  if (bin && lane == 63) red[4 + wv] = c;
  __syncthreads();
  if (bin) {
    for (int k = 0; k < wv; ++k) c += red[4 + k];
    lut[((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] = (uint8_t)((255u * c + area / 2u) / area);
  }
}

// floor((2 p + 1 - t) / (2 t)), the unclamped index of the tile whose centre lies at or before pixel p
__device__ __forceinline__ int tile_before(int p, int t, float r2t) {
  const int a = 2 * p + 1 - t;
  return a < 0 ? -1 : (int)div_small((uint32_t)a, 2u * (uint32_t)t, r2t);
}
__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

struct ApplyArgs {
  int w, h, src_stride, dst_stride, tw, th, tiles_x, tiles_y;
  float r2tw, r2th, rden;  // 1 / (2 tw), 1 / (2 th), 1 / (4 tw th)
};

// kRows rows per thread, 16 apart: a workgroup covers 64 x (16 kRows) pixels
template <int kRows>
__global__ __launch_bounds__(kBlock) void clahe_apply_kernel(const uint8_t* src, ApplyArgs g,
                                                             const uint8_t* __restrict__ lut, uint8_t* dst) {
  __shared__ uint32_t staged[kStageTables * 64];
  const int tid = threadIdx.x;
  constexpr int kTH = kRowStep * kRows;
  const int x = blockIdx.x * kTW + (tid & 15) * kPix, y0 = blockIdx.y * kTH + (tid >> 4);
  const int w = g.w, h = g.h, tw = g.tw, th = g.th, tiles_x = g.tiles_x, tiles_y = g.tiles_y;
  // the thread's pixels first: four of each of its kRows rows (y0, y0 + 16, ...), every load under way
  // before the tables are staged
  const bool whole = x + 3 < w;
  uint32_t px[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + r * kRowStep;
    px[r] = 0;
    if (y < h && x < w) {
      const uint8_t* s = src + (long)y * g.src_stride + x;
      if (whole) {
        __builtin_memcpy(&px[r], s, 4);
      } else {
        for (int i = 0; i < kPix; ++i)
          if (x + i < w) px[r] |= (uint32_t)s[i] << (8 * i);
      }
    }
  }
  // the tables the workgroup's pixels blend: columns ia .. ib, rows ja .. jb (the same in every thread)
  const int ia = clampi(tile_before(blockIdx.x * kTW, tw, g.r2tw), tiles_x - 1);
  const int ib = clampi(tile_before(min((int)blockIdx.x * kTW + kTW, w) - 1, tw, g.r2tw) + 1, tiles_x - 1);
  const int ja = clampi(tile_before(blockIdx.y * kTH, th, g.r2th), tiles_y - 1);
  const int jb = clampi(tile_before(min((int)blockIdx.y * kTH + kTH, h) - 1, th, g.r2th) + 1, tiles_y - 1);
  const int nx = ib - ia + 1, ny = jb - ja + 1;
#ifndef ME_CLAHE_NO_STAGE
  const bool stage = nx * ny <= kStageTables;
#else
  const bool stage = false;
#endif
  if (stage) {
    // table t of the staged block is (ja + t / nx, ia + t % nx); a wave copies one table at a time
    int jj = 0, ii = tid >> 6;
    for (int t = tid >> 6; t < nx * ny; t += kBlock / 64) {
      while (ii >= nx) {
        ii -= nx;
        ++jj;
      }
      uint32_t v;  // (lut_out of a caller may sit at any address)
      __builtin_memcpy(&v, lut + ((long)(ja + jj) * tiles_x + ia + ii) * 256 + 4 * (tid & 63), 4);
      staged[t * 64 + (tid & 63)] = v;
      ii += kBlock / 64;
    }
    __syncthreads();
  }
  if (x >= w) return;
  // the first pixel's pair of tile columns; the next three follow by increments (2 <= 2 tw)
  const int i0u_first = tile_before(x, tw, g.r2tw);
  const uint32_t fx_first = (uint32_t)(2 * x + 1 - tw - i0u_first * 2 * tw);
  const uint32_t wx = 2u * (uint32_t)tw;
  const uint32_t half = wx * (uint32_t)th, den = 2u * half;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + r * kRowStep;
    if (y >= h) break;
    // the row's pair of tile rows
    const int j0u = tile_before(y, th, g.r2th);
    const uint32_t fy = (uint32_t)(2 * y + 1 - th - j0u * 2 * th), gy = 2u * (uint32_t)th - fy;
    const int j0 = clampi(j0u, tiles_y - 1), j1 = clampi(j0u + 1, tiles_y - 1);
    const uint8_t *l0 = lut + (long)j0 * tiles_x * 256, *l1 = lut + (long)j1 * tiles_x * 256;
    const int s0 = ((j0 - ja) * nx - ia) * 64, s1 = ((j1 - ja) * nx - ia) * 64;  // staged table (j, i): word s + 64 i
    int i0u = i0u_first;
    uint32_t fx = fx_first;
    uint32_t out[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const uint32_t v = (px[r] >> (8 * i)) & 255u;
      const int i0 = clampi(i0u, tiles_x - 1), i1 = clampi(i0u + 1, tiles_x - 1);
      uint32_t a, b, c, d;
      if (stage) {  // (the same in every thread; whole words of the LDS array, the byte picked in registers)
        const uint32_t sh = 8u * (v & 3u);
        const int o0 = i0 * 64 + (int)(v >> 2), o1 = i1 * 64 + (int)(v >> 2);
        a = (staged[s0 + o0] >> sh) & 255u;
        b = (staged[s0 + o1] >> sh) & 255u;
        c = (staged[s1 + o0] >> sh) & 255u;
        d = (staged[s1 + o1] >> sh) & 255u;
      } else {
        const int o0 = i0 * 256 + (int)v, o1 = i1 * 256 + (int)v;
        a = l0[o0], b = l0[o1], c = l1[o0], d = l1[o1];
      }
      // (top (2th - fy) + bot fy) with the four weights multiplied out: every factor is below 2^24 (a weight is
      // at most 4 tw th <= 2^22), so the 24-bit multiplier gives the exact 32-bit sums of the definition
      const uint32_t gx = wx - fx;
      const uint32_t n = __umul24(a, __umul24(gx, gy)) + __umul24(b, __umul24(fx, gy)) +
                         __umul24(c, __umul24(gx, fy)) + __umul24(d, __umul24(fx, fy)) + half;
      out[i] = div_small(n, den, g.rden);
      fx += 2;
      if (fx >= wx) {
        fx -= wx;
        ++i0u;
      }
    }
    uint8_t* o = dst + (long)y * g.dst_stride + x;
    if (whole && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i)
        if (x + i < w) o[i] = (uint8_t)out[i];
    }
  }
}

}  // namespace

// Rows per thread of the apply kernel for an image: 4 where that still leaves every CU four workgroups and
// more, else 1
static int apply_rows(const me_ctx* c, int width, int height) {
  const long gx = (width + kTW - 1) / kTW, gy4 = (height + 4 * kRowStep - 1) / (4 * kRowStep);
  return gx * gy4 >= 4L * std::max(1, c->num_cu) ? 4 : 1;
}

extern "C" int me_clahe_apply_rows(me_ctx* c, int width, int height) {
  if (!c || width < 1 || height < 1) return ME_ERR_INVALID;
  return apply_rows(c, width, height);
}

extern "C" void me_clahe_default_params(me_clahe_params* p) {
  if (!p) return;
  p->tiles_x = 8;
  p->tiles_y = 8;
  p->clip_limit = 3.0;
}

// The parameter checks every entry point shares (me_vo_loop_set_equalise as well): NULL on success,
// else the message, which names the argument.
const char* me_clahe_check(const me_clahe_params* p, int width, int height) {
  if (!p) return "null params";
  if (width < 1 || height < 1) return "width / height must be >= 1";
  if (p->tiles_x < 1 || p->tiles_x > kMaxTiles || p->tiles_x > width) return "tiles_x must be in 1 .. min(width, 16)";
  if (p->tiles_y < 1 || p->tiles_y > kMaxTiles || p->tiles_y > height) return "tiles_y must be in 1 .. min(height, 16)";
  if (!(std::isfinite(p->clip_limit) && p->clip_limit >= 0.0)) return "clip_limit must be finite and >= 0";
  const long tw = (width + p->tiles_x - 1) / p->tiles_x, th = (height + p->tiles_y - 1) / p->tiles_y;
  if (tw * th > kMaxArea) return "area (tile width * tile height) must be <= 2^20";
  return nullptr;
}

extern "C" int me_clahe(me_ctx* c, me_mem mem, const uint8_t* src, int width, int height, int src_stride,
                        const me_clahe_params* p, uint8_t* dst, int dst_stride, uint8_t* lut_out) {
  me_range range_("me_clahe");
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, src != nullptr, "me_clahe: null src");
  ME_CHECK(c, dst != nullptr, "me_clahe: null dst");
  if (const char* why = me_clahe_check(p, width, height)) return me_set_error(c, ME_ERR_INVALID, "me_clahe: %s", why);
  ME_CHECK(c, src_stride >= width, "me_clahe: src_stride must be >= width");
  ME_CHECK(c, dst_stride >= width, "me_clahe: dst_stride must be >= width");
  ME_CHECK(c, (long)src_stride * height < (1L << 31), "me_clahe: src_stride * height must be < 2^31");
  ME_CHECK(c, (long)dst_stride * height < (1L << 31), "me_clahe: dst_stride * height must be < 2^31");
  ME_HIP(c, hipSetDevice(c->device));
  const int tx = p->tiles_x, ty = p->tiles_y;
  const int tw = (width + tx - 1) / tx, th = (height + ty - 1) / ty;
  const long area = (long)tw * th;
  // the clip limit, once, in FP64
  uint32_t lim = (uint32_t)area;
  if (p->clip_limit != 0.0) {
    const double q = std::floor(p->clip_limit * (double)area / 256.0);
    lim = q >= (double)area ? (uint32_t)area : (q < 1.0 ? 1u : (uint32_t)q);
  }
  const size_t lut_bytes = (size_t)tx * ty * 256, lut_room = (size_t)kMaxTiles * kMaxTiles * 256;
  const size_t src_bytes = (size_t)src_stride * (height - 1) + width;
  const size_t dst_bytes = (size_t)dst_stride * (height - 1) + width;
  const uint8_t* dsrc = src;
  uint8_t *ddst = dst, *dlut = lut_out;
  if (mem == ME_HOST) {
    // one slot: lut | src | dst, each part 16-byte aligned
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    void* base;
    ME_TRY(me_scratch(c, SLOT_CLAHE, lut_room + up(src_bytes) + up(dst_bytes), &base));
    uint8_t* b = (uint8_t*)base;
    dlut = b;
    b += lut_room;
    ME_HIP(c, hipMemcpyAsync(b, src, src_bytes, hipMemcpyHostToDevice, c->stream));
    dsrc = b;
    b += up(src_bytes);
    // dst == src with equal strides: the kernels run in place on the staged copy, as they would on the device
    ddst = (dst == src && dst_stride == src_stride) ? const_cast<uint8_t*>(dsrc) : b;
  } else if (!dlut) {
    void* base;
    ME_TRY(me_scratch(c, SLOT_CLAHE, lut_room, &base));
    dlut = (uint8_t*)base;
  }
  {
    me_ktimer t(c, ME_KT_CLAHE);
    hipLaunchKernelGGL(clahe_table_kernel, dim3(tx, ty), dim3(kTableBlock), 0, c->stream, dsrc, width, height,
                       src_stride, tw, th, lim, 1.0f / (float)((tw + kUnit - 1) / kUnit), dlut);
  }
  ME_TRY(me_check_launch(c, "clahe_table_kernel"));
  {
    me_ktimer t(c, ME_KT_CLAHE);
    const ApplyArgs g{width,          height,
                      src_stride,     dst_stride,
                      tw,             th,
                      tx,             ty,
                      0.5f / (float)tw, 0.5f / (float)th,
                      0.25f / ((float)tw * (float)th)};
    // four rows per thread where that still leaves every CU four workgroups and more (the staging and the
    // latency of a pixel load are paid once per thread); one row per thread on smaller images
    const unsigned gx = (width + kTW - 1) / kTW, gy4 = (height + 4 * kRowStep - 1) / (4 * kRowStep);
    if (apply_rows(c, width, height) == 4)
      hipLaunchKernelGGL(clahe_apply_kernel<4>, dim3(gx, gy4), dim3(kBlock), 0, c->stream, dsrc, g, dlut, ddst);
    else
      hipLaunchKernelGGL(clahe_apply_kernel<1>, dim3(gx, (height + kRowStep - 1) / kRowStep), dim3(kBlock), 0,
                         c->stream, dsrc, g, dlut, ddst);
  }
  ME_TRY(me_check_launch(c, "clahe_apply_kernel"));
  if (mem == ME_HOST) {
    // row by row: the caller's stride padding keeps its bytes
    ME_HIP(c, hipMemcpy2DAsync(dst, dst_stride, ddst, dst_stride, width, height, hipMemcpyDeviceToHost, c->stream));
    if (lut_out) ME_HIP(c, hipMemcpyAsync(lut_out, dlut, lut_bytes, hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipStreamSynchronize(c->stream));
  }
  return ME_OK;
}
