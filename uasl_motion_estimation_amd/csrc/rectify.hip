// rectify.hip — stereo rectification on the device (build-defined; no reference).
//
// The reference takes undistorted, row-aligned images and leaves the warp to
// the caller; the definition is stated in me_hip.h (section A12d) and restated
// in numpy in uasl_motion_estimation_amd/rectify.py, the checker.  Two kernels:
//  * rectify_map_kernel: one thread per rectified pixel, the header's formulas
//    operation by operation in the round-to-nearest FP64 intrinsics (nothing
//    for the compiler to contract or reorder), one 8-byte store per pixel.
//    Runs once per calibration.
//  * remap_q5_kernel: the per-frame warp, one 64 x 16 tile of destination
//    pixels per workgroup, four horizontally adjacent pixels per thread.
//    1. each thread loads its four map entries (two 16-byte loads when the
//       map's rows keep them aligned, four 8-byte loads otherwise) and keeps
//       them in registers;
//    2. the bounding box of the taps that touch the image is reduced with
//       shuffles inside each wave, then over the four waves through LDS (no
//       atomics); thread 0 alone decides the path and shares the decision and
//       the box through LDS, so the branch ahead of the barriers is uniform;
//    3. path 0: the box is staged in LDS as whole 32-bit words of four pixels
//       (word-aligned in source x, `border` substituted outside the image,
//       odd word stride so that neighbouring rows sit on different banks);
//       a pixel's two taps of a row come from two ds_read_b32 and one
//       v_alignbyte, never from byte-wide LDS traffic;
//    4. path 1 (box larger than the staging buffer: strong rotation,
//       decimation, wild maps): the taps come from global memory, each judged
//       against the image on its own;
//    5. four pixels leave as one dword where the row's address allows, bytes
//       otherwise (ragged right edge, unaligned rows); padding is not written.
//    tile_path receives the path per tile from one lane (plain store).
// -DME_REMAP_NO_STAGE builds the kernel without path 0 (timing experiments,
// tools/build_variant.sh).
#include <climits>
#include <cmath>
#include "me_internal.hpp"

namespace {

constexpr int kTW = 64, kTH = 16, kBlock = 256, kPix = 4;
constexpr int kStageWords = 4095;  // 63 * 65: an odd row stride can fill it exactly
static_assert(kBlock == (kTW / kPix) * kTH, "one thread per four pixels of the tile");

struct MapArgs {
  double fx_r, fy_r, cx_r, cy_r;
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  double R[9];
};

__global__ __launch_bounds__(256) void rectify_map_kernel(MapArgs m, int w, int h, int2* __restrict__ map) {
  const int u = blockIdx.x * 64 + (threadIdx.x & 63), v = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (u >= w || v >= h) return;
  const double x = __ddiv_rn(__dsub_rn((double)u, m.cx_r), m.fx_r);
  const double y = __ddiv_rn(__dsub_rn((double)v, m.cy_r), m.fy_r);
  const double X = __dadd_rn(__dadd_rn(__dmul_rn(m.R[0], x), __dmul_rn(m.R[3], y)), m.R[6]);
  const double Y = __dadd_rn(__dadd_rn(__dmul_rn(m.R[1], x), __dmul_rn(m.R[4], y)), m.R[7]);
  const double W = __dadd_rn(__dadd_rn(__dmul_rn(m.R[2], x), __dmul_rn(m.R[5], y)), m.R[8]);
  const double a = __ddiv_rn(X, W), b = __ddiv_rn(Y, W);
  const double a2 = __dmul_rn(a, a), b2 = __dmul_rn(b, b), r2 = __dadd_rn(a2, b2);
  const double tab = __dmul_rn(2.0, __dmul_rn(a, b));
  const double rad = __dadd_rn(
      1.0, __dmul_rn(r2, __dadd_rn(m.k1, __dmul_rn(r2, __dadd_rn(m.k2, __dmul_rn(r2, m.k3))))));
  const double xd = __dadd_rn(__dadd_rn(__dmul_rn(a, rad), __dmul_rn(m.p1, tab)),
                              __dmul_rn(m.p2, __dadd_rn(r2, __dmul_rn(2.0, a2))));
  const double yd = __dadd_rn(__dadd_rn(__dmul_rn(b, rad), __dmul_rn(m.p1, __dadd_rn(r2, __dmul_rn(2.0, b2)))),
                              __dmul_rn(m.p2, tab));
  const double us = __dadd_rn(__dmul_rn(m.fx, xd), m.cx), vs = __dadd_rn(__dmul_rn(m.fy, yd), m.cy);
  const double lim = 16777216.0;  // 2^24
  int2 e = make_int2(INT_MIN, INT_MIN);
  if (W > 0.0 && fabs(us) < lim && fabs(vs) < lim)  // (all false for NaN)
    e = make_int2((int)rint(__dmul_rn(us, 32.0)), (int)rint(__dmul_rn(vs, 32.0)));
  map[(long)v * w + u] = e;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ int blend(int p00, int p10, int p01, int p11, int fxq, int fyq) {
  return (p00 * (32 - fxq) * (32 - fyq) + p10 * fxq * (32 - fyq) + p01 * (32 - fxq) * fyq + p11 * fxq * fyq + 512) >>
         10;
}

__global__ __launch_bounds__(kBlock) void remap_q5_kernel(const uint8_t* __restrict__ src, int src_w, int src_h,
                                                          int src_stride, const int2* __restrict__ map, int dst_w,
                                                          int dst_h, int border, uint8_t* __restrict__ dst,
                                                          int dst_stride, int map_vec, uint8_t* __restrict__ tile_path) {
  // [0, kStageWords]: the staged box (+ 1 word the last tap pair may load and not use);
  // then 16 words of the wave reductions and 6 of the decision
  __shared__ uint32_t lds[kStageWords + 1 + 16 + 6];
  int* red = reinterpret_cast<int*>(lds + kStageWords + 1);
  int* dec = red + 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x = blockIdx.x * kTW + (tid & 15) * kPix, y = blockIdx.y * kTH + (tid >> 4);
  const bool row_in = y < dst_h;

  // 1. the thread's map entries; a pixel outside the destination gets an entry that touches nothing
  int2 e[kPix];
#pragma unroll
  for (int i = 0; i < kPix; ++i) e[i] = make_int2(INT_MIN, INT_MIN);
  if (row_in && x < dst_w) {
    const int2* mp = map + (long)y * dst_w + x;
    if (map_vec && x + 3 < dst_w) {
      const int4 a = *reinterpret_cast<const int4*>(mp), b = *reinterpret_cast<const int4*>(mp + 2);
      e[0] = make_int2(a.x, a.y);
      e[1] = make_int2(a.z, a.w);
      e[2] = make_int2(b.x, b.y);
      e[3] = make_int2(b.z, b.w);
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i)
        if (x + i < dst_w) e[i] = mp[i];
    }
  }

  // 2. bounding box of the taps of the entries that touch the image, clamped to [-1, src_w] x [-1, src_h]
  int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    const int sx = e[i].x >> 5, sy = e[i].y >> 5;
    if (sx >= -1 && sx <= src_w - 1 && sy >= -1 && sy <= src_h - 1) {
      x0 = min(x0, sx);
      x1 = max(x1, sx + 1);
      y0 = min(y0, sy);
      y1 = max(y1, sy + 1);
    }
  }
  x0 = wave_min(x0);
  y0 = wave_min(y0);
  x1 = wave_max(x1);
  y1 = wave_max(y1);
  if (lane == 0) {
    red[4 * wv] = x0;
    red[4 * wv + 1] = y0;
    red[4 * wv + 2] = x1;
    red[4 * wv + 3] = y1;
  }
  __syncthreads();
  if (tid == 0) {  // one thread decides: the branch below is uniform by construction
    for (int k = 1; k < kBlock / 64; ++k) {
      x0 = min(x0, red[4 * k]);
      y0 = min(y0, red[4 * k + 1]);
      x1 = max(x1, red[4 * k + 2]);
      y1 = max(y1, red[4 * k + 3]);
    }
    int path = 0, xa = 0, nw = 0, rows = 0, sw = 1;
    if (x1 >= x0) {
      xa = (x0 >> 2) * 4;  // (arithmetic shift: -1 -> -4)
      nw = (x1 >> 2) - (x0 >> 2) + 1;
      rows = y1 - y0 + 1;
      sw = (nw + 1) | 1;
      if ((long)rows * sw > (long)kStageWords) path = 1;
    }
#ifdef ME_REMAP_NO_STAGE
    if (x1 >= x0) path = 1;
#endif
    dec[0] = path;
    dec[1] = xa;
    dec[2] = y0;
    dec[3] = nw;
    dec[4] = rows;
    dec[5] = sw;
    if (tile_path) tile_path[(long)blockIdx.y * gridDim.x + blockIdx.x] = (uint8_t)path;
  }
  __syncthreads();
  const int path = dec[0];
  const uint32_t bw = (uint32_t)border * 0x01010101u;
  int out[kPix];

  if (path == 0) {
    const int xa = dec[1], ya = dec[2], nw = dec[3], rows = dec[4], sw = dec[5];
    // 3. stage the box: word (i, k) = source pixels (ya + i, xa + 4k .. xa + 4k + 3)
    for (int q = tid; q < rows * nw; q += kBlock) {
      const int i = q / nw, k = q - i * nw;
      const int ys = ya + i, xs = xa + 4 * k;
      uint32_t v = bw;
      if (ys >= 0 && ys < src_h) {
        const uint8_t* row = src + (long)ys * src_stride;
        if (xs >= 0 && xs + 3 < src_w) {
          __builtin_memcpy(&v, row + xs, 4);
        } else {
          v = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int xx = xs + j;
            const uint32_t p = (xx >= 0 && xx < src_w) ? (uint32_t)row[xx] : (uint32_t)border;
            v |= p << (8 * j);
          }
        }
      }
      lds[i * sw + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int sx = e[i].x >> 5, sy = e[i].y >> 5;
      int r = border;
      if (sx >= -1 && sx <= src_w - 1 && sy >= -1 && sy <= src_h - 1) {
        const int cx = sx - xa, k = cx >> 2, sh = cx & 3;
        const uint32_t* p = lds + (sy - ya) * sw + k;
        // bytes sh, sh + 1 of the word pair: taps sx and sx + 1 of a row
        const uint32_t t = __builtin_amdgcn_alignbyte(p[1], p[0], sh);
        const uint32_t b = __builtin_amdgcn_alignbyte(p[sw + 1], p[sw], sh);
        r = blend((int)(t & 255u), (int)((t >> 8) & 255u), (int)(b & 255u), (int)((b >> 8) & 255u), e[i].x & 31,
                  e[i].y & 31);
      }
      out[i] = r;
    }
  } else {
    // 4. taps from global memory, each judged on its own
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int sx = e[i].x >> 5, sy = e[i].y >> 5;
      int r = border;
      if (sx >= -1 && sx <= src_w - 1 && sy >= -1 && sy <= src_h - 1) {
        const bool xl = sx >= 0, xr = sx + 1 < src_w, yt = sy >= 0, yb = sy + 1 < src_h;
        const uint8_t* p = src + (long)sy * src_stride + sx;
        const int p00 = (xl && yt) ? p[0] : border, p10 = (xr && yt) ? p[1] : border;
        const int p01 = (xl && yb) ? p[src_stride] : border, p11 = (xr && yb) ? p[src_stride + 1] : border;
        r = blend(p00, p10, p01, p11, e[i].x & 31, e[i].y & 31);
      }
      out[i] = r;
    }
  }

  // 5. the four pixels: one dword where the address allows, bytes otherwise
  if (row_in && x < dst_w) {
    uint8_t* o = dst + (long)y * dst_stride + x;
    if (x + 3 < dst_w && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) =
          (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < kPix; ++i)
        if (x + i < dst_w) o[i] = (uint8_t)out[i];
    }
  }
}

bool finite_all(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// Argument checks of a camera / rectified model
int check_models(me_ctx* c, const char* who, const me_camera_model* cam, const me_rectified_model* rect) {
  if (cam) {
    ME_CHECK(c, cam->width >= 1 && cam->height >= 1 && (long)cam->width * cam->height < (1L << 31),
             "%s: camera model width / height must be >= 1 (and width * height < 2^31)", who);
    const double k[4] = {cam->fx, cam->fy, cam->cx, cam->cy};
    ME_CHECK(c, finite_all(k, 4), "%s: camera model fx / fy / cx / cy must be finite", who);
    ME_CHECK(c, cam->fx > 0.0 && cam->fy > 0.0, "%s: camera model fx and fy must be > 0", who);
    ME_CHECK(c, finite_all(cam->dist, 5), "%s: camera model dist must be finite", who);
    ME_CHECK(c, finite_all(cam->R, 9), "%s: camera model R must be finite", who);
  }
  if (rect) {
    ME_CHECK(c, rect->width >= 1 && rect->height >= 1 && (long)rect->width * rect->height < (1L << 31),
             "%s: rectified model width / height must be >= 1 (and width * height < 2^31)", who);
    const double k[4] = {rect->fx, rect->fy, rect->cx, rect->cy};
    ME_CHECK(c, finite_all(k, 4), "%s: rectified model fx / fy / cx / cy must be finite", who);
    ME_CHECK(c, rect->fx > 0.0 && rect->fy > 0.0, "%s: rectified model fx and fy must be > 0", who);
  }
  return ME_OK;
}

}  // namespace

extern "C" int me_rectify_map(me_ctx* c, me_mem mem, const me_camera_model* cam, const me_rectified_model* rect,
                              int32_t* map) {
  me_range range_("me_rectify_map");
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, cam != nullptr, "me_rectify_map: null camera model");
  ME_CHECK(c, rect != nullptr, "me_rectify_map: null rectified model");
  ME_CHECK(c, map != nullptr, "me_rectify_map: null map");
  ME_TRY(check_models(c, "me_rectify_map", cam, rect));
  ME_HIP(c, hipSetDevice(c->device));
  const int w = rect->width, h = rect->height;
  const size_t bytes = 8 * (size_t)w * h;
  int32_t* dmap = map;
  if (mem == ME_HOST) {
    void* p;
    ME_TRY(me_scratch(c, SLOT_RECTIFY, bytes, &p));
    dmap = (int32_t*)p;
  }
  MapArgs m{rect->fx, rect->fy, rect->cx, rect->cy, cam->fx,      cam->fy,      cam->cx,
            cam->cy,  cam->dist[0], cam->dist[1], cam->dist[2], cam->dist[3], cam->dist[4], {}};
  for (int k = 0; k < 9; ++k) m.R[k] = cam->R[k];
  {
    me_ktimer t(c, ME_KT_RECTIFY);
    hipLaunchKernelGGL(rectify_map_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, c->stream, m, w, h,
                       reinterpret_cast<int2*>(dmap));
  }
  ME_TRY(me_check_launch(c, "rectify_map_kernel"));
  if (mem == ME_HOST) {
    ME_HIP(c, hipMemcpyAsync(map, dmap, bytes, hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipStreamSynchronize(c->stream));
  }
  return ME_OK;
}

extern "C" int me_remap_tile_dims(int* tw, int* th, int* stage_words) {
  if (!tw || !th) return ME_ERR_INVALID;
  *tw = kTW;
  *th = kTH;
  if (stage_words) *stage_words = kStageWords;
  return ME_OK;
}

extern "C" int me_remap_q5(me_ctx* c, me_mem mem, const uint8_t* src, int src_w, int src_h, int src_stride,
                           const int32_t* map, int dst_w, int dst_h, int border, uint8_t* dst, int dst_stride,
                           uint8_t* tile_path) {
  me_range range_("me_remap_q5");
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, src != nullptr, "me_remap_q5: null src");
  ME_CHECK(c, map != nullptr, "me_remap_q5: null map");
  ME_CHECK(c, dst != nullptr, "me_remap_q5: null dst");
  ME_CHECK(c, src_w >= 1 && src_h >= 1 && (long)src_w * src_h < (1L << 31),
           "me_remap_q5: src_w / src_h must be >= 1 (and src_w * src_h < 2^31)");
  ME_CHECK(c, src_stride >= src_w && (long)src_stride * src_h < (1L << 31),
           "me_remap_q5: src_stride must be >= src_w");
  ME_CHECK(c, dst_w >= 1 && dst_h >= 1 && (long)dst_w * dst_h < (1L << 31),
           "me_remap_q5: dst_w / dst_h must be >= 1 (and dst_w * dst_h < 2^31)");
  ME_CHECK(c, dst_stride >= dst_w && (long)dst_stride * dst_h < (1L << 31),
           "me_remap_q5: dst_stride must be >= dst_w");
  ME_CHECK(c, border >= 0 && border <= 255, "me_remap_q5: border must be in 0..255");
  ME_HIP(c, hipSetDevice(c->device));
  const dim3 grid((dst_w + kTW - 1) / kTW, (dst_h + kTH - 1) / kTH);
  const size_t ntile = (size_t)grid.x * grid.y;
  const uint8_t* dsrc = src;
  const int32_t* dmap = map;
  uint8_t *ddst = dst, *dpath = tile_path;
  const size_t src_bytes = (size_t)src_stride * (src_h - 1) + src_w;
  const size_t dst_bytes = (size_t)dst_stride * (dst_h - 1) + dst_w;
  const size_t map_bytes = 8 * (size_t)dst_w * dst_h;
  if (mem == ME_HOST) {
    // one slot: map | src | dst | tile_path, each part 16-byte aligned
    auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
    void* base;
    ME_TRY(me_scratch(c, SLOT_RECTIFY, up(map_bytes) + up(src_bytes) + up(dst_bytes) + up(ntile), &base));
    uint8_t* b = (uint8_t*)base;
    ME_HIP(c, hipMemcpyAsync(b, map, map_bytes, hipMemcpyHostToDevice, c->stream));
    dmap = (const int32_t*)b;
    b += up(map_bytes);
    ME_HIP(c, hipMemcpyAsync(b, src, src_bytes, hipMemcpyHostToDevice, c->stream));
    dsrc = b;
    b += up(src_bytes);
    ddst = b;
    b += up(dst_bytes);
    dpath = tile_path ? b : nullptr;
  }
  ME_CHECK(c, (reinterpret_cast<uintptr_t>(dmap) & 7) == 0, "me_remap_q5: map must be 8-byte aligned");
  // 16-byte map loads: every group of four entries (x a multiple of 4) starts on a 16-byte boundary
  const int map_vec = (reinterpret_cast<uintptr_t>(dmap) & 15) == 0 && (dst_w & 1) == 0;
  {
    me_ktimer t(c, ME_KT_RECTIFY);
    hipLaunchKernelGGL(remap_q5_kernel, grid, dim3(kBlock), 0, c->stream, dsrc, src_w, src_h, src_stride,
                       reinterpret_cast<const int2*>(dmap), dst_w, dst_h, border, ddst, dst_stride, map_vec, dpath);
  }
  ME_TRY(me_check_launch(c, "remap_q5_kernel"));
  if (mem == ME_HOST) {
    // row by row: the caller's stride padding keeps its bytes
    ME_HIP(c, hipMemcpy2DAsync(dst, dst_stride, ddst, dst_stride, dst_w, dst_h, hipMemcpyDeviceToHost, c->stream));
    if (tile_path) ME_HIP(c, hipMemcpyAsync(tile_path, dpath, ntile, hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipStreamSynchronize(c->stream));
  }
  return ME_OK;
}
