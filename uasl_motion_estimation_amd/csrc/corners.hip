// corners.hip — corner detector of the VO loop (build-defined; no reference).
//
// The reference contains no detector (the app that drove it is absent); the
// definition is stated in me_hip.h (section A12b) and restated in numpy in
// uasl_motion_estimation_amd/corners.py, the checker.  The response of a pixel
// is the KLT's own acceptance quantity -- the minimum eigenvalue of the
// structure tensor of the win x win window centred on it, in the KLT's integer
// formulation (klt.hip) -- so a new track starts where the tracker's test is
// strongest.  MI355X design:
//  * corner_response_kernel: one 64 x 32 tile of output pixels per workgroup.
//    The u8 tile plus a (half + 1)-pixel halo is staged in LDS as whole 32-bit
//    words (reflect-101 at the image border); Scharr derivatives and the three
//    products run in registers; the win x win sum is separable: a sliding
//    horizontal sum per (gradient row, 16-column segment) in int32
//    (31 * 4080^2 < 2^31) written to LDS, then a sliding vertical sum per
//    output column in int64 (441 * 4080^2 > 2^32), the FP64 value, one
//    coalesced store per row.  LDS rows have an odd word stride and the lanes
//    of a wave walk different rows (horizontal pass) or different columns
//    (vertical pass): every ds access is an aligned b32 without bank conflicts.
//  * corner_cells_kernel: one workgroup per grid cell scans the cell's pixel
//    rectangle, applies the 3 x 3 key test on the map and reduces the cell's
//    best corner by a 64-bit compare (response bits, then index) -- shuffles
//    and LDS, no atomics, nothing depends on scheduling.
//  * corner_select_kernel: vo_cells_kernel's selection (occupancy bits of the
//    good tracked features, block scan over "unoccupied and holds a corner",
//    the first `want` cells emitted in order).  One workgroup.
#include <algorithm>
#include <cmath>
#include "me_internal.hpp"

namespace {

constexpr int kTX = 64, kTY = 32, kBlock = 256, kSeg = 16;
constexpr int kMinWin = 3, kMaxWin = 31;
static_assert(kBlock == kTX * (kTY / 8), "vertical pass: one thread per column and 8 rows");
static_assert(kTX % kSeg == 0 && kSeg % 4 == 0, "segments start on a staged word");
static_assert((long)kMaxWin * 4080 * 4080 < (1L << 31), "row sums fit int32");

__device__ __forceinline__ int refl(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
  }
  return i;
}

// word stride of the staged rows: the tile's columns plus one word the column
// walker may load past them, odd (rows on different banks)
__host__ __device__ constexpr int tile_stride(int half) {
  const int words = (kTX + 2 * half + 2 + 3) / 4 + 1;
  return words | 1;
}
constexpr int kSumStride = kTX + 1;  // row-sum rows, odd
__host__ __device__ constexpr size_t response_lds_bytes(int half) {
  return 4 * ((size_t)(kTY + 2 * half + 2) * tile_stride(half) + 3 * (size_t)(kTY + 2 * half) * kSumStride);
}

// Walks three staged rows (y - 1, y, y + 1) along x, one aligned word per row
// and four columns: per column the Scharr smoothing t0 = 3 (a + c) + 10 b and
// difference t1 = c - a of the three pixels.
struct ColWalker {
  const uint32_t* p;
  int sw, j;
  uint32_t w0, w1, w2;
  __device__ __forceinline__ void load() {
    const int k = j >> 2;
    w0 = p[k];
    w1 = p[sw + k];
    w2 = p[2 * sw + k];
  }
  __device__ __forceinline__ void seek(const uint32_t* rows, int stride, int j0) {
    p = rows;
    sw = stride;
    j = j0;
    load();
  }
  __device__ __forceinline__ void next(int& t0, int& t1) {
    const int sh = 8 * (j & 3);
    const int a = (int)((w0 >> sh) & 255u), b = (int)((w1 >> sh) & 255u), c = (int)((w2 >> sh) & 255u);
    t0 = 3 * (a + c) + 10 * b;
    t1 = c - a;
    ++j;
    if ((j & 3) == 0) load();  // (uniform: every walker of a pass starts on the same column mod 4)
  }
};
// Scharr derivatives (scharr_levels_kernel's integers) of consecutive pixels of a row
struct GradWalker {
  ColWalker c;
  int t0a, t1a, t0b, t1b;
  __device__ __forceinline__ void seek(const uint32_t* rows, int stride, int g0) {
    c.seek(rows, stride, g0);
    c.next(t0a, t1a);
    c.next(t0b, t1b);
  }
  __device__ __forceinline__ void next(int& dx, int& dy) {
    int t0c, t1c;
    c.next(t0c, t1c);
    dx = t0c - t0a;
    dy = 3 * (t1c + t1a) + 10 * t1b;
    t0a = t0b;
    t1a = t1b;
    t0b = t0c;
    t1b = t1c;
  }
};

__global__ __launch_bounds__(kBlock) void corner_response_kernel(const uint8_t* __restrict__ img, int w, int h,
                                                                 int stride, int win, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int half = (win - 1) / 2;
  const int ri = kTY + 2 * half + 2;  // staged image rows
  const int rg = kTY + 2 * half;      // gradient rows
  const int sw = tile_stride(half);
  uint32_t* tile = lds;                                        // [ri][sw] words of four pixels
  int* sums = reinterpret_cast<int*>(lds + (size_t)ri * sw);   // [3][rg][kSumStride]
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;

  // 1. the tile and its halo: staged (i, j) = image (y0 - half - 1 + i, x0 - half - 1 + j), reflect-101
  for (int q = tid; q < ri * sw; q += kBlock) {
    const int i = q / sw, k = q - i * sw;
    const uint8_t* row = img + (long)refl(y0 - half - 1 + i, h) * stride;
    const int xs = x0 - half - 1 + 4 * k;
    uint32_t v;
    if (xs >= 0 && xs + 3 < w) {
      __builtin_memcpy(&v, row + xs, 4);
    } else {
      v = (uint32_t)row[refl(xs, w)] | ((uint32_t)row[refl(xs + 1, w)] << 8) | ((uint32_t)row[refl(xs + 2, w)] << 16) |
          ((uint32_t)row[refl(xs + 3, w)] << 24);
    }
    tile[q] = v;
  }
  __syncthreads();

  // 2. horizontal sums: gradient row g = image row y0 - half + g (staged rows g .. g + 2), gradient
  // column c = image column x0 - half + c (staged columns c .. c + 2); sums[.][g][c] = the win
  // products from gradient column c on.  Rows outside the image feed no valid output: skipped.
  for (int task = tid; task < rg * (kTX / kSeg); task += kBlock) {
    const int s = task / rg, g = task - s * rg;
    const int y = y0 - half + g, c0 = s * kSeg;
    if (y < 0 || y >= h || x0 + c0 >= w) continue;
    GradWalker lead, trail;
    lead.seek(tile + (size_t)g * sw, sw, c0);
    trail.seek(tile + (size_t)g * sw, sw, c0);
    int s11 = 0, s12 = 0, s22 = 0, dx, dy;
    for (int k = 0; k < win; ++k) {
      lead.next(dx, dy);
      s11 += dx * dx;
      s12 += dx * dy;
      s22 += dy * dy;
    }
    int* o = sums + (size_t)g * kSumStride + c0;
    o[0] = s11;
    o[(size_t)rg * kSumStride] = s12;
    o[2 * (size_t)rg * kSumStride] = s22;
    for (int c = 1; c < kSeg; ++c) {
      int ex, ey;
      lead.next(dx, dy);
      trail.next(ex, ey);
      s11 += dx * dx - ex * ex;
      s12 += dx * dy - ex * ey;
      s22 += dy * dy - ey * ey;
      o[c] = s11;
      o[(size_t)rg * kSumStride + c] = s12;
      o[2 * (size_t)rg * kSumStride + c] = s22;
    }
  }
  __syncthreads();

  // 3. vertical sums and the value: thread = (column, 8 rows); the window of output row ty is
  // gradient rows ty .. ty + win - 1.  Valid pixels (the KLT's level-0 test) are contiguous.
  const int tx = tid & (kTX - 1), x = x0 + tx;
  if (x >= w) return;
  const bool xvalid = x >= half && x <= w - half - 2;
  const double FLT_SCALE = 1.0 / (1 << 20);
  const int* c11 = sums + tx;
  const int* c12 = c11 + (size_t)rg * kSumStride;
  const int* c22 = c12 + (size_t)rg * kSumStride;
  long A11 = 0, A12 = 0, A22 = 0;
  bool have = false;
  const int ty0 = (tid / kTX) * 8;
  for (int q = 0; q < 8; ++q) {
    const int ty = ty0 + q, y = y0 + ty;
    if (y >= h) break;
    double R = 0.0;
    if (xvalid && y >= half && y <= h - half - 2) {
      if (!have) {
        A11 = A12 = A22 = 0;
        for (int k = 0; k < win; ++k) {
          A11 += c11[(ty + k) * kSumStride];
          A12 += c12[(ty + k) * kSumStride];
          A22 += c22[(ty + k) * kSumStride];
        }
        have = true;
      } else {
        A11 += c11[(ty + win - 1) * kSumStride] - c11[(ty - 1) * kSumStride];
        A12 += c12[(ty + win - 1) * kSumStride] - c12[(ty - 1) * kSumStride];
        A22 += c22[(ty + win - 1) * kSumStride] - c22[(ty - 1) * kSumStride];
      }
      // the KLT's expression and operation order (klt.hip, oracle/klt.cpp:115-117)
      const double a11 = (double)A11 * FLT_SCALE, a12 = (double)A12 * FLT_SCALE, a22 = (double)A22 * FLT_SCALE;
      R = __ddiv_rn(a22 + a11 - __dsqrt_rn((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12), 2.0 * win * win);
    }
    out[(long)y * w + x] = R;
  }
}

// Key of a corner: larger response first (positive doubles order as their
// bits), then the smaller row-major index.
struct Key {
  unsigned long long r;
  int idx;
};
__device__ __forceinline__ bool beats(unsigned long long r, int idx, const Key& k) {
  return r > k.r || (r == k.r && idx < k.idx);
}

__device__ __forceinline__ int cell_of(float u, float margin, double c, int n) {
  return min(max((int)(((double)u - (double)margin) / c), 0), n - 1);
}
__device__ __forceinline__ bool inside_margin(float u, float v, int width, int height, float margin) {
  return u >= margin && u < (float)width - margin && v >= margin && v < (float)height - margin;
}

// best[cell] = row-major index of the cell's best corner, -1 if it holds none
__global__ __launch_bounds__(kBlock) void corner_cells_kernel(const double* __restrict__ R, int w, int h,
                                                              float margin, int nx, int ny, double cw, double ch,
                                                              double min_eig, int32_t* __restrict__ best) {
  __shared__ unsigned long long wr[kBlock / 64];
  __shared__ int wi[kBlock / 64];
  const int cell = blockIdx.x, cx = cell % nx, cy = cell / nx;
  const int tid = threadIdx.x;
  // a pixel rectangle that contains the cell (the forward formula decides membership below)
  const double m = (double)margin;
  auto lo_of = [&](int c, double cs, int n) {
    return c == 0 ? 0 : (int)fmin(fmax(floor(m + (double)c * cs) - 1.0, 0.0), (double)n);
  };
  auto hi_of = [&](int c, int nc, double cs, int n) {
    return c == nc - 1 ? n - 1 : (int)fmin(fmax(ceil(m + (double)(c + 1) * cs) + 1.0, -1.0), (double)(n - 1));
  };
  const int xa = lo_of(cx, cw, w), xb = hi_of(cx, nx, cw, w);
  const int ya = lo_of(cy, ch, h), yb = hi_of(cy, ny, ch, h);
  const int rw = max(xb - xa + 1, 0), rh = max(yb - ya + 1, 0);
  Key k{0ull, 0x7fffffff};
  for (long q = tid; q < (long)rw * rh; q += kBlock) {
    const int yy = (int)(q / rw), y = ya + yy, x = xa + (int)(q - (long)yy * rw);
    const float xf = (float)x, yf = (float)y;
    if (!inside_margin(xf, yf, w, h, margin)) continue;
    if (cell_of(xf, margin, cw, nx) != cx || cell_of(yf, margin, ch, ny) != cy) continue;
    const double r = R[(long)y * w + x];
    if (!(r >= min_eig)) continue;
    bool corner = true;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dy == 0 && dx == 0) continue;
        const int py = y + dy, px = x + dx;
        if (py < 0 || py >= h || px < 0 || px >= w) continue;
        const double nb = R[(long)py * w + px];
        const bool earlier = dy < 0 || (dy == 0 && dx < 0);  // a neighbour with a smaller index wins a tie
        corner = corner && (earlier ? r > nb : r >= nb);
      }
    if (!corner) continue;
    const unsigned long long rb = (unsigned long long)__double_as_longlong(r);
    const int idx = y * w + x;
    if (beats(rb, idx, k)) k = Key{rb, idx};
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long r2 = __shfl_xor(k.r, off, 64);
    const int i2 = __shfl_xor(k.idx, off, 64);
    if (beats(r2, i2, k)) k = Key{r2, i2};
  }
  if ((tid & 63) == 0) {
    wr[tid >> 6] = k.r;
    wi[tid >> 6] = k.idx;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < kBlock / 64; ++v)
      if (beats(wr[v], wi[v], k)) k = Key{wr[v], wi[v]};
    best[cell] = k.r ? k.idx : -1;
  }
}

// vo_cells_kernel's selection with "empty" replaced by "unoccupied and holds a corner"
constexpr int kSelBlock = 1024, kMaxCells = 65536;
__global__ __launch_bounds__(kSelBlock) void corner_select_kernel(const int32_t* __restrict__ best,
                                                                  const float* __restrict__ uv,
                                                                  const uint8_t* __restrict__ status,
                                                                  const uint8_t* __restrict__ ok, int n, int width,
                                                                  int height, float margin, int nx, int ny, double cw,
                                                                  double ch, int n_feats, int d_min,
                                                                  float* __restrict__ out_uv,
                                                                  int32_t* __restrict__ out_lo,
                                                                  int32_t* __restrict__ out_count) {
  __shared__ uint32_t occ[kMaxCells / 32];
  __shared__ int wsum[kSelBlock / 64];
  __shared__ int ngood;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ncell = nx * ny;
  for (int i = tid; i < (ncell + 31) / 32; i += kSelBlock) occ[i] = 0u;
  if (tid == 0) ngood = 0;
  __syncthreads();
  int cnt = 0;
  for (int k = tid; k < n; k += kSelBlock) {
    const float u = uv[2 * k], v = uv[2 * k + 1];
    if (!(status[k] == 1 && ok[k] != 0 && inside_margin(u, v, width, height, margin))) continue;
    ++cnt;
    const int c = cell_of(v, margin, ch, ny) * nx + cell_of(u, margin, cw, nx);
    atomicOr(&occ[c >> 5], 1u << (c & 31));
  }
  atomicAdd(&ngood, cnt);
  __syncthreads();
  const int want = max(0, n_feats - ngood);
  // candidate cells in ascending order: contiguous chunk per thread, block scan of the counts
  const int chunk = (ncell + kSelBlock - 1) / kSelBlock;
  const int c0 = min(ncell, tid * chunk), c1 = min(ncell, c0 + chunk);
  auto candidate = [&](int c) { return !((occ[c >> 5] >> (c & 31)) & 1u) && best[c] >= 0; };
  int e = 0;
  for (int c = c0; c < c1; ++c) e += candidate(c) ? 1 : 0;
  int x = e;
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < kSelBlock / 64; ++k) {
      const int v = wsum[k];
      wsum[k] = acc;
      acc += v;
    }
    *out_count = min(want, acc);
  }
  __syncthreads();
  int r = wsum[wv] + x - e;
  for (int c = c0; c < c1 && r < want; ++c) {
    if (!candidate(c)) continue;
    const int idx = best[c];
    out_uv[2 * r] = (float)(idx % width);
    out_uv[2 * r + 1] = (float)(idx / width);
    out_lo[r] = d_min;
    ++r;
  }
}

int check_params(me_ctx* c, const char* who, const me_corner_params* p) {
  ME_CHECK(c, p->win >= kMinWin && p->win <= kMaxWin && (p->win & 1), "%s: window must be odd and in [%d, %d]", who,
           kMinWin, kMaxWin);
  ME_CHECK(c, p->min_eig > 0.0, "%s: min_eig must be > 0", who);
  return ME_OK;
}

void launch_response(me_ctx* c, const uint8_t* dimg, int w, int h, int stride, int win, double* dout) {
  const dim3 grid((w + kTX - 1) / kTX, (h + kTY - 1) / kTY);
  hipLaunchKernelGGL(corner_response_kernel, grid, dim3(kBlock), response_lds_bytes((win - 1) / 2), c->stream, dimg,
                     w, h, stride, win, dout);
}

}  // namespace

extern "C" void me_corner_default_params(me_corner_params* p) {
  p->win = 21;
  p->min_eig = 1e-4;
}

extern "C" int me_corner_response(me_ctx* c, me_mem mem, const uint8_t* img, int w, int h, int stride,
                                  const me_corner_params* p, double* response) {
  me_range range_("me_corner_response");
  if (!c || !p) return ME_ERR_INVALID;
  ME_CHECK(c, img && response && w > 0 && h > 0 && stride >= w && (long)w * h < (1L << 31),
           "me_corner_response: bad image");
  ME_TRY(check_params(c, "me_corner_response", p));
  ME_HIP(c, hipSetDevice(c->device));
  const size_t npx = (size_t)w * h;
  const uint8_t* dimg = img;
  double* dout = response;
  if (mem == ME_HOST) {
    void *a, *o;
    const size_t bytes = (size_t)stride * (h - 1) + w;
    ME_TRY(me_scratch(c, SLOT_IMG_L, bytes, &a));
    ME_TRY(me_scratch(c, SLOT_CORNERS, 8 * npx, &o));
    ME_HIP(c, hipMemcpyAsync(a, img, bytes, hipMemcpyHostToDevice, c->stream));
    dimg = (const uint8_t*)a;
    dout = (double*)o;
  }
  {
    me_ktimer t(c, ME_KT_CORNERS);
    launch_response(c, dimg, w, h, stride, p->win, dout);
  }
  ME_TRY(me_check_launch(c, "corner_response_kernel"));
  if (mem == ME_HOST) {
    ME_HIP(c, hipMemcpyAsync(response, dout, 8 * npx, hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipStreamSynchronize(c->stream));
  }
  return ME_OK;
}

extern "C" int me_vo_new_corners(me_ctx* c, const uint8_t* img, int width, int height, int stride, const float* uv,
                                 const uint8_t* status, const uint8_t* ok, int n, float margin, int nx, int ny,
                                 double cw, double ch, int n_feats, int d_min, const me_corner_params* p,
                                 float* out_uv, int32_t* out_lo, int32_t* out_count) {
  me_range range_("me_vo_new_corners");
  if (!c || !p) return ME_ERR_INVALID;
  ME_CHECK(c, img && width > 0 && height > 0 && stride >= width && (long)width * height < (1L << 31),
           "me_vo_new_corners: bad image");
  ME_CHECK(c, n >= 0 && (n == 0 || (uv && status && ok)), "me_vo_new_corners: bad tracked features");
  ME_CHECK(c, nx > 0 && ny > 0 && (long)nx * ny <= kMaxCells && n_feats >= 0 && cw > 0 && ch > 0 && margin >= 0.0f &&
                  std::isfinite(margin),
           "me_vo_new_corners: bad sizes (at most %d cells)", kMaxCells);
  ME_CHECK(c, out_uv && out_lo && out_count, "me_vo_new_corners: null output");
  ME_TRY(check_params(c, "me_vo_new_corners", p));
  ME_HIP(c, hipSetDevice(c->device));
  const size_t npx = (size_t)width * height;
  const int ncell = nx * ny;
  void* base;
  ME_TRY(me_scratch(c, SLOT_CORNERS, 8 * npx + 4 * (size_t)ncell, &base));
  double* map = (double*)base;
  int32_t* best = (int32_t*)(map + npx);
  {
    me_ktimer t(c, ME_KT_CORNERS);
    launch_response(c, img, width, height, stride, p->win, map);
    hipLaunchKernelGGL(corner_cells_kernel, dim3(ncell), dim3(kBlock), 0, c->stream, (const double*)map, width, height,
                       margin, nx, ny, cw, ch, p->min_eig, best);
    hipLaunchKernelGGL(corner_select_kernel, dim3(1), dim3(kSelBlock), 0, c->stream, (const int32_t*)best, uv, status,
                       ok, n, width, height, margin, nx, ny, cw, ch, n_feats, d_min, out_uv, out_lo, out_count);
  }
  return me_check_launch(c, "corner kernels");
}
