// motion_gate.hip — rigid-motion gate of the VO loop's tracked features
// (include/me_hip.h, section A12h; the numpy restatement is
// motion_gate.motion_gate_ref).
//
// Three launches on the ctx stream, none of which needs its grid co-resident:
//  1. gate_prep_kernel    one thread per feature: the usable flag and the two
//                         triangulations P (keyframe t - 1) and Q (keyframe t);
//  2. gate_count_kernel   one workgroup per hypothesis: thread 0 draws the
//                         triple and forms (R, t), the workgroup counts the
//                         inliers with wave ballots (an integer: any order);
//  3. gate_finish_kernel  one workgroup: the first maximum, the Gauss-Newton
//                         steps (ordered sums: one wave per chunk of 64
//                         features, a lane per sum walks the chunk's 64 staged
//                         terms in index order, then the chunk partials in
//                         chunk order), the final inliers, ok_out, err_out, info.
//                         (Staging the terms in device scratch and summing with
//                         a thread per (chunk, sum) over 512 threads was
//                         measured slower: 130 us against 97 us per call at
//                         2000 features)
// FP64 throughout, + - * / sqrt only, every sum in the header's order; the
// library is built with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include "gate_math.hpp"
#include "me_internal.hpp"

namespace {

using namespace me_gate;  // cross3, dot3, reproject, gn_update

constexpr int kBlock = 256;       // threads of every kernel here
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 64;        // feature indices per partial of the ordered sums
constexpr int kSums = 27;         // 21 (upper triangle of J^T J) + 6 (J^T r)
constexpr int kMaxHyp = 1024;
constexpr int kMaxRefine = 8;
constexpr int kInfoBytes = 128;

struct GateArgs {
  const float* prev_uv;
  const float* prev_xr;
  const float* cur_uv;
  const float* cur_xr;
  const uint8_t* status;
  const uint8_t* ok;
  int n;
  double f, cx, cy, fb;    // fb = f * baseline
  float margin, wlim, hlim;  // wlim = (float)width - margin, hlim likewise
  double min_disp, g2;     // g2 = gate_max * gate_max
  uint32_t t, seed;
  int n_hyp, refine, min_inliers;
  // scratch
  uint8_t* flag;  // bit 0: usable, bit 1 (finish kernel): inlier of the final pose
  double* P;      // 3 per feature
  double* Q;
  double* hyp;    // 12 per hypothesis: R row-major, t
  int* cnt;       // per hypothesis: inliers, -1 void
  double* part;   // kSums per chunk
  // outputs
  uint8_t* ok_out;
  float* err_out;
  unsigned char* info;
};

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// Orthonormal frame of the triangle with edges a, b: false when it is degenerate
__device__ __forceinline__ bool frame3(const double* a, const double* b, double* e1, double* e2, double* e3) {
  const double aa = dot3(a, a), bb = dot3(b, b);
  double c[3];
  cross3(a, b, c);
  const double cc = dot3(c, c);
  if (!(cc > (1e-6 * aa) * bb)) return false;
  const double la = sqrt(aa), lc = sqrt(cc);
  for (int k = 0; k < 3; ++k) {
    e1[k] = a[k] / la;
    e3[k] = c[k] / lc;
  }
  cross3(e3, e1, e2);
  return true;
}

__global__ __launch_bounds__(kBlock) void gate_prep_kernel(GateArgs g) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= g.n) return;
  const float u0 = g.prev_uv[2 * (size_t)k], v0 = g.prev_uv[2 * (size_t)k + 1], x0 = g.prev_xr[k];
  const float u1 = g.cur_uv[2 * (size_t)k], v1 = g.cur_uv[2 * (size_t)k + 1], x1 = g.cur_xr[k];
  const bool good = g.status[k] == 1 && g.ok[k] != 0 && u1 >= g.margin && u1 < g.wlim && v1 >= g.margin && v1 < g.hlim;
  const double d0 = (double)u0 - (double)x0, d1 = (double)u1 - (double)x1;
  const bool usable = good && d0 >= g.min_disp && d1 >= g.min_disp;
  g.flag[k] = usable ? 1 : 0;
  if (!usable) return;
  const double Z0 = g.fb / d0, Z1 = g.fb / d1;
  double* P = g.P + 3 * (size_t)k;
  double* Q = g.Q + 3 * (size_t)k;
  P[0] = ((double)u0 - g.cx) * Z0 / g.f;
  P[1] = ((double)v0 - g.cy) * Z0 / g.f;
  P[2] = Z0;
  Q[0] = ((double)u1 - g.cx) * Z1 / g.f;
  Q[1] = ((double)v1 - g.cy) * Z1 / g.f;
  Q[2] = Z1;
}

// Hypothesis h: the triple, then (R, t) into out[12]; false when a slot finds no feature or a triangle is degenerate
__device__ bool hypothesis(const GateArgs& g, uint32_t h, double* out) {
  const uint32_t base = g.t * 0x9E3779B1u + h * 0x85EBCA77u + g.seed;
  uint32_t idx[3] = {0, 0, 0};
  for (int s = 0; s < 3; ++s) {
    bool got = false;
    for (int a = 0; a < 8 && !got; ++a) {
      const uint32_t key = base + (uint32_t)(s * 8 + a) * 0xC2B2AE3Du;
      const uint32_t i = (uint32_t)(((uint64_t)lowbias32(key) * (uint64_t)(uint32_t)g.n) >> 32);  // < n
      bool take = (g.flag[i] & 1) != 0;
      for (int s0 = 0; s0 < s; ++s0) take = take && i != idx[s0];
      if (take) {
        idx[s] = i;
        got = true;
      }
    }
    if (!got) return false;
  }
  const double *P0 = g.P + 3 * (size_t)idx[0], *P1 = g.P + 3 * (size_t)idx[1], *P2 = g.P + 3 * (size_t)idx[2];
  const double *Q0 = g.Q + 3 * (size_t)idx[0], *Q1 = g.Q + 3 * (size_t)idx[1], *Q2 = g.Q + 3 * (size_t)idx[2];
  double a[3], b[3], e[3][3], f[3][3];
  for (int k = 0; k < 3; ++k) {
    a[k] = P1[k] - P0[k];
    b[k] = P2[k] - P0[k];
  }
  const bool ve = frame3(a, b, e[0], e[1], e[2]);
  for (int k = 0; k < 3; ++k) {
    a[k] = Q1[k] - Q0[k];
    b[k] = Q2[k] - Q0[k];
  }
  const bool vf = frame3(a, b, f[0], f[1], f[2]);
  if (!(ve && vf)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (f[0][i] * e[0][j] + f[1][i] * e[1][j]) + f[2][i] * e[2][j];
  for (int i = 0; i < 3; ++i)
    out[9 + i] = Q0[i] - ((out[3 * i] * P0[0] + out[3 * i + 1] * P0[1]) + out[3 * i + 2] * P0[2]);
  return true;
}

__global__ __launch_bounds__(kBlock) void gate_count_kernel(GateArgs g) {
  __shared__ double sh[12];
  __shared__ int s_valid;
  __shared__ int s_wave[kWaves];
  const int h = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    double o[12];
    const bool v = hypothesis(g, (uint32_t)h, o);
    s_valid = v ? 1 : 0;
    if (v) {
      for (int i = 0; i < 12; ++i) {
        sh[i] = o[i];
        g.hyp[12 * (size_t)h + i] = o[i];
      }
    } else {
      g.cnt[h] = -1;
    }
  }
  __syncthreads();
  if (!s_valid) return;  // (uniform)
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = sh[i];
  for (int i = 0; i < 3; ++i) t[i] = sh[9 + i];
  int mine = 0;
  const int rounds = (g.n + kBlock - 1) / kBlock;
  for (int j = 0; j < rounds; ++j) {  // (uniform trip count: the ballot sees whole waves)
    const int k = j * kBlock + tid;
    bool inl = false;
    if (k < g.n && (g.flag[k] & 1)) {
      double Y[3], r[3], e2;
      reproject(R, t, g.P + 3 * (size_t)k, (double)g.cur_uv[2 * (size_t)k], (double)g.cur_uv[2 * (size_t)k + 1],
                (double)g.cur_xr[k], g, Y, r, e2);
      inl = Y[2] > 0.0 && e2 <= g.g2;
    }
    mine += __popcll(__ballot(inl));  // every lane holds its wave's count
  }
  if ((tid & 63) == 0) s_wave[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += s_wave[w];
    g.cnt[h] = c;
  }
}

__global__ __launch_bounds__(kBlock) void gate_finish_kernel(GateArgs g) {
  __shared__ double s_stage[kWaves][kSums][kChunk + 1];  // (+1: a lane per sum reads its row without bank conflicts)
  __shared__ double s_tot[kSums];
  __shared__ double s_pose[12];
  __shared__ unsigned long long s_key;
  __shared__ int s_nvalid, s_nusable, s_ninl, s_stop;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int n = g.n;
  if (tid == 0) {
    s_key = 0;
    s_nvalid = 0;
    s_nusable = 0;
    s_ninl = 0;
    s_stop = 0;
  }
  __syncthreads();
  // the first maximum of the counts: the largest (count + 1, kMaxHyp - 1 - h)
  {
    unsigned long long best = 0;
    int nv = 0;
    for (int h = tid; h < g.n_hyp; h += kBlock) {
      const int c = g.cnt[h];
      if (c < 0) continue;
      ++nv;
      const unsigned long long key = ((unsigned long long)(c + 1) << 10) | (unsigned)(kMaxHyp - 1 - h);
      best = key > best ? key : best;
    }
    if (nv) {
      atomicMax(&s_key, best);
      atomicAdd(&s_nvalid, nv);
    }
    int nu = 0;
    for (int k = tid; k < n; k += kBlock) nu += g.flag[k] & 1;
    if (nu) atomicAdd(&s_nusable, nu);
  }
  __syncthreads();
  const int winner = s_nvalid > 0 ? kMaxHyp - 1 - (int)(s_key & (kMaxHyp - 1)) : -1;
  if (winner >= 0) {
    if (tid < 12) s_pose[tid] = g.hyp[12 * (size_t)winner + tid];
    __syncthreads();
    const int nchunks = (n + kChunk - 1) / kChunk;
    for (int it = 0; it < g.refine; ++it) {
      double R[9], t[3];
      for (int i = 0; i < 9; ++i) R[i] = s_pose[i];
      for (int i = 0; i < 3; ++i) t[i] = s_pose[9 + i];
      for (int c0 = 0; c0 < nchunks; c0 += kWaves) {  // (uniform trip count: barriers inside)
        const int chunk = c0 + wv;
        const int k = chunk * kChunk + lane;
        double term[kSums];
        for (int s = 0; s < kSums; ++s) term[s] = 0.0;
        if (chunk < nchunks && k < n && (g.flag[k] & 1)) {
          double Y[3], r[3], e2;
          reproject(R, t, g.P + 3 * (size_t)k, (double)g.cur_uv[2 * (size_t)k], (double)g.cur_uv[2 * (size_t)k + 1],
                    (double)g.cur_xr[k], g, Y, r, e2);
          if (Y[2] > 0.0 && e2 <= g.g2) {
            const double a = g.f / Y[2], q = Y[2] * Y[2];
            double J[3][6];
            const double gr[3][3] = {{a, 0.0, -(g.f * Y[0]) / q}, {0.0, a, -(g.f * Y[1]) / q}, {a, 0.0, (g.fb - g.f * Y[0]) / q}};
            for (int m = 0; m < 3; ++m) {
              cross3(Y, gr[m], J[m]);
              for (int i = 0; i < 3; ++i) J[m][3 + i] = gr[m][i];
            }
            int s = 0;
            for (int i = 0; i < 6; ++i)
              for (int j = i; j < 6; ++j) term[s++] = (J[0][i] * J[0][j] + J[1][i] * J[1][j]) + J[2][i] * J[2][j];
            for (int i = 0; i < 6; ++i) term[s++] = (J[0][i] * r[0] + J[1][i] * r[1]) + J[2][i] * r[2];
          }
        }
        for (int s = 0; s < kSums; ++s) s_stage[wv][s][lane] = term[s];
        __syncthreads();
        if (chunk < nchunks && lane < kSums) {
          double acc = 0.0;
          for (int j0 = 0; j0 < kChunk; j0 += 16) {  // (16 reads in flight, then their adds in index order)
            double v[16];
            for (int j = 0; j < 16; ++j) v[j] = s_stage[wv][lane][j0 + j];
            for (int j = 0; j < 16; ++j) acc = acc + v[j];
          }
          g.part[(size_t)chunk * kSums + lane] = acc;
        }
        __syncthreads();
      }
      if (tid < kSums) {
        double tot = 0.0;
        int c = 0;
        for (; c + 8 <= nchunks; c += 8) {  // (8 loads in flight, then their adds in chunk order)
          double v[8];
          for (int j = 0; j < 8; ++j) v[j] = g.part[(size_t)(c + j) * kSums + tid];
          for (int j = 0; j < 8; ++j) tot = tot + v[j];
        }
        for (; c < nchunks; ++c) tot = tot + g.part[(size_t)c * kSums + tid];
        s_tot[tid] = tot;
      }
      __syncthreads();
      if (tid == 0) {
        if (!gn_update(s_tot, s_pose)) s_stop = 1;  // (H d = -b, the Cayley update: gate_math.hpp)
      }
      __syncthreads();
      if (s_stop) break;  // (uniform)
    }
    // the final pose's inliers and errors
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = s_pose[i];
    for (int i = 0; i < 3; ++i) t[i] = s_pose[9 + i];
    int mine = 0;
    for (int k = tid; k < n; k += kBlock) {
      const uint8_t fl = g.flag[k] & 1;
      float err = INFINITY;
      bool inl = false;
      if (fl) {
        double Y[3], r[3], e2;
        reproject(R, t, g.P + 3 * (size_t)k, (double)g.cur_uv[2 * (size_t)k], (double)g.cur_uv[2 * (size_t)k + 1],
                  (double)g.cur_xr[k], g, Y, r, e2);
        if (Y[2] > 0.0) {
          err = (float)sqrt(e2);
          inl = e2 <= g.g2;
        }
      }
      if (inl) {
        g.flag[k] = 3;
        ++mine;
      }
      if (g.err_out) g.err_out[k] = err;
    }
    if (mine) atomicAdd(&s_ninl, mine);
  } else if (g.err_out) {
    for (int k = tid; k < n; k += kBlock) g.err_out[k] = INFINITY;
  }
  __syncthreads();  // (this thread's own flag bytes are read back below: same thread, same index)
  const bool abstain = winner < 0 || s_ninl < g.min_inliers;
  for (int k = tid; k < n; k += kBlock) {
    const uint8_t o = g.ok[k];
    g.ok_out[k] = (!abstain && g.flag[k] == 1) ? (uint8_t)0 : o;
  }
  if (tid == 0) {
    int32_t* iw = (int32_t*)g.info;
    iw[0] = s_nusable;
    iw[1] = s_nvalid;
    iw[2] = winner;
    iw[3] = s_ninl;
    iw[4] = abstain ? 1 : 0;
    iw[5] = iw[6] = iw[7] = 0;
    double* dw = (double*)(g.info + 32);
    for (int i = 0; i < 12; ++i) dw[i] = winner >= 0 ? s_pose[i] : 0.0;
  }
}

}  // namespace

extern "C" void me_motion_gate_default_params(me_motion_gate_params* p) {
  if (!p) return;
  p->gate_max = 2.0;
  p->min_disp = 0.5;
  p->n_hyp = 256;
  p->refine = 3;
  p->min_inliers = 10;
  p->seed = 0;
}

// The parameter checks the entry point and me_vo_loop_set_motion_gate share: NULL on success, else the
// message, which names the argument.
const char* me_motion_gate_check(const me_motion_gate_params* p) {
  if (!p) return "null params";
  if (!(std::isfinite(p->gate_max) && p->gate_max > 0.0)) return "gate_max must be finite and > 0";
  if (!(std::isfinite(p->min_disp) && p->min_disp > 0.0)) return "min_disp must be finite and > 0";
  if (p->n_hyp < 1 || p->n_hyp > kMaxHyp) return "n_hyp must be in 1 .. 1024";
  if (p->refine < 0 || p->refine > kMaxRefine) return "refine must be in 0 .. 8";
  if (p->min_inliers < 3) return "min_inliers must be >= 3";
  return nullptr;
}

extern "C" int me_motion_gate(me_ctx* c, const float* prev_uv, const float* prev_xr, const float* cur_uv,
                              const float* cur_xr, const uint8_t* status, const uint8_t* ok_in, int n, double f,
                              double cx, double cy, double baseline, int width, int height, float margin, int t,
                              const me_motion_gate_params* p, uint8_t* ok_out, float* err_out, void* info) {
  me_range range_("me_motion_gate");
  if (!c) return ME_ERR_INVALID;
  if (const char* why = me_motion_gate_check(p)) return me_set_error(c, ME_ERR_INVALID, "me_motion_gate: %s", why);
  ME_CHECK(c, n >= 0 && n <= (1 << 24), "me_motion_gate: n must be in 0 .. 2^24");
  ME_CHECK(c, n == 0 || (prev_uv && prev_xr && cur_uv && cur_xr && status && ok_in && ok_out),
           "me_motion_gate: null feature array");
  ME_CHECK(c, std::isfinite(f) && f > 0.0, "me_motion_gate: f must be finite and > 0");
  ME_CHECK(c, std::isfinite(baseline) && baseline > 0.0, "me_motion_gate: baseline must be finite and > 0");
  ME_CHECK(c, std::isfinite(cx) && std::isfinite(cy), "me_motion_gate: cx and cy must be finite");
  ME_CHECK(c, width >= 1 && height >= 1, "me_motion_gate: width / height must be >= 1");
  ME_CHECK(c, std::isfinite(margin) && margin >= 0.0f, "me_motion_gate: margin must be finite and >= 0");
  ME_CHECK(c, t >= 0, "me_motion_gate: t must be >= 0");
  ME_CHECK(c, ((uintptr_t)info & 7) == 0, "me_motion_gate: info must be 8-byte aligned");
  ME_HIP(c, hipSetDevice(c->device));
  // one slot: info (when the caller gives none) | P | Q | hyp | part | cnt | flag
  const size_t m = (size_t)n, nchunks = (m + kChunk - 1) / kChunk;
  const size_t o_p = kInfoBytes, o_q = o_p + 24 * m, o_hyp = o_q + 24 * m, o_part = o_hyp + 96 * (size_t)p->n_hyp;
  const size_t o_cnt = o_part + 8 * kSums * nchunks, o_flag = o_cnt + 4 * (size_t)p->n_hyp;
  void* base;
  ME_TRY(me_scratch(c, SLOT_GATE, o_flag + m + 8, &base));
  unsigned char* b = (unsigned char*)base;
  GateArgs g{};
  g.prev_uv = prev_uv;
  g.prev_xr = prev_xr;
  g.cur_uv = cur_uv;
  g.cur_xr = cur_xr;
  g.status = status;
  g.ok = ok_in;
  g.n = n;
  g.f = f;
  g.cx = cx;
  g.cy = cy;
  g.fb = f * baseline;
  g.margin = margin;
  g.wlim = (float)width - margin;
  g.hlim = (float)height - margin;
  g.min_disp = p->min_disp;
  g.g2 = p->gate_max * p->gate_max;
  g.t = (uint32_t)t;
  g.seed = p->seed;
  g.n_hyp = n > 0 ? p->n_hyp : 0;  // (no feature: no hypothesis is drawn, the finish kernel writes the info block)
  g.refine = p->refine;
  g.min_inliers = p->min_inliers;
  g.P = (double*)(b + o_p);
  g.Q = (double*)(b + o_q);
  g.hyp = (double*)(b + o_hyp);
  g.part = (double*)(b + o_part);
  g.cnt = (int*)(b + o_cnt);
  g.flag = b + o_flag;
  g.ok_out = ok_out;
  g.err_out = err_out;
  g.info = info ? (unsigned char*)info : b;
  if (n > 0) {
    {
      me_ktimer tm(c, ME_KT_GATE);
      hipLaunchKernelGGL(gate_prep_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, g);
    }
    ME_TRY(me_check_launch(c, "gate_prep_kernel"));
    {
      me_ktimer tm(c, ME_KT_GATE);
      hipLaunchKernelGGL(gate_count_kernel, dim3(p->n_hyp), dim3(kBlock), 0, c->stream, g);
    }
    ME_TRY(me_check_launch(c, "gate_count_kernel"));
  }
  {
    me_ktimer tm(c, ME_KT_GATE);
    hipLaunchKernelGGL(gate_finish_kernel, dim3(1), dim3(kBlock), 0, c->stream, g);
  }
  return me_check_launch(c, "gate_finish_kernel");
}
