// ba_plan.hpp — part of ba.hip: the observation layout built on the device
// from the raw inputs, and the solve's read-back.  Kernels: plan_count_kernel,
// plan_scan_kernel, plan_scatter_kernel, plan_segsort_kernel, plan_band_kernel,
// plan_order_kernel, output_kernel.  Every other part reads what they write.
#pragma once
#include "ba_types.hpp"
#include "ba_residual.hpp"

using namespace ba;

namespace {

// The observation layout is built on the device from the raw inputs, so a
// problem already resident in HBM (me_ba_problem.mem == ME_DEVICE) never
// crosses PCIe and no host sort sits on the frame's critical path.
//   plan_count   per obs: point histogram (atomics), per-(block, camera)
//                counts (LDS), index validation; per point: box feasibility;
//                copies the starting parameters into the solver buffers.
//   plan_scan    one workgroup: CSR offsets by point, per-camera block offsets,
//                State initialisation.
//   plan_scatter per obs: point slot (atomic), camera slot = block offset +
//                stable rank inside the block (original order kept).
//   plan_segsort per point: its slots sorted by (camera, obs index), exactly
//                the host stable_sort by camera; pos / p_cam / dup.
enum { F_BAD = 0, F_INFEASIBLE = 1 };
struct PlanWork {
  int* cnt_p;
  int* fill_p;
  int* blk_cam;
  int* flags;
};
__device__ __forceinline__ PlanWork plan_work(const Geo& g, int* w) {
  PlanWork pw;
  pw.cnt_p = w;
  pw.fill_p = w + g.np;
  pw.blk_cam = w + 2 * (long)g.np;
  pw.flags = pw.blk_cam + (long)g.nblk_obs * g.nc;
  return pw;
}

__global__ __launch_bounds__(kBlock) void plan_count_kernel(Geo g, Bufs b, const double* cams_in,
                                                            const double* pts_in) {
  extern __shared__ int lcnt[];  // nc
  const PlanWork w = plan_work(g, b.work);
  const int t = threadIdx.x, blk = blockIdx.x;
  const long gid = (long)blk * kBlock + t;
  // the launch's last workgroup: the starting cameras' rotation table, beside
  // the counting workgroups (its sin / cos chain on none of their paths)
  if (blk == (int)gridDim.x - 1) {
    for (int c = t; c < g.nc; c += kBlock) rot_entry(cams_in + 6 * c + 3, b.rot[0] + kRotStride * c);
    return;
  }
  for (int c = t; c < g.nc; c += kBlock) lcnt[c] = 0;
  __syncthreads();
  if (blk < g.nblk_obs && gid < g.no) {
    const int ci = b.cam_idx[gid], pi = b.pt_idx[gid];
    if (ci < 0 || ci >= g.nc || pi < 0 || pi >= g.np) {
      atomicOr(&w.flags[F_BAD], 1);
    } else {
      atomicAdd(&w.cnt_p[pi], 1);
      atomicAdd(&lcnt[ci], 1);
    }
  }
  if (gid < g.np) {
    for (int a = 0; a < 3; ++a) {
      const double x = pts_in[3 * gid + a];
      if (!(x >= g.lo[a] && x <= g.hi[a])) atomicOr(&w.flags[F_INFEASIBLE], 1);
    }
  }
  if (cams_in != b.cams[0] && gid < 6 * (long)g.nc) b.cams[0][gid] = cams_in[gid];
  if (pts_in != b.pts[0] && gid < 3 * (long)g.np) b.pts[0][gid] = pts_in[gid];
  __syncthreads();
  if (blk < g.nblk_obs)
    for (int c = t; c < g.nc; c += kBlock) w.blk_cam[(long)blk * g.nc + c] = lcnt[c];
}

constexpr int kScanBlock = 1024;
constexpr int kMaxScanCams = 4096;
__global__ __launch_bounds__(kScanBlock) void plan_scan_kernel(Geo g, Bufs b, Opts o) {
  __shared__ int wsum[kScanBlock / 64];
  __shared__ int total;
  const PlanWork w = plan_work(g, b.work);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // exclusive scan of the point counts: contiguous chunk per thread
  const int chunk = (g.np + kScanBlock - 1) / kScanBlock;
  const int beg = min(g.np, t * chunk), end = min(g.np, beg + chunk);
  int s = 0;
  for (int j = beg; j < end; ++j) s += w.cnt_p[j];
  int x = s;  // inclusive wave scan
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < kScanBlock / 64; ++k) {
      const int v = wsum[k];
      wsum[k] = acc;
      acc += v;
    }
    total = acc;
  }
  __syncthreads();
  int run = wsum[wv] + x - s;
  for (int j = beg; j < end; ++j) {
    b.p_off[j] = run;
    run += w.cnt_p[j];
  }
  if (t == 0) b.p_off[g.np] = total;
  // per-camera offsets of every observation block (variable cameras only):
  // one wave per camera scans its column of block counts, then the camera
  // totals are scanned and added
  __shared__ int ctot[kMaxScanCams];
  const int bchunk = (g.nblk_obs + 63) / 64;
  for (int c = wv; c < g.m; c += kScanBlock / 64) {
    const int k0 = min(g.nblk_obs, lane * bchunk), k1 = min(g.nblk_obs, k0 + bchunk);
    int cs = 0;
    for (int k = k0; k < k1; ++k) cs += w.blk_cam[(long)k * g.nc + g.nf + c];
    int cx = cs;
    for (int off = 1; off < 64; off <<= 1) {
      const int y = __shfl_up(cx, off, 64);
      if (lane >= off) cx += y;
    }
    int r = cx - cs;
    for (int k = k0; k < k1; ++k) {
      int* e = &w.blk_cam[(long)k * g.nc + g.nf + c];
      const int v = *e;
      *e = r;
      r += v;
    }
    if (lane == 63) ctot[c] = cx;
  }
  __syncthreads();
  __shared__ int ufst[kMaxScanCams + 1];  // first camera-assembly unit of every camera | the unit total
  __shared__ int ctotal;                  // c_off[m]
  if (t == 0) {
    int acc = 0, units = 0;
    for (int c = 0; c < g.m; ++c) {
      b.c_off[c] = acc;
      const int v = ctot[c];
      ctot[c] = acc;
      acc += v;
      ufst[c] = units;
      units += max(1, (v + kBlock - 1) / kBlock);
    }
    b.c_off[g.m] = acc;
    ctotal = acc;
    ufst[g.m] = units;  // (at most g.ncu = ceil(no / 256) + m: every camera rounds up by less than one unit)
  }
  __syncthreads();
  for (int c = wv; c < g.m; c += kScanBlock / 64) {
    const int k0 = min(g.nblk_obs, lane * bchunk), k1 = min(g.nblk_obs, k0 + bchunk);
    for (int k = k0; k < k1; ++k) w.blk_cam[(long)k * g.nc + g.nf + c] += ctot[c];
    // the camera's units (ba_types.hpp CU_*): 256 slots each, the last one the remainder
    const int cbeg = ctot[c], cend = c + 1 < g.m ? ctot[c + 1] : ctotal;
    const int first = ufst[c], count = ufst[c + 1] - first;
    for (int k = lane; k < count; k += 64) {
      int* e = b.cunit + (long)kCuStride * (first + k);
      e[CU_CAM] = c;
      e[CU_BEG] = cbeg + k * kBlock;
      e[CU_END] = min(cend, cbeg + (k + 1) * kBlock);
      e[CU_COUNT] = count;
      e[CU_FIRST] = first;
    }
  }
  // units the host launches beyond the total: no camera
  for (int u = ufst[g.m] + t; u < (g.ncu + 7) / 8 * 8; u += kScanBlock) b.cunit[(long)kCuStride * u + CU_CAM] = -1;
  for (int i = t; i < g.n6; i += kScanBlock) b.csc[i] = 0.0;
  if (t == 0) {
    State* st = b.st;
    st->cur = 0;
    st->need_lin = 1;
    st->done = 0;
    st->termination = 1;
    st->iterations = st->successful = st->invalid_count = 0;
    st->fail = st->scaled = st->accepted = st->final_pass = st->spin_err = 0;
    st->bad_input = w.flags[F_BAD];
    st->infeasible = w.flags[F_INFEASIBLE];
    st->radius = o.initial_radius;
    st->decrease = 2.0;
    st->x_cost = st->cand_cost = st->model_change = st->initial_cost = 0.0;
    st->cam_step2 = st->cam_xn2 = st->cam_model = st->last_q = 0.0;
    for (int k = 0; k < 16; ++k) st->stamps[k] = 0;
    st->stamps[14] = ufst[g.m];  // the camera-assembly unit total (me_debug_read; no timing build uses the word)
    if (st->bad_input || st->infeasible) {
      st->done = 1;
      st->termination = 2;
    }
  }
}

__global__ __launch_bounds__(kBlock) void plan_scatter_kernel(Geo g, Bufs b) {
  __shared__ int scam[kBlock];
  const PlanWork w = plan_work(g, b.work);
  if (w.flags[F_BAD]) return;
  const int t = threadIdx.x, blk = blockIdx.x;
  const int o = blk * kBlock + t;
  const int ci = o < g.no ? b.cam_idx[o] : -1;
  scam[t] = ci;
  if (o < g.no) {
    const int pi = b.pt_idx[o];
    b.tmp_obs[b.p_off[pi] + atomicAdd(&w.fill_p[pi], 1)] = o;
  }
  __syncthreads();
  if (o < g.no) {
    int slot = -1;
    if (ci >= g.nf) {
      int rank = 0;
      for (int k = 0; k < t; ++k) rank += scam[k] == ci;
      slot = w.blk_cam[(long)blk * g.nc + ci] + rank;
      b.c_obs[slot] = o;
    }
    b.cpos[o] = slot;
  }
}

// One wave per point: rank of each slot by (camera, observation index) --
// the order of the host stable_sort by camera -- then p_obs / pos / p_cam /
// dup.  Segments of <= 64 observations rank with shuffles; longer ones with a
// loop over the (cached) segment.
constexpr int kSortBlock = 256;
__global__ __launch_bounds__(kSortBlock) void plan_segsort_kernel(Geo g, Bufs b) {
  const PlanWork w = plan_work(g, b.work);
  if (w.flags[F_BAD]) return;
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (kSortBlock / 64) + (threadIdx.x >> 6);
  if (j >= g.np) return;
  const int beg = b.p_off[j], k = b.p_off[j + 1] - beg;
  auto key_of = [&](int o) { return ((unsigned long long)(unsigned)b.cam_idx[o] << 32) | (unsigned)o; };
  if (k <= 64) {
    const int o = lane < k ? b.tmp_obs[beg + lane] : 0;
    const unsigned long long key = lane < k ? key_of(o) : ~0ull;
    int rank = 0, same = 0;
    for (int l = 0; l < k; ++l) {
      const unsigned long long kl = __shfl(key, l, 64);
      rank += kl < key;
      same += (kl >> 32) == (key >> 32);
    }
    if (lane < k) {
      const int q = beg + rank;
      b.p_obs[q] = o;
      b.pos[o] = q;
      b.p_cam[q] = (int)(key >> 32) - g.nf;
      b.dup[o] = same > 1 ? 1 : 0;
    }
    return;
  }
  for (int e = lane; e < k; e += 64) {
    const int o = b.tmp_obs[beg + e];
    const unsigned long long key = key_of(o);
    int rank = 0, same = 0;
    for (int l = 0; l < k; ++l) {
      const unsigned long long kl = key_of(b.tmp_obs[beg + l]);
      rank += kl < key;
      same += (kl >> 32) == (key >> 32);
    }
    const int q = beg + rank;
    b.p_obs[q] = o;
    b.pos[o] = q;
    b.p_cam[q] = (int)(key >> 32) - g.nf;
    b.dup[o] = same > 1 ? 1 : 0;
  }
}

// Band order of the landmarks for the Schur runs (pt_schur_kernel): key =
// first tile * T + last tile of the landmark's variable-camera columns
// (slots are sorted by camera: the first variable slot and the last slot), a
// landmark without variable cameras in the last bucket.  Stable counting
// sort: per 256-landmark block, the rank of each key among the block's
// earlier landmarks (within a wave by ballots over its distinct keys, plus the
// counts of the earlier waves) and the block's key counts (bucket-major),
// then plan_order_kernel scans the counts and scatters.  Only for windows
// with many tile pairs (g.sorted); otherwise the runs keep the landmark order
// and every run takes the whole tile set.
constexpr int kMaxBandKeys = 19 * 19;  // T <= 19 (npairs <= 192)
__global__ __launch_bounds__(kBlock) void plan_band_kernel(Geo g, Bufs b) {
  __shared__ int wcnt[kBlock / 64][kMaxBandKeys];
  const PlanWork w = plan_work(g, b.work);
  const int t = threadIdx.x, blk = blockIdx.x, j = blk * kBlock + t, lane = t & 63, wv = t >> 6;
  const int K = g.T * g.T;
  for (int k = t; k < (kBlock / 64) * K; k += kBlock) wcnt[k / K][k % K] = 0;
  int key = -1;
  if (j < g.np) {
    key = K - 1;
    const int beg = b.p_off[j], end = b.p_off[j + 1];
    const int hi = (!w.flags[F_BAD] && end > beg) ? b.p_cam[end - 1] : -1;
    if (hi >= 0) {
      int q = beg;
      while (b.p_cam[q] < 0) ++q;  // fixed cameras (negative) sort first
      key = (6 * b.p_cam[q] / 16) * g.T + (6 * hi + 5) / 16;
    }
  }
  __syncthreads();
  // rank among the wave's lower lanes with the same key: one ballot per distinct key
  int rank = 0;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {
    const int lead = __builtin_ctzll(todo);
    const int kl = __shfl(key, lead, 64);
    const unsigned long long m = __ballot(key == kl);
    if (key == kl) rank = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == lead) wcnt[wv][kl] = __builtin_popcountll(m);
    todo &= ~m;
  }
  __syncthreads();
  if (j < g.np) {
    for (int v = 0; v < wv; ++v) rank += wcnt[v][key];
    b.pkey[j] = key;
    b.prank[j] = rank;
  }
  for (int k = t; k < K; k += kBlock) {
    int c = 0;
#pragma unroll
    for (int v = 0; v < kBlock / 64; ++v) c += wcnt[v][k];
    b.phist[(long)k * g.nblkp + blk] = c;
  }
}

// One workgroup: exclusive scan of the block key counts -> band order, and
// with the scatter each run's band (first tile of its first landmark, largest
// last tile: LDS max); then per tile pair the partial slots of the runs whose
// tile set holds it, in run order.
constexpr int kMaxRuns = 1024;
__global__ __launch_bounds__(kScanBlock) void plan_order_kernel(Geo g, Bufs b) {
  __shared__ int wsum[kScanBlock / 64];
  __shared__ int rA[kMaxRuns], rB[kMaxRuns];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int r = t; r < g.nruns; r += kScanBlock) {
    rA[r] = g.T - 1;  // (a run past the last landmark: the z tile alone)
    rB[r] = 0;
  }
  const long nh = (long)g.T * g.T * g.nblkp;
  const long chunk = (nh + kScanBlock - 1) / kScanBlock;
  const long beg = min(nh, t * chunk), end = min(nh, beg + chunk);
  int s = 0;
  for (long i = beg; i < end; ++i) s += b.phist[i];
  int x = s;  // inclusive wave scan
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  if (t == 0) {
    int acc = 0;
    for (int k = 0; k < kScanBlock / 64; ++k) {
      const int v = wsum[k];
      wsum[k] = acc;
      acc += v;
    }
  }
  __syncthreads();
  int run = wsum[wv] + x - s;
  for (long i = beg; i < end; ++i) {
    const int v = b.phist[i];
    b.phist[i] = run;
    run += v;
  }
  __syncthreads();
  for (int j = t; j < g.np; j += kScanBlock) {
    const int key = b.pkey[j];
    const int pos = b.phist[(long)key * g.nblkp + j / kBlock] + b.prank[j];
    b.order[pos] = j;
    const int r = pos / g.rlen;
    if (pos == r * g.rlen) rA[r] = key / g.T;  // keys ascend: the run's first landmark has its smallest first tile
    atomicMax(&rB[r], key % g.T);
  }
  __syncthreads();
  for (int r = t; r < g.nruns; r += kScanBlock) {
    const int B = max(rA[r], rB[r]);
    rB[r] = B;
    b.rband[2 * r] = rA[r];
    b.rband[2 * r + 1] = B;
  }
  __syncthreads();
  for (int p = t; p < g.npairs; p += kScanBlock) {
    int I = 0, rem = p;
    while (rem >= g.T - I) {
      rem -= g.T - I;
      ++I;
    }
    const int J = I + rem;
    int cnt = 0;
    for (int r = 0; r < g.nruns; ++r) {
      const int A = rA[r], B = rB[r];
      const int nb = B - A + 1, ns = nb + (B < g.T - 1 ? 1 : 0);
      const int ka = (I >= A && I <= B) ? I - A : (I == g.T - 1 ? nb : -1);
      const int kb = (J >= A && J <= B) ? J - A : (J == g.T - 1 ? nb : -1);
      if (ka < 0 || kb < 0) continue;
      b.tl[(long)p * g.nruns + cnt++] = r * g.npairs + ka * ns - ka * (ka - 1) / 2 + (kb - ka);
    }
    b.tcnt[p] = cnt;
    for (int q = cnt; q < g.nruns; ++q) b.tl[(long)p * g.nruns + q] = -1;  // (the assembly reads whole lists)
  }
}

// State | cams[cur] | pts[cur] -> one contiguous read-back (or straight into
// the caller's device arrays for a device-resident problem)
__global__ __launch_bounds__(kBlock) void output_kernel(Geo g, Bufs b, double* cams_dst, double* pts_dst) {
  const int cur = b.st->cur;
  const long gid = (long)blockIdx.x * kBlock + threadIdx.x;
  constexpr int kStateWords = (int)(sizeof(State) / 8);
  if (gid < kStateWords) b.out[gid] = ((const double*)b.st)[gid];
  if (gid < 6 * (long)g.nc) cams_dst[gid] = b.cams[cur][gid];
  if (gid < 3 * (long)g.np) pts_dst[gid] = b.pts[cur][gid];
}

}  // namespace
