// ba_vo_chain.hpp — part of ba.hip: the VO loop's device-side glue around a
// window's solve.  Kernels: vo_chain_kernel (window t's start from window
// t-1's result), window_indices_kernel.  Reads the State, cameras and points a
// solve leaves (output_kernel's sources).
#pragma once
#include "me_internal.hpp"
#include "ba_types.hpp"

using namespace ba;

// The windowed VO loop (pipeline.py, WindowedStereoVO.process step 7) forms
// window t's BA start from window t-1's BA result: the poses and landmarks it
// solved (when it succeeded, BundleAdjuster status 2), pose(t) predicted again
// from the refined poses, and the landmarks new in t moved with it (their
// camera-frame coordinates kept).  On the device the same arithmetic, in the
// same order (fp-contract off; the rotation of the new pose by a fixed Taylor
// series in theta^2: no libm), runs behind window t-1's solve, so window t is
// queued before t-1 completes; the host repeats it on the downloaded result
// (pipeline.rot_series, bit for bit).

namespace {
__device__ __constant__ double kRotA[24] = {
    1.0, -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
    -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15,
    -8.22063524662433e-18, 1.9572941063391263e-20, -3.868170170630684e-23, 6.446950284384474e-26,
    -9.183689863795546e-29, 1.1309962886447716e-31, -1.216125041553518e-34, 1.151633562077195e-37,
    -9.67759295863189e-41, 7.265460179153071e-44, -4.902469756513544e-47, 2.9893108271424046e-50,
    -1.6552108677421951e-53, 8.359650847182804e-57, -3.866628513960594e-60};  // (-1)^k / (2k+1)!
__device__ __constant__ double kRotB[24] = {
    0.5, -0.041666666666666664, 0.001388888888888889, -2.48015873015873e-05, 2.755731922398589e-07,
    -2.08767569878681e-09, 1.1470745597729725e-11, -4.779477332387385e-14, 1.5619206968586225e-16,
    -4.110317623312165e-19, 8.896791392450574e-22, -1.6117375710961184e-24, 2.4795962632247976e-27,
    -3.279889237069838e-30, 3.7699876288159054e-33, -3.8003907548547434e-36, 3.387157535521162e-39,
    -2.6882202662866363e-42, 1.911963205040282e-45, -1.2256174391283858e-48, 7.117406731291439e-52,
    -3.7618428812322616e-55, 1.817315401561479e-58, -8.055476070751236e-62};  // (-1)^k / (2k+2)!

// R = I + A [a]x + B [a]x^2, A = sin(th) / th, B = (1 - cos th) / th^2, th = |a|
__device__ void rot_series(const double* a, double* R) {
  const double t2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
  double A = kRotA[23], B = kRotB[23];
  for (int k = 22; k >= 0; --k) {
    A = A * t2 + kRotA[k];
    B = B * t2 + kRotB[k];
  }
  const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double k2 = a[i] * a[j] - (i == j ? t2 : 0.0);
      R[3 * i + j] = ((i == j ? 1.0 : 0.0) + A * K[3 * i + j]) + B * k2;
    }
}

// One launch over the window's landmarks; every workgroup forms pose(t)
// itself, workgroup 0 also writes the cameras.  A camera with a source index
// / a landmark whose track ID the previous window holds takes the previous
// solve's value when that solve succeeded, else keeps the host's (the loop's
// state before the solve); a landmark with ID >= new_from is new in t (moved
// when pose(t) changed).
__global__ __launch_bounds__(256) void vo_chain_kernel(const double* pc, const double* pp, const State* pst, double* cams,
                                                       int nc, double* pts, int np, const int* cam_src,
                                                       const int* win_ids, const int* prev_ids, int n_prev,
                                                       int new_from, me_vo_chain_args a) {
  __shared__ double sh[6 + 9];  // pose(t) | its rotation
  const bool ok = pst->termination != 2;
  auto cam = [&](int k, int j) {
    const int s = cam_src[k];
    return ok && s >= 0 ? pc[6 * s + j] : cams[6 * k + j];
  };
  if (threadIdx.x == 0) {
    double p2[6];
    for (int j = 0; j < 6; ++j) {
      if (a.mode != 1 && a.mode != 0) {  // kept: k1 / k0 are not checked for this mode, so not read either
        p2[j] = cams[6 * (nc - 1) + j];
        continue;
      }
      const double c1 = cam(a.k1, j);
      p2[j] = a.mode == 1 ? c1 + (c1 - cam(a.k0, j)) : c1 + a.vel[j];
    }
    for (int j = 0; j < 6; ++j) sh[j] = p2[j];
    rot_series(p2 + 3, sh + 6);
  }
  __syncthreads();
  if (blockIdx.x == 0) {  // (formed in LDS first: cam() reads the fallbacks in place)
    extern __shared__ double scam[];
    for (int e = threadIdx.x; e < 6 * nc; e += blockDim.x) scam[e] = e >= 6 * (nc - 1) ? sh[e % 6] : cam(e / 6, e % 6);
    __syncthreads();
    for (int e = threadIdx.x; e < 6 * nc; e += blockDim.x) cams[e] = scam[e];
  }
  bool moved = false;
  for (int j = 0; j < 6; ++j) moved = moved || sh[j] != a.pose[j];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  // landmark i's source: its track ID in the previous window's ascending IDs
  const int id = win_ids[i];
  int s = -2;
  if (id < new_from) {
    int lo = 0, hi = n_prev;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (prev_ids[mid] < id)
        lo = mid + 1;
      else
        hi = mid;
    }
    s = lo < n_prev && prev_ids[lo] == id ? lo : -1;
  }
  double* X = pts + 3 * (long)i;
  if (s >= 0) {
    if (ok)
      for (int k = 0; k < 3; ++k) X[k] = pp[3 * (long)s + k];
  } else if (s == -2 && moved) {
    const double* R = a.R;
    const double* R2 = sh + 6;
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = (((X[0] * R[3 * k] + X[1] * R[3 * k + 1]) + X[2] * R[3 * k + 2]) + a.pose[k]) - sh[k];
    double y[3];
    for (int k = 0; k < 3; ++k) y[k] = (d[0] * R2[k] + d[1] * R2[3 + k]) + d[2] * R2[6 + k];
    for (int k = 0; k < 3; ++k) X[k] = y[k];
  }
}
}  // namespace

// BundleAdjuster<M>::initialiseObservations on the device
// (BundleAdjuster.h:354-376): for a window whose observations are stored by
// frame and track ID, camIdx = frame - first_frame and ptIdx = the track's
// index among the window's tracks (win_ids ascending: the order of the
// reference's observations vector).  One thread per observation, binary
// search over win_ids; an ID absent from the window gets -1 (the BA plan then
// reports bad input).
__global__ void window_indices_kernel(const int32_t* __restrict__ frame, const int32_t* __restrict__ ids, int n_obs,
                                      int f0, const int32_t* __restrict__ win_ids, int n_pts,
                                      int32_t* __restrict__ cam_idx, int32_t* __restrict__ pt_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_obs) return;
  const int32_t id = ids[i];
  int lo = 0, hi = n_pts;  // first win_ids[k] >= id
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (win_ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  cam_idx[i] = frame[i] - f0;
  pt_idx[i] = (lo < n_pts && win_ids[lo] == id) ? lo : -1;
}
