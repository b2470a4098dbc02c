/* me_hip.h — C ABI of the MI355X-native stereo-VO hot path (libme_hip.so).
 *
 * Drop-in boundary for abeauvisage/uasl_motion_estimation.  Every entry point
 * names the reference interface it replaces (paths relative to the reference
 * root).  Plain pointers and sizes only: no OpenCV / Eigen / Ceres / torch
 * types cross this boundary.  The C++ adapters that keep the reference's
 * include/MotionEstimation signatures live in include/MotionEstimationAMD/.
 *
 * Conventions
 *  - Every function returns ME_OK (0) or a negative ME_ERR_* code; the
 *    message of the last error on a context is returned by me_last_error().
 *  - One me_ctx per host thread (the reference is single-threaded).  A ctx
 *    owns a HIP device, a stream and scratch memory.
 *  - `mem` = ME_HOST: pointers are host memory, the call copies in/out and
 *    returns when results are on the host.  ME_DEVICE: pointers are device
 *    memory on the ctx device; the call is asynchronous on the ctx stream
 *    (call me_synchronize() before reading results on the host).
 *  - Images are 8-bit grayscale, row-major with a stride in bytes (the
 *    reference reads CV_8U images, src/core/file_IO.cpp:300,304).
 */
#ifndef ME_HIP_H
#define ME_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ME_ABI_VERSION 4

enum {
  ME_OK = 0,
  ME_ERR_INVALID = -1,     /* bad argument / shape (reference: assert / cv::Exception) */
  ME_ERR_HIP = -2,         /* HIP runtime error */
  ME_ERR_NOMEM = -3,
  ME_ERR_UNSUPPORTED = -4,
  ME_ERR_STATE = -5,       /* misuse of a stateful object (reference: std::cerr + status) */
  ME_ERR_NO_DEVICE = -6    /* no HIP device: the product path never falls back to the CPU */
};

typedef enum { ME_HOST = 0, ME_DEVICE = 1 } me_mem;

typedef struct me_ctx me_ctx;

/* ---- context ---------------------------------------------------------- */
int me_abi_version(void);
/* roctx ranges (rocprofv3 --marker-trace): every compute entry point opens
   one named after itself; callers can bracket their own stages (the VO
   loop's KLT / matching / BA / scale stages). */
int me_range_push(const char* name);
int me_range_pop(void);
int me_device_count(int* n);
int me_create(me_ctx** out, int hip_device);
void me_destroy(me_ctx* ctx);
const char* me_last_error(const me_ctx* ctx);
/* Use an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream);
   NULL restores the ctx-owned stream. */
int me_set_stream(me_ctx* ctx, void* hip_stream);
void* me_get_stream(me_ctx* ctx);
/* Restrict the ctx-owned stream to a set of compute units (bit i of mask[i/32]
   = CU i; nwords = 0 restores all CUs): the stream is re-created with
   hipExtStreamCreateWithCUMask after the old one drains.  Lets two contexts
   of one GPU (e.g. a tracking front end and a BA back end) run side by side
   on disjoint CUs instead of sharing every CU's issue slots.  No reference
   counterpart (the reference runs one CPU thread).  hipExtStreamCreateWithCUMask
   takes no flags: the masked stream is a blocking stream (it orders with
   work on the legacy null stream, e.g. torch's default stream), unlike the
   hipStreamNonBlocking stream a ctx owns otherwise; me_stream_flags reports
   the flags of the ctx's current stream.  On MI355X logical CU i sits on XCD
   i mod 8: give each context whole XCDs (CU i to the front end iff
   i mod 8 < k) so the two keep separate L2s -- measured +2 % on the bench
   frame and +7 / +15 % on the config-3 / config-5 VO loop against a split
   that shares every XCD. */
int me_set_cu_mask(me_ctx* ctx, const uint32_t* mask, int nwords);
int me_stream_flags(me_ctx* ctx, unsigned* flags);
/* Compute units of the ctx device (the CU count a me_set_cu_mask split divides). */
int me_cu_count(me_ctx* ctx, int* n);
int me_synchronize(me_ctx* ctx);
int me_malloc(me_ctx* ctx, void** dptr, size_t bytes);
int me_free(me_ctx* ctx, void* dptr);
int me_memcpy_h2d(me_ctx* ctx, void* dst, const void* src, size_t bytes);
int me_memcpy_d2h(me_ctx* ctx, void* dst, const void* src, size_t bytes);
int me_memcpy_d2d(me_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Asynchronous copy in any direction on the ctx stream (page-locked host
   memory from me_host_alloc for a truly asynchronous host side). */
int me_memcpy_async(me_ctx* ctx, void* dst, const void* src, size_t bytes);
int me_host_alloc(me_ctx* ctx, void** hptr, size_t bytes);
int me_host_free(me_ctx* ctx, void* hptr);

/* Per-kernel timing with HIP events on the ctx stream (for bench.py's
   roofline): enable a bitmask of families (bit k = ME_KT k; ME_KT_ALL = every
   family, 0 = off), then read the number of launches and the summed
   milliseconds of a family.  Each timed launch adds two event records to the
   stream, so time only the families a measurement needs. */
enum { ME_KT_MI = 0, ME_KT_SCALE_RES = 1, ME_KT_SCALE_NEQ = 2, ME_KT_BA_LINEARIZE = 3, ME_KT_BA_POINTS = 4,
       ME_KT_BA_SCHUR = 5, ME_KT_BA_SOLVE = 6, ME_KT_BA_STEP = 7, ME_KT_KLT = 8, ME_KT_PYR = 9, ME_KT_NMS = 10,
       ME_KT_CORNERS = 11, ME_KT_RECTIFY = 12, ME_KT_CLAHE = 13, ME_KT_TONEMAP = 14, ME_KT_GATE = 15,
       ME_KT_KEYFRAME = 16, ME_KT_FRAMEPOSE = 17, ME_KT_BA_CHECK = 18, ME_KT_COUNT = 19, ME_KT_ALL = 0x7ffff };
int me_timing_enable(me_ctx* ctx, int family_mask);
int me_timing_read(me_ctx* ctx, int kernel, long* launches, double* total_ms);
int me_timing_reset(me_ctx* ctx);
/* Time only every k-th launch of each timed family (k >= 1; 1 = every launch,
   the default): a live measurement of the average launch duration whose
   event records perturb the stream k times less. */
int me_timing_sample(me_ctx* ctx, int every);
/* Measured HBM bandwidth of this device (GB/s, read + write bytes / time):
   a 16-byte-per-lane streaming copy of `bytes` bytes, `reps` timed launches
   on the ctx stream (after one untimed) -- the measured denominator beside
   the 8 TB/s datasheet peak in bench.py's roofline objects.  Allocates and
   frees 2 x bytes of device memory; synchronises the ctx stream. */
int me_hbm_copy_gbs(me_ctx* ctx, size_t bytes, int reps, double* gbs);

/* ---- A1/A2: mutual information ---------------------------------------
 * Replaces float me::computeMutualInformation(const cv::Mat&, const cv::Mat&)
 * (include/MotionEstimation/core/mutual_information.h:20,
 *  src/core/mutual_information.cpp:55-86), batched: n patch pairs of
 * patch_w x patch_h pixels whose top-left corners are xyL[2k],xyL[2k+1] in imgL
 * and xyR[2k],xyR[2k+1] in imgR (the reference truncates ROI corners to int,
 * SURVEY A-4).  Bit-exact with the reference's float result (20-bin calcHist,
 * fl32(c*fl32(1/N)) normalisation, row-major float sum, glibc log2f). */
int me_mi_scores(me_ctx* ctx, me_mem mem, const uint8_t* imgL, int strideL, const uint8_t* imgR, int strideR,
                 int width, int height, const int32_t* xyL, const int32_t* xyR, int n, int patch_w, int patch_h,
                 float* mi_out);
/* Whole-patch form (any size, the literal computeMutualInformation(L, R)). */
int me_mutual_information(me_ctx* ctx, me_mem mem, const uint8_t* L, int strideL, const uint8_t* R, int strideR,
                          int w, int h, float* mi_out);
/* Epipolar stereo matcher of the VO loop (the application's MI stereo
   matching around me::computeMutualInformation; build-defined like KLT, no
   reference symbol): feature k at (u_k, v_k) of imgL (rectified pair, one
   stride), candidate disparities d = lo_k .. lo_k + nd - 1, left patch at
   (floor(u - patch/2), floor(v - patch/2)), right patch d pixels to its
   left; a candidate is scored (MI, the bits of me_mi_scores) iff its right
   patch starts at x >= 0, d <= d_max and the feature is valid (valid_k != 0
   when valid is given; status_k == 1 and margin <= u < width - margin,
   margin <= v < height - margin when status is given -- the KLT gate).
   Pick: first maximum, interior, FP64 parabola vertex, optional uniqueness
   (best >= ratio * best outside +-2 candidates); xr_k = u_k - disparity
   (float), ok_k = 1 iff the pick holds and xr_k >= margin.  Every array is
   device memory; asynchronous on the ctx stream. */
int me_mi_epipolar_match(me_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int width, int height, int stride,
                         const float* uv, const int32_t* lo, const uint8_t* valid, const uint8_t* status, int n,
                         int nd, int patch, int d_max, int unique, double ratio, float margin, float* xr_out,
                         uint8_t* ok_out);
/* me_mi_epipolar_match over the first *n_dev features (a device count left
   by a preceding kernel, at most n_max), no valid / status gate. */
int me_mi_epipolar_match_count(me_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int width, int height,
                               int stride, const float* uv, const int32_t* lo, const int32_t* n_dev, int n_max,
                               int nd, int patch, int d_max, int unique, double ratio, float margin, float* xr_out,
                               uint8_t* ok_out);
/* ---- A2b: left-right consistency check of the epipolar matcher (build-
 * defined; no reference symbol) -- the stereo twin of me_klt_track_fb: match
 * left -> right, match the right patch that won back into the left image
 * over the same disparity candidates, keep the match only if the way back
 * arrives at the same disparity.  With P = patch, half = patch / 2,
 * x0 = floor((double)u - half), y0 likewise, d_c = lo_f + c, c = 0 .. nd - 1:
 *  1. forward: me_mi_epipolar_match with the same arguments.  xr_out is its
 *     xr_out bit for bit for every feature, ok_f its ok_out; kk is its clamped
 *     pick index and disp_f = (double)(lo_f + kk) + delta its FP64 disparity.
 *  2. backward, only for features with ok_f = 1: the template is the right
 *     patch at the integer winner, corner (xb, y0), xb = x0 - (lo_f + kk);
 *     candidate c is the left patch with corner (xb + d_c, y0) = (x0 + c - kk,
 *     y0); its score is the MI of (that left patch, the template) in
 *     me_mi_scores argument order, computed iff d_c <= d_max, xb + d_c >= 0
 *     and xb + d_c + P <= width, -inf otherwise.  Candidate c = kk is the
 *     forward winner's own pair: the forward score, bit for bit.
 *  3. backward pick: the forward pick's rule with unique = 0 and without the
 *     xr >= margin test (first maximum, interior, finite best and neighbours,
 *     negative curvature, the same FP64 parabola): ok_b and
 *     disp_b = (double)(lo_f + kk_b) + delta_b.
 *  4. gate, FP64, no contraction: a = fabs(disp_b - disp_f);
 *     ok_out = 1 iff ok_f && ok_b && a <= lr_max; lr_err (n floats, may be
 *     NULL) = (float)a, rounded to nearest, when ok_f && ok_b, +inf otherwise.
 * lr_max must be > 0 (NaN, 0, negative: ME_ERR_INVALID); +inf accepts every
 * feature both passes matched.  The other argument checks are the plain
 * call's; n = 0 is allowed.  Device memory, asynchronous on the ctx stream;
 * timed in the ME_KT_MI family.  The numpy restatement is
 * pipeline.match_lr_host.  The _count form is to me_mi_epipolar_match_count
 * what the first is to me_mi_epipolar_match. */
int me_mi_epipolar_match_lr(me_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int width, int height, int stride,
                            const float* uv, const int32_t* lo, const uint8_t* valid, const uint8_t* status, int n,
                            int nd, int patch, int d_max, int unique, double ratio, float margin, double lr_max,
                            float* xr_out, uint8_t* ok_out, float* lr_err);
int me_mi_epipolar_match_lr_count(me_ctx* ctx, const uint8_t* imgL, const uint8_t* imgR, int width, int height,
                                  int stride, const float* uv, const int32_t* lo, const int32_t* n_dev, int n_max,
                                  int nd, int patch, int d_max, int unique, double ratio, float margin, double lr_max,
                                  float* xr_out, uint8_t* ok_out, float* lr_err);
/* New-feature cells of the VO loop (pipeline.new_cells on the device; no
   reference symbol -- the application's grid detector around WBA_Point
   creation): tracked feature k is good iff status_k == 1, ok_k != 0 and it
   lies inside the margin; good features occupy their grid cell
   (trunc((u - margin) / cw), trunc((v - margin) / ch)) clamped, FP64; the
   first max(0, n_feats - #good) empty cells in ascending order get a feature
   at margin + (cell + 0.5 + jitter(t, cell)) * (cw, ch) (float), lo = d_min;
   *out_count = their number.  Device memory, asynchronous on the ctx stream:
   with me_mi_epipolar_match_count the new features are matched in the same
   submission as the tracked ones. */
int me_vo_new_cells(me_ctx* ctx, const float* uv, const uint8_t* status, const uint8_t* ok, int n, int width,
                    int height, float margin, int nx, int ny, double cw, double ch, int n_feats, int t, int d_min,
                    float* out_uv, int32_t* out_lo, int32_t* out_count);
/* me::computeEntropy (src/core/mutual_information.cpp:28-45). */
int me_entropy(me_ctx* ctx, me_mem mem, const uint8_t* img, int stride, int w, int h, float* out);

/* ---- A3: the other patch utilities of src/core/mutual_information.cpp -
 * Batched over n pairs of rows x cols float patches stored contiguously
 * (pair k at A + k * rows * cols, row-major).  me_compare_pc replaces
 * me::comparePC (mutual_information.cpp:14-25, bit-exact); me_ccoeff_normed
 * replaces me::applyCCOEFFNormed (:136-140; OpenCV MatExpr rounding restated,
 * parity unpinned); me_quantise replaces me::quantise(img, {lo, hi}) (:48-53),
 * in place, lo != hi. */
int me_compare_pc(me_ctx* ctx, me_mem mem, const float* A, const float* B, int n, int rows, int cols, float* out);
int me_ccoeff_normed(me_ctx* ctx, me_mem mem, const float* A, const float* B, int n, int rows, int cols, float* out);
int me_quantise(me_ctx* ctx, me_mem mem, uint8_t* img, int stride, int w, int h, int lo, int hi);

/* ---- A4-A9: ScaleState optimiser --------------------------------------
 * Replaces me::optimisation::Optimiser<ScaleState, std::vector<std::pair<cv::Mat,cv::Mat>>>
 * (include/MotionEstimation/optimisation/optimisation.h:76-125,
 *  src/optimisation/optimisation.cpp:29-228,435-747).  The state is the
 * flattened ScaleState: tracks (WBA_Ptf) as homogeneous points + flags, the
 * last poses of the window, intrinsics, scale, baseline, window size and the
 * last keyframe image pair (m_obs[poses.first.size()-1]). */
typedef struct {
  int n_left, n_right;
  const double* X_left;      /* 4*n_left, WBA_Point::get3DLocation() */
  const double* X_right;     /* 4*n_right */
  const uint8_t* tri_left;   /* WBA_Point::isTriangulated() */
  const uint8_t* tri_right;
  const uint32_t* last_left; /* WBA_Point::getLastFrameIdx() */
  const uint32_t* last_right;
  uint32_t lframe;           /* poses.first[0].ID + poses.first.size()-1 */
  double K1[9], K2[9];       /* state.K.first / .second, row-major */
  double q1[4], t1[3];       /* poses.first.back(): Quat (w,x,y,z), position */
  double q2[4], t2[3];       /* poses.second.back() */
  double scale, baseline;
  int window_size;
  const uint8_t* imgL;       /* m_obs[f_idx].first  (mem = img_mem) */
  const uint8_t* imgR;       /* m_obs[f_idx].second */
  int stride, cols, rows;
  int bb_cols, bb_rows;      /* m_obs[0].first.cols, m_obs[1].first.rows */
  const uint8_t* mask;       /* optional Eigen::VectorXi mask as 0/1 bytes (host) */
  int mask_len;
  me_mem img_mem;
  me_mem tracks_mem;         /* X_*, tri_*, last_* in host (ME_HOST) or device memory; mask is always host */
} me_scale_state;

typedef struct {
  int type;                  /* 0 = OptimType::GN, 1 = OptimType::LM */
  int minim;
  int max_nb_iter;
  double v, tau, mu, abs_tol, grad_tol, incr_tol, rel_tol, alpha;
  int weighting;
} me_optim_params;

/* OptimisationParams() defaults (optimisation.h:31) */
void me_optim_default_params(me_optim_params* p);
/* Optimiser::compute_residuals (optimisation.cpp:149-228): res has
   n_left+n_right slots; *n_rows receives the row count. */
int me_scale_residuals(me_ctx* ctx, const me_scale_state* s, int weighting, double* res, int* n_rows);
/* Optimiser::compute_normal_equations (optimisation.cpp:435-537). */
int me_scale_normal_equations(me_ctx* ctx, const me_scale_state* s, int weighting, const double* res, double* JJ,
                              double* e);
/* Optimiser::compute_jacobian / getJacobian (optimisation.cpp:539-634). */
int me_scale_jacobian(me_ctx* ctx, const me_scale_state* s, int weighting, double* JJ);
/* Optimiser::optimise (optimisation.cpp:29-147): updates s->scale, returns the
   StopCondition (rotation_utils.h:20) in *stop. trace: {e1, scale} per outer
   iteration (optional). */
int me_scale_optimise(me_ctx* ctx, me_scale_state* s, const me_optim_params* p, int test, int* stop,
                      int* iterations, double* trace, int trace_cap, long* mi_evals);
/* Counters of the last me_scale_optimise on this ctx, in the reference loop's
   terms (optimisation.cpp:29-147, :685-730): compute_residuals calls,
   compute_normal_equations calls and rejected LM candidates (the else branch
   of run_LM_step, :719-727).  An evaluation the device skips because its
   result is already known (same state) still counts.  executed = residual
   evaluations the device actually ran (speculative candidates included). */
int me_scale_last_counters(me_ctx* ctx, long* res_evals, long* neq_evals, long* rejections, long* executed);
/* Launch form me_scale_optimise picks for nb track blocks (16 tracks each)
   when `cap` workgroups of the persistent LM kernel fit on the ctx's CUs:
   1 = the one persistent launch (nb x 2 workgroups, at most half of cap),
   0 = one launch per LM phase.  The persistent grid does not need to be
   co-resident (a workgroup roster deals the work over the workgroups that
   run), so this is a throughput choice; no environment
   variable changes it.  Host only: no device, no ctx. */
int me_scale_persistent(int nb, int cap);
/* double ScaleState::compute_residuals(std::vector<std::pair<cv::Mat,cv::Mat>>&)
   (include/MotionEstimation/optimisation/optimisation.h:86, src/optimisation/optimisation.cpp:230-278):
   one mutual information over the stacked 2w x 2w patch pairs of the left
   tracks (triangulated, seen in the last keyframe, both reprojections inside
   Rect(w, w, cols - 2w, rows - 2w)).  The reference's stacking
   (`left_img(Range..) = imgs[i].first`, :273-274) rebinds a temporary ROI
   header and copies no pixels, so its stacked images are uninitialised and
   its result undefined; this computes the evident intent (the MI of the
   stacked patches), parity unpinned.  n_patches (optional) receives the
   number of stacked pairs; none -> ME_ERR_INVALID (the reference's
   computeMutualInformation asserts on empty input). */
int me_scale_state_mi(me_ctx* ctx, const me_scale_state* s, double* mi_out, int* n_patches);
/* Optimiser::compute_inliers (optimisation.cpp:732-747): row indices. */
int me_scale_inliers(me_ctx* ctx, const me_scale_state* s, int weighting, double threshold, int* idx, int cap,
                     int* n_out);

/* ---- A13-A17: windowed stereo bundle adjustment ----------------------
 * Replaces me::optimisation::BundleAdjuster<4>::optimise(int fixedFrames)
 * (include/MotionEstimation/optimisation/BundleAdjuster.h:142-180,431-476)
 * and the Ceres solve it wraps: StereoReprojectionError residual/Jacobian,
 * HuberLoss(1.0), LM trust region with Jacobi scaling, point-first Schur
 * elimination, box bounds on points.  cams are Matx61d {t, angle-axis}
 * (BundleAdjuster.h:297-310), observations Observation<4>.
 * obs_dim = 2 selects BundleAdjuster<2>::optimise (BundleAdjuster.h:378-429):
 * Observation<2> {x, y} with cam_id = Observation::camID, residual
 * StandardReprojectionError (:71-103) for camID 0 and StereoRightError
 * (:106-139) otherwise, K[0] only, a zero baseline replaced by 0.5 (:389-390). */
typedef struct {
  int n_cams, n_pts, n_obs;
  double* cams;              /* n_cams*6, updated in place */
  double* pts;               /* n_pts*3, updated in place */
  const double* obs;         /* n_obs*4 {xL, yL, xR, yR} */
  const int32_t* cam_idx;    /* Observation::camIdx */
  const int32_t* pt_idx;     /* Observation::ptIdx */
  double K0[9], K1[9];       /* CalibrationParameters::K[0], K[1] */
  double baseline, feat_var;
  int fixed_frames;          /* optimise(fixedFrames) */
  me_mem mem;                /* ME_HOST: the arrays above are host memory (copied in/out);
                                ME_DEVICE: device memory on the ctx device, cams/pts updated in
                                place on the device (me_ba_solve / me_ba_solve_sharded only) */
  int obs_dim;               /* 4 (or 0): Observation<4>; 2: Observation<2> (BundleAdjuster<2>) */
  const int32_t* cam_id;     /* obs_dim 2: Observation::camID per observation; ignored otherwise */
} me_ba_problem;

typedef struct {
  int max_num_iterations;          /* Ceres default 50 */
  double function_tolerance;       /* 1e-3 (BundleAdjuster.h:465) */
  double gradient_tolerance;       /* 1e-10 */
  double parameter_tolerance;      /* 1e-8 */
  double initial_trust_region_radius, max_trust_region_radius, min_trust_region_radius;
  double min_lm_diagonal, max_lm_diagonal, min_relative_decrease;
  int max_num_consecutive_invalid_steps;
  int jacobi_scaling;
} me_ba_options;

typedef struct {
  int status;                /* BundleAdjuster::Status: 2 SUCCESSFUL, 3 FAILED */
  int termination;           /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE */
  int iterations;
  int successful_steps;
  double initial_cost, final_cost;
} me_ba_summary;
/* final_cost.  With gradient_tolerance > 0 (or max_num_iterations == 0) a solve
   that reaches the iteration limit linearises once more at its final point for
   the closing gradient test, and final_cost is that linearisation's cost.  With
   gradient_tolerance <= 0 and max_num_iterations > 0 that pass is not run: the
   last step's decision ends the solve, and final_cost is the candidate cost of
   the last accepted step -- the same quantity, summed from the step
   evaluation's residuals, not the linearisation's (equal to about 1e-13
   relative).  A final point whose gradient is exactly zero in every component
   then reports the iteration limit (termination 1), not convergence: with the
   tolerance at 0 only such a gradient could pass the closing test. */

void me_ba_default_options(me_ba_options* o);
int me_ba_solve(me_ctx* ctx, me_ba_problem* p, const me_ba_options* o, me_ba_summary* s);
/* Asynchronous form of me_ba_solve (same BundleAdjuster<M>::optimise,
   BundleAdjuster.h:378-476, same results bit for bit): queues every
   possible iteration (max_num_iterations linearisations, one more where the
   closing gradient test runs, see me_ba_summary; launches after
   convergence return at once, so it suits fixed-iteration windows) and the
   read-back on the ctx stream, and returns without waiting.  The caller keeps
   *p's arrays alive until me_ba_wait, which blocks on this solve only (not on
   work queued after it), writes host-problem results back and fills *s.  Up
   to two solves may be queued per ctx (each in its own scratch and staging):
   window t+1 can be queued behind window t before t is waited, so the device
   never idles while the host builds the next plan; me_ba_wait completes the
   oldest.  A third me_ba_solve_async before a wait is ME_ERR_STATE.  Any other
   BA call on the ctx completes the queued solves first (their summaries stay
   readable by me_ba_wait). */
int me_ba_solve_async(me_ctx* ctx, me_ba_problem* p, const me_ba_options* o);
int me_ba_wait(me_ctx* ctx, me_ba_summary* s);
/* me_ba_wait, and for a device-resident problem (ME_DEVICE) its solved cams
   (6 per camera) / pts (3 per point) copied to host arrays (either may be
   NULL): read back behind the solve, so the wait does not block on work
   queued after it. */
int me_ba_wait_out(me_ctx* ctx, me_ba_summary* s, double* cams, double* pts);
/* me_ba_wait_out, and the window covariance that me_vo_window_submit queued
   behind the solve (me_vo_window.cov), from the same staging: cam_cov
   (n_cams*36) and pt_cov (n_pts*9, written only when cov was 2) as
   me_ba_covariance_full gives them at the cams / pts the solve left.
   *cov_ok = the queued mode (1 or 2) when the covariance succeeded, else 0
   with both arrays untouched (none queued, ok = 0, or the wait failed).  Any
   of the three may be NULL. */
int me_ba_wait_out_cov(me_ctx* ctx, me_ba_summary* s, double* cams, double* pts, double* cam_cov, double* pt_cov,
                       int* cov_ok);
/* me_ba_wait_out_cov, and the flags of the residual check that
   me_vo_window_submit queued behind the solve (me_vo_window.check), from the
   same staging and with no further wait: flags (n_pts bytes) and
   *check_ok = 1.  *check_ok = 0 with flags untouched when none was queued,
   the solve failed (termination 2) or the wait failed.  flags and check_ok
   may be NULL.  me_ba_wait, me_ba_wait_out and me_ba_wait_out_cov are this
   call with the outputs they lack NULL. */
int me_ba_wait_out_check(me_ctx* ctx, me_ba_summary* s, double* cams, double* pts, double* cam_cov, double* pt_cov,
                         int* cov_ok, uint8_t* flags, int* check_ok);
/* Sizes the ctx's BA scratch and page-locked staging (synchronous, both
   asynchronous sets, the window covariance's set, me_ba_covariance_full, and
   the residual check's flags, me_ba_point_check) for windows up to these sizes, so a growing window does
   not reallocate (a reallocation waits for the ctx stream).  No solve may be
   queued. */
int me_ba_reserve(me_ctx* ctx, int n_cams, int n_pts, int n_obs, int obs_dim, int fixed_frames);
/* Windowed VO loop (pipeline.py WindowedStereoVO.process, step 7), no
   counterpart in the reference (whose loop solves each window before the
   next keyframe, WBA_Point / BundleAdjuster.h): window t's BA start formed on
   the device from the last queued device-resident solve (window t-1) before
   that solve completes.  cams (n_cams x 6) / pts (n_pts x 3), device memory,
   hold the host's values (the loop state before window t-1's result); camera
   k with cam_src >= 0 takes that solve's camera cam_src, landmark i (track ID
   win_ids[i]) that solve's point of the same ID in prev_ids (window t-1's
   ascending IDs, n_prev), when it succeeded (termination != FAILURE); a
   landmark with ID >= new_from is new in keyframe t, moved from pose
   (rotation R, row-major) to the new pose(t) when they differ; camera
   n_cams - 1 is pose(t):
   mode 1: c[k1] + (c[k1] - c[k0]), mode 0: c[k1] + vel, mode -1: kept (k1
   and k0 are neither checked nor read).  The new pose's rotation is a fixed
   Taylor series in theta^2 (the loop's host code repeats the arithmetic bit
   for bit).  Asynchronous on the ctx stream. */
typedef struct me_vo_chain_args {
  double pose[6];
  double R[9];
  double vel[6];
  int k1, k0, mode;
} me_vo_chain_args;
int me_vo_ba_chain(me_ctx* ctx, double* cams, int n_cams, double* pts, int n_pts, const int32_t* cam_src,
                   const int32_t* win_ids, const int32_t* prev_ids, int n_prev, int32_t new_from,
                   const me_vo_chain_args* a);
/* Per-landmark residual check of a BA problem at its current parameters
   (build-defined: the reference has no counterpart).  Read
   only.  Per observation o, with the sigma-scaled residual r of me_ba_evaluate
   (rows 2, 3 zero for obs_dim 2) and the camera-frame depth Z_o (the third
   coordinate of R X + t):
     s_o = ((r0 r0 + r1 r1) + r2 r2) + r3 r3      (FP64, no contraction: the
                                                   BA cost's sum without the
                                                   Huber correction)
   Per landmark i over all of its observations, constant cameras included:
     chi2[i]  = max s_o; a non-finite s_o counts as +inf; no observation: 0
     flags[i] bit 0 (1): !(chi2[i] <= chi2_max)
              bit 1 (2): some observation has !(Z_o > z_min)
   so a NaN landmark sets both bits.  A maximum and an "any": the result does
   not depend on the order of the observation arrays, bit for bit.
   Defaults (me_ba_point_check_default_params): chi2_max = 18.47, the 99.9 %
   point of chi-square with 4 degrees of freedom, and z_min = 0 -- both from
   the statistics of a 4-row residual with the stated sigma, not tuned on real
   data.  chi2_max must be > 0 (+inf allowed), z_min finite and >= 0; NaN is
   ME_ERR_INVALID.  params NULL: the defaults.
   ME_HOST problems: host outputs, chi2 (n_pts, may be NULL), flags (n_pts),
   *n_flagged (may be NULL) = landmarks with flags != 0; the call returns with
   them.  ME_DEVICE problems: chi2 / flags are device pointers, n_flagged must
   be NULL and the call is asynchronous on the ctx stream; like
   me_ba_covariance_full it does not wait for solves queued on the ctx and
   works in that call's scratch set (me_ba_reserve sizes it).  A
   device-resident problem whose observations index outside the window gets
   +inf and both bits everywhere.  One launch, timed as ME_KT_BA_CHECK. */
typedef struct me_ba_point_check_params {
  double chi2_max;
  double z_min;
} me_ba_point_check_params;
void me_ba_point_check_default_params(me_ba_point_check_params* p);
int me_ba_point_check(me_ctx* ctx, const me_ba_problem* p, const me_ba_point_check_params* params,
                      double* chi2 /* n_pts or NULL */, uint8_t* flags /* n_pts */, int* n_flagged);
/* One keyframe's window solve in one call (for a thread that queues window t
   while another waits for window t-1 with me_ba_wait_out -- the two may run
   concurrently on one ctx; no other call on the ctx meanwhile): the staged
   H2D (stage -> dev, stage_bytes, may be 0), me_vo_ba_chain when `chain`
   (on p->cams / p->pts), me_ba_window_indices (frame / ids of the window's
   p->n_obs observations, first_frame, win_ids -> p->cam_idx / p->pt_idx),
   me_ba_solve_async(p, o). */
typedef struct me_vo_window {
  const void* stage;
  void* dev;
  size_t stage_bytes;
  int chain;
  const int32_t* cam_src;
  const int32_t* win_ids;
  const int32_t* prev_ids;
  int n_prev;
  int32_t new_from;
  me_vo_chain_args args;
  const int32_t* frame;
  const int32_t* ids;
  int first_frame;
  int cov; /* 0: none.  1 / 2: the window covariance (camera blocks / also landmark blocks, me_ba_covariance_full)
              queued directly behind the solve on the ctx stream, in scratch of its own, read back into the solve's
              staging ahead of its event: me_ba_wait_out_cov returns it with the solve's result, no further wait */
  const me_ba_point_check_params* check; /* NULL: none.  Else me_ba_point_check at the cams / pts the solve leaves,
              launched directly behind the solve (behind the covariance when both are asked for); its flags (n_pts
              bytes) go into the solve's staging ahead of its event: me_ba_wait_out_check returns them */
} me_vo_window;
int me_vo_window_submit(me_ctx* ctx, const me_vo_window* w, me_ba_problem* p, const me_ba_options* o);
/* ---- the windowed stereo VO loop, native (round 5) ----------------------
 * The application loop around the hot path (pipeline.py WindowedStereoVO
 * with its GPU backend, every step in C++ behind this ABI): per keyframe t
 * the KLT of the active tracks, the epipolar MI matching of the tracked and
 * of the new features (one front-end round trip), the WBA_Point bookkeeping
 * (include/MotionEstimation/core/feature_types.h:121-197: IDs from the value
 * constructor, addMatch, pop of features leaving the window, deletion of
 * empty tracks) over a structure-of-arrays track table, the scale LM
 * (Optimiser<ScaleState,...>::optimise, optimisation.cpp:29-147) of keyframe
 * t-1 and the sliding-window BA (BundleAdjuster<4>::optimise over the last
 * `window` keyframes, initialiseObservations order, BundleAdjuster.h:354-376,
 * 431-476) queued behind the previous window's solve (me_vo_window_submit).
 * The loop is lagged exactly as pipeline.py's: BA(t-1) enters the state after
 * keyframe t is matched and booked.  Two contexts of one device: `ba` runs the
 * window solves, `front` the KLT, the matchers and the scale LM (they may be
 * the same ctx: then nothing runs on a worker thread).  Results are the
 * Python loop's bit for bit (tests/test_pipeline.py (test_native_loop_*, test_cpp_host_drives_the_loop)).  One loop per pair of
 * contexts; no other call on either ctx while a loop call runs. */
typedef struct {
  int width, height, n_feats, window;
  int ba_iters, scale_iters, fixed_frames, d_min, d_max;
  double baseline, feat_var;
  double K[9];                /* row-major intrinsics (both cameras) */
  double first_pose[6];       /* {t, angle-axis} world -> camera of keyframe 0 */
  double velocity[6];         /* motion prior of keyframe 1 (has_velocity) */
  int has_velocity;
  int log_events;             /* keep the WBA_Point event log (me_vo_loop_events) */
  int async_enqueue;          /* window solves queued from a worker thread (ignored when ba == front) */
  int detector;               /* new features of a keyframe: 0 grid (me_vo_new_cells), 1 corners (me_vo_new_corners) */
  int corner_win;             /* me_corner_params of the corner detector (21, 1e-4) */
  double corner_min_eig;
  double klt_fb_max;          /* > 0: the tracker is me_klt_track_fb with this bound (pixels); 0: me_klt_track */
} me_vo_loop_config;
typedef struct {              /* pipeline.FrameResult */
  int t, n_tracked, n_new, n_active, n_window_pts, n_window_obs;
  double scale;
  int scale_stop, scale_iters, ba_iters;
  double ba_cost;
  double pose[6];
} me_vo_frame_result;
typedef struct {              /* one WBA_Point call: kind 0 new (value ctor), 1 addMatch, 2 pop, 3 deleted */
  int kind, t;
  int64_t id;
  float feat[4];              /* {xl, yl, xr, yr} (new / add) */
} me_vo_event;
typedef struct me_vo_loop me_vo_loop;
void me_vo_loop_default_config(me_vo_loop_config* c);
int me_vo_loop_create(me_ctx* ba, me_ctx* front, const me_vo_loop_config* cfg, me_vo_loop** out);
void me_vo_loop_destroy(me_vo_loop* v);
const char* me_vo_loop_last_error(const me_vo_loop* v);
/* The left-right check of the loop's stereo matches (A2b): lr_max > 0 makes
   every matcher call of the loop its _lr form with that bound (disparity
   pixels); 0 (the default) switches it off.  NaN or negative: ME_ERR_INVALID;
   after the first me_vo_loop_process: ME_ERR_STATE.  (A setter, not a
   me_vo_loop_config field: the struct and the ABI version stay as they are.) */
int me_vo_loop_set_match_lr(me_vo_loop* v, double lr_max);
/* Guided tracking inside the loop (A12f): on = 1 predicts pose(t) before the
   KLT is queued (the prediction of step 3: the pops in between change none of
   its inputs), projects every active landmark with it -- Z as in the disparity
   prediction, Xc = (X0 R00 + X1 R01) + X2 R02 + t0, Yc likewise with row 1,
   u = f Xc / Z + cx, v = f Yc / Z + cy in FP64 (f = K[0], cx = K[2],
   cy = K[5]), cast to float, NaN where Z <= 0 -- uploads the guesses behind
   the features in the same copy, and tracks with me_klt_track_guided
   (me_klt_track_guided_fb when klt_fb_max > 0).  Everything downstream is
   unchanged.  0 (the default): the loop makes exactly the calls it makes
   without this setter.  Other values: ME_ERR_INVALID; after the first
   me_vo_loop_process: ME_ERR_STATE. */
int me_vo_loop_set_klt_predict(me_vo_loop* v, int on);
/* Window covariance (NULL: off, the default; set before the first frame).
   Every window's covariance is queued on the BA context's stream directly
   behind that window's solve and ahead of the next window's submission,
   evaluated at the cams and pts the solve leaves, and read back with the
   solve's own result: no extra host wait per keyframe, and read only (events,
   poses and results are those of the loop without it).  The gauge is the
   BA's own: the window's first fixed_frames cameras are constant, so their
   blocks are zero and every block is relative to them.  landmarks != 0 also
   computes the landmark blocks.
   me_vo_loop_pose_covs: per keyframe t that had a window of its own, the
   6x6 block of that window's last camera (cov36, row-major) and ok.
   me_vo_loop_track_covs: per live track (the order of me_vo_loop_tracks), the
   3x3 block from the latest window that held it (cov9) and ok.  A failed
   solve (termination 2) or a covariance with ok = 0 leaves zeros with ok = 0
   and does not stop the loop.  Both readers: *n = entries, at most cap
   written; outputs may be NULL. */
typedef struct me_vo_cov_params {
  int landmarks;
} me_vo_cov_params;
int me_vo_loop_set_covariance(me_vo_loop* v, const me_vo_cov_params* p);
int me_vo_loop_pose_covs(me_vo_loop* v, int32_t* ts, double* cov36, uint8_t* ok, int cap, int* n);
int me_vo_loop_track_covs(me_vo_loop* v, int64_t* ids, double* cov9, uint8_t* ok, int cap, int* n);
/* Residual check behind every window solve (NULL: off, the default; set
   before the first frame; parameters as me_ba_point_check, else
   ME_ERR_INVALID).  Every window's check is queued with its solve
   (me_vo_window.check) and read back with its result: no extra host wait.
   When window t-1's result is applied (step 7 of keyframe t), every live
   track of that window with flags != 0 is made inactive: it keeps the
   observations it has (keyframe t's included: BA(t) may already be queued),
   is tracked no further from keyframe t+1 on, frees its cell for a new
   feature and leaves the window by the ordinary pops.  A failed solve
   (termination 2) applies no flags.  No event kind is added; independent of
   the covariance, motion gate, keyframe selection and frame pose switches.
   me_vo_loop_flagged: every (window keyframe, track ID, flags) applied so far,
   in the order applied (window by window, table order inside one); *n =
   entries, at most cap written; outputs may be NULL. */
int me_vo_loop_set_track_check(me_vo_loop* v, const me_ba_point_check_params* p /* NULL: off */);
int me_vo_loop_flagged(me_vo_loop* v, int32_t* ts, int64_t* ids, uint8_t* flags, int cap, int* n);
/* Rectification inside the loop (A12d): with two camera models the loop builds
   their maps once on the front context -- the rectified model is the loop's
   own width, height and K (fx = K[0], fy = K[4], cx = K[2], cy = K[5]) -- and
   me_vo_loop_process takes raw images from then on: left is
   left->width x left->height, right is right->width x right->height (stride =
   width each; the two sizes may differ).  Both are remapped (me_remap_q5,
   `border` outside) into loop-owned device buffers on the front-end stream
   ahead of the KLT, and every later stage reads the rectified pair; the
   lifetime rule of caller images is unchanged.  Two NULL models switch it off
   (the default); one NULL model, a bad model or border: ME_ERR_INVALID; after
   the first me_vo_loop_process: ME_ERR_STATE. */
struct me_camera_model; /* defined in section A12d below */
int me_vo_loop_set_rectify(me_vo_loop* v, const struct me_camera_model* left, const struct me_camera_model* right,
                           int border);
/* Local contrast equalisation inside the loop (A12e): with parameters both
   images of every keyframe are equalised (me_clahe, stride = width) on the
   front-end stream ahead of the KLT -- after the remaps when the loop also
   rectifies -- and every later stage (KLT, corner detector, both matchers,
   scale LM) reads the equalised pair.  Caller-owned device images are never
   written: they are equalised into a loop-owned pair (the loop's pool of at
   most four pairs: a frame takes one that neither the previous pushed frame
   nor the last two keyframes hold); uploaded, tone-mapped and rectified pairs
   are equalised in place.  The lifetime rule of caller images is unchanged.
   NULL switches it off (the default: the loop runs exactly the calls it runs
   without this setter).  Bad parameters (me_clahe's rules, against the loop's
   width x height): ME_ERR_INVALID, and the switch is left off; after the first
   me_vo_loop_process: ME_ERR_STATE. */
struct me_clahe_params; /* defined in section A12e below */
int me_vo_loop_set_equalise(me_vo_loop* v, const struct me_clahe_params* p /* NULL: off */);
/* Keyframe t (t = 0, 1, 2, ... in order): left / right 8-bit images of
   width x height (stride = width).  mem = ME_DEVICE: device memory on the
   ctx device, read during this call and the next one (keep it alive until
   me_vo_loop_process(t + 1) returns); ME_HOST: copied in. */
int me_vo_loop_process(me_vo_loop* v, int t, const uint8_t* left, const uint8_t* right, me_mem mem);
/* 16-bit ingest (A12g): with parameters the loop takes 16-bit keyframes
   through me_vo_loop_process16 and reduces them to 8 bits itself.  Each camera
   has a tone-map state of its own, created by the loop.  NULL switches it off
   (the default: the loop makes exactly the calls it makes without this
   setter).  Bad parameters (me_tonemap16's rules): ME_ERR_INVALID, and the
   switch is left off; after the first process call: ME_ERR_STATE. */
struct me_tonemap_params; /* defined in section A12g below */
int me_vo_loop_set_tonemap(me_vo_loop* v, const struct me_tonemap_params* p /* NULL: off */);
/* The rigid-motion gate inside the loop (A12h): with parameters every keyframe
   with tracked features queues me_motion_gate right after their stereo match,
   on the same stream, in place on the ok byte that me_vo_new_cells /
   me_vo_new_corners and the host's `good` mask read: a rejected track leaves
   the window and frees its cell in the same keyframe, and the keyframe keeps
   its single submission and round trip.  The previous keyframe's x_r (4 bytes
   per feature) is uploaded behind the tracker's input.  t is the keyframe
   number, f / cx / cy / baseline / margin the loop's.  NULL switches the gate
   off (the default: the loop queues what it queued without this setter).  The
   first keyframe's matches are not gated.  Bad parameters (me_motion_gate's
   rules) are ME_ERR_INVALID, a call after the first me_vo_loop_process
   ME_ERR_STATE. */
struct me_motion_gate_params; /* defined in section A12h below */
int me_vo_loop_set_motion_gate(me_vo_loop* v, const struct me_motion_gate_params* p /* NULL: off */);
/* Keyframe t as 16-bit images: width x height of the loop (stride = width), or
   the two camera models' raw sizes when the loop rectifies.  ME_ERR_STATE
   unless me_vo_loop_set_tonemap is on.  The two tone maps (me_tonemap16, each
   with its camera's state) are queued on the front-end stream first, into a
   loop-owned 8-bit pair (the keyframe's pair of the loop's pool, or with a
   rectifier one raw-size buffer reused in stream order, which the remaps
   read); caller images are never written.  Then the remaps, the
   CLAHE and every later stage run as in me_vo_loop_process on that 8-bit pair.
   Nothing is read back: a keyframe keeps its one submission and round trip.
   mem and the lifetime rule of caller device images are me_vo_loop_process's.
   The keyframes of one loop all come through this entry or all through
   me_vo_loop_process: mixing them is ME_ERR_STATE. */
int me_vo_loop_process16(me_vo_loop* v, int t, const uint16_t* left, const uint16_t* right, me_mem mem);
/* Keyframe selection inside the loop (A12i): with parameters the loop takes
   camera frames through me_vo_loop_push and chooses its keyframes itself.
   NULL switches it off (the default: me_vo_loop_push is ME_ERR_STATE and the
   loop makes exactly the calls it makes without this setter).  Bad parameters
   (me_kf_update's rules) and a loop whose tone map is on (its temporal state
   per pushed frame is not defined) are ME_ERR_INVALID; after the first frame:
   ME_ERR_STATE. */
struct me_kf_params; /* defined in section A12i below */
int me_vo_loop_set_keyframe_select(me_vo_loop* v, const struct me_kf_params* p /* NULL: off */);
/* One camera frame (8-bit images as me_vo_loop_process takes them; ME_DEVICE
   images are read during this call only: the loop keeps copies).
   *keyframe_t = the keyframe index the frame became, or -1.
    - The first frame is keyframe 0; keyframe indices are consecutive.
    - After keyframe t the state of A12i is seeded from its active tracks, in
      the order the next tracker call uploads them: ref_uv = cur_uv = their
      left positions, alive = 1, gap = 0.
    - Every later frame runs the front-end chain once (remap, CLAHE where
      set), then the loop's tracker (me_klt_track, or me_klt_track_fb when
      klt_fb_max > 0; not guided) from the previous pushed frame to this one
      at cur_uv over all n features, then me_kf_update on the same stream;
      the 32-byte info block is the frame's one read-back.
    - flags == 0: the frame's images become the previous pushed frame and
      nothing else in the loop moves.
    - flags != 0: the keyframe body of me_vo_loop_process runs on the images
      already prepared.  With gap >= 2 its tracker call is the guided form
      (me_klt_track_guided / _guided_fb) from keyframe t - 1's image and
      positions, the guess being cur_uv of the alive features and ref_uv of
      the others; that guess takes the place of me_vo_loop_set_klt_predict's.
      With gap == 1 (no frame in between) the body runs exactly as
      me_vo_loop_process runs it.
   A loop takes its frames through this entry or through me_vo_loop_process,
   not both: ME_ERR_STATE. */
int me_vo_loop_push(me_vo_loop* v, const uint8_t* left, const uint8_t* right, me_mem mem, int* keyframe_t);
/* Frame-rate pose output (A12j): with parameters every pushed frame after the
   first, a frame that becomes a keyframe included, gets a pose relative to the
   last keyframe.  The seed uploads the keyframe's x_r beside ref_uv (4 more
   bytes per feature in the same copy) and zeroes the state's 128-byte pose
   block, which sits directly behind the 32-byte keyframe block; me_frame_pose
   is queued right behind me_kf_update on the same stream with start == info
   (the previous frame's pose is the warm start, identity after a keyframe), and
   one 160-byte copy stays the frame's one read-back.  The estimate is read
   only: it feeds neither the keyframe decision, nor alive, nor the pose
   prediction, so keyframes and events are those of a loop without it.  NULL
   switches it off (the default: the loop makes exactly the calls it makes
   without this setter).  Called after me_vo_loop_set_keyframe_select and
   before the first frame: ME_ERR_INVALID otherwise, and for bad parameters
   (me_frame_pose's rules).  A setter: me_vo_loop_config and ME_ABI_VERSION
   stay as they are. */
struct me_frame_pose_params; /* defined in section A12j below */
int me_vo_loop_set_frame_pose(me_vo_loop* v, const struct me_frame_pose_params* p /* NULL: off */);
/* The frame poses of the pushed frames after the first, in push order
   (*n = their number; min(cap, *n) copied).  t: the keyframe index the frame
   became, or -1; t_ref: the keyframe (R, t) is relative to; gap: frames since
   it; the counts and valid of A12j's info block; X_frame = R X_t_ref + t. */
typedef struct me_vo_frame_pose {
  int32_t frame, t, t_ref, gap, n_usable, n_inliers, steps, valid;
  double R[9], t_rel[3];
} me_vo_frame_pose;
int me_vo_loop_frame_poses(me_vo_loop* v, me_vo_frame_pose* out, int cap, int* n);
/* Completes the last keyframe (its pops, scale LM and BA). */
int me_vo_loop_finish(me_vo_loop* v);
/* Results of the completed keyframes (*n = their number; min(cap, *n) copied). */
int me_vo_loop_results(me_vo_loop* v, me_vo_frame_result* out, int cap, int* n);
int me_vo_loop_events(me_vo_loop* v, me_vo_event* out, long cap, long* n);
/* Live track table (creation = ID order): IDs, landmarks (3 per track), active flag, first held / last frame. */
int me_vo_loop_tracks(me_vo_loop* v, int64_t* ids, double* X, uint8_t* active, int64_t* first, int64_t* last, int cap,
                      int* n);
int me_vo_loop_poses(me_vo_loop* v, int32_t* ts, double* poses, int cap, int* n);
/* Observations of keyframe t still held (ascending track IDs, {xl, yl, xr, yr}); *n = -1 when none. */
int me_vo_loop_frame_obs(me_vo_loop* v, int t, int64_t* ids, float* feats, int cap, int* n);
int me_vo_loop_frames(me_vo_loop* v, int32_t* ts, int cap, int* n);
/* [0] host seconds outside waits, [1] seconds blocked on device results, [2] tracks created (latestID),
   [3..8] seconds blocked in: KLT + matching, first-keyframe matching, scale LM submit, window submit,
   BA result, scale LM result. */
int me_vo_loop_stats(me_vo_loop* v, double* out, int n);

/* BundleAdjuster<M>::initialiseObservations (BundleAdjuster.h:354-376) for a
   device-resident window: observation i was seen in frame[i] by the track
   ids[i]; cam_idx[i] = frame[i] - first_frame and pt_idx[i] = the position of
   ids[i] in win_ids (the window's track IDs, ascending), -1 if absent.  All
   arrays device memory; asynchronous on the ctx stream.  With the
   observations stored frame by frame, a sliding window appends one keyframe's
   observations per step and re-indexes on the device. */
int me_ba_window_indices(me_ctx* ctx, const int32_t* frame, const int32_t* ids, int n_obs, int first_frame,
                         const int32_t* win_ids, int n_pts, int32_t* cam_idx, int32_t* pt_idx);
/* Cost (Ceres ½Σρ) at the problem's current parameters. */
int me_ba_cost(me_ctx* ctx, const me_ba_problem* p, double* cost);
/* Residuals (sigma-scaled, uncorrected) and Jacobian blocks per observation:
   res D/obs, Jc 6D/obs (row-major Dx6), Jp 3D/obs (Dx3), D = obs_dim (4 or 2). */
int me_ba_evaluate(me_ctx* ctx, const me_ba_problem* p, double* res, double* Jc, double* Jp);
/* Reduced camera system of the first LM step at trust radius `radius`
   (scaled coordinates), S (6m x 6m row-major) and b (6m), m = non-fixed cams. */
int me_ba_reduced_system(me_ctx* ctx, const me_ba_problem* p, double radius, double* S, double* b);
/* Pose covariance at the problem's current parameters: replaces
   BundleAdjuster<M>::extract_covariance (BundleAdjuster.h:478-528), i.e.
   ceres::Covariance over the camera blocks with the loss function applied:
   cov[36 i .. 36 i + 35] = 6x6 row-major block i of (J^T J)^-1, obtained as
   the inverse of the point-eliminated camera system; constant (fixed) cameras
   get zero blocks as in Ceres.  *ok = 0 (and cov untouched) when J^T J is not
   positive definite (Ceres reports a rank-deficient Jacobian). */
int me_ba_covariance(me_ctx* ctx, const me_ba_problem* p, double* cov /* n_cams*36 */, int* ok);
/* Window covariance: the camera blocks of me_ba_covariance and the landmark
   blocks the reference declares and never fills (getPointsCovariance /
   m_point_covs, BundleAdjuster.h:239,277; their computation is commented out
   at :498-523).  pt_cov[9 j .. 9 j + 8] = 3x3 row-major block j of (J^T J)^-1,
   by the Schur form: V_j^-1 + sum_a sum_b T_a^T Sigma_cc[a, b] T_b with
   T_a = (Jc^T Jp) V_j^-1 over landmark j's observations in variable cameras
   (loss-corrected rows); a landmark seen only by constant cameras gets V_j^-1.
   The gauge is the BA's own: the first fixed_frames cameras are constant and
   their blocks zero.  Either output may be NULL, not both.  *ok = 0 (outputs
   untouched) exactly where me_ba_covariance reports 0, and when a V_j is not
   positive definite.
   ME_HOST problems: host outputs, the call returns with them.  ME_DEVICE
   problems: cam_cov, pt_cov and ok are device pointers and the call is
   asynchronous on the ctx stream; it does not wait for solves queued on the
   ctx (me_ba_solve_async) and works in a scratch set of its own, which
   me_ba_reserve also sizes. */
int me_ba_covariance_full(me_ctx* ctx, const me_ba_problem* p, double* cam_cov /* n_cams*36 or NULL */,
                          double* pt_cov /* n_pts*9 or NULL */, int* ok);

/* ---- §8e: landmark-sharded BA over several GPUs ----------------------
 * No reference counterpart (the reference solves on one CPU thread); the
 * sharded solve replaces BundleAdjuster<4>::optimise (BundleAdjuster.h:431-476)
 * when the window's landmarks are split over ranks: every rank holds all
 * cameras and a contiguous landmark range with its observations.
 *
 * A communicator joins the ranks, one process (one me_ctx) per GPU:
 *  - me_comm_create_rccl: native RCCL over xGMI.  Rank 0 draws an id with
 *    me_comm_unique_id and hands the ME_COMM_ID_BYTES bytes to the other
 *    ranks (any side channel: a torch.distributed store, a file, MPI); every
 *    rank then creates its communicator on its ctx device (collective call).
 *    All-reduces are enqueued on the ctx stream: no host round trip.
 *  - me_comm_create_callback: a caller all-reduce (allreduce(dev_ptr, n, user)
 *    sums n doubles in place over the ranks, n < 0: max over |n|; it must be
 *    ordered on the ctx stream, e.g. host-staged gloo, or threads driving
 *    several contexts of one GPU).  Collective like the RCCL form: every
 *    rank creates its communicator concurrently.
 * Both creators calibrate the communicator (me_comm_calibrate): a few
 * all-reduces at the two exchange sizes of a sharded LM iteration, timed on
 * this rank, then the max over the ranks (one more exchange), so every rank
 * holds the same per-exchange costs and the landmark-count gate takes the
 * same decision everywhere (me_ba_shard_worthwhile_comm).
 * Per LM iteration the sharded solve exchanges twice: one sum of the packed
 * reduced camera system [S upper block triangle | b | diag(U) | camera
 * gradient | cost | failure count | per-rank gradient max-norm slots] after
 * the Schur pass, and one sum of the five step scalars after the point step;
 * the first linearisation also sums the Jacobi column norms.  Every rank
 * solves the camera system redundantly and steps its own landmarks. */
typedef int (*me_allreduce_fn)(double* dev_buf, int n, void* user);
typedef struct me_comm me_comm;
#define ME_COMM_ID_BYTES 128
enum { ME_COMM_SUM = 0, ME_COMM_MAX = 1 };
int me_comm_unique_id(void* id_out, int id_bytes);
int me_comm_create_rccl(me_ctx* ctx, int world, int rank, const void* id, me_comm** out);
int me_comm_create_callback(me_ctx* ctx, int world, int rank, me_allreduce_fn allreduce, void* user,
                            me_comm** out);
void me_comm_destroy(me_comm* comm);
int me_comm_info(const me_comm* comm, int* world, int* rank, int* native);
/* In-place all-reduce of n doubles of device memory on the ctx stream. */
int me_comm_allreduce(me_comm* comm, double* dev_buf, long n, int op);
/* Re-measures the communicator's exchange costs (collective: every rank
   calls it): `reps` timed all-reduces (after 3 untimed) of ME_COMM_CAL_SYSTEM
   doubles -- the packed reduced camera system of a 30-keyframe window -- and
   of 5 doubles (the step scalars), wall time per call including the stream
   synchronisation, max over the ranks.  The creators run it with reps = 10. */
#define ME_COMM_CAL_SYSTEM 17000
int me_comm_calibrate(me_comm* comm, int reps);
/* The calibrated costs (microseconds per exchange) of the system and the
   scalar exchange; 0 before any calibration. */
int me_comm_exchange_us(const me_comm* comm, double* system_us, double* scalars_us);
/* The gate below with this communicator's world and calibrated costs
   (xch_us = the mean of the two, so 2 * xch_us is one LM iteration's
   exchanges); uncalibrated: the built-in estimate.  Host only. */
int me_ba_shard_worthwhile_comm(const me_comm* comm, long n_obs);
int me_ba_solve_comm(me_ctx* ctx, me_ba_problem* p, const me_ba_options* o, me_comm* comm, me_ba_summary* s);
/* The same with a bare callback and no rank information (ABI v2 form): the
   gradient max-norm then travels in a separate max all-reduce. */
int me_ba_solve_sharded(me_ctx* ctx, me_ba_problem* p, const me_ba_options* o, me_allreduce_fn allreduce,
                        void* user, me_ba_summary* s);
/* Landmark-count gate of the sharded solve (shard "only when the
   landmark count warrants it").  Every rank solves the camera system
   redundantly, so sharding saves only landmark-kernel time (linearisation,
   Schur pass, point step) and costs two all-reduces per LM iteration.  Model
   per LM iteration: t(n) = max(ME_SHARD_FLOOR_US, n * ME_SHARD_OBS_NS / 1000)
   microseconds for n observations (fitted to the one-GPU shard timings of
   bench.py's sharded_ba.crossover_model); returns 1 when
   t(n_obs) - t(ceil(n_obs / world)) > 2 * xch_us, else 0 (world <= 1: 0).
   xch_us <= 0 takes the built-in per-exchange estimate for `world`
   (me_ba_shard_exchange_us, a fallback only: a communicator measures its
   own, me_comm_exchange_us).  Host only: no device, no ctx. */
#define ME_SHARD_OBS_NS 1.0
#define ME_SHARD_FLOOR_US 40.0
int me_ba_shard_worthwhile(long n_obs, int world, double xch_us);
double me_ba_shard_exchange_us(int world);

/* ---- A12: KLT feature tracking (build-defined; no reference) ----------
 * The position contract.  At pyramid level L (scale sc = 2^-L, exact) the
 * template window of feature p has the float32 origin xw = p.x * sc -
 * (win - 1) / 2, yw likewise, and lies inside the level iff
 *     xw >= 0 && xw < W_L - win && yw >= 0 && yw < H_L - win,
 * compared as floats, before anything is converted to an integer: the same
 * predicate as 0 <= floor(xw), floor(xw) + win < W_L for every position whose
 * floor fits an int, false for NaN and "outside" for +-inf and for positions
 * of any magnitude.  The search window of every iteration is tested the same
 * way.  A level whose template window is outside is skipped.  A feature whose
 * position is NaN or +-inf in either component, or whose template window is
 * outside at level 0, is never read from the images and gets status 0; its
 * pts_out is what the level loop leaves, per component: p * 2^-max_level
 * doubled max_level times when every level skipped it (p itself, bit for bit,
 * unless the scaling underflowed; NaN for a NaN input: compare with isnan, the
 * payload is not specified), otherwise where the upper levels' searches
 * arrived, scaled to level 0.  The other features of a call are unaffected.
 * me_klt_track_fb and the guided forms inherit the rule for pts_in; their own
 * extra inputs (the gate's start, the guess) are tested in float as well. */
typedef struct { int win; int max_level; int max_iters; double eps; double min_eig; } me_klt_params;
void me_klt_default_params(me_klt_params* p);
int me_klt_track(me_ctx* ctx, me_mem mem, const uint8_t* prev, const uint8_t* next, int width, int height,
                 int stride, const float* pts_in, float* pts_out, uint8_t* status, int n, const me_klt_params* p);

/* ---- A12c: forward-backward KLT check (build-defined; no reference) -----
 * me_klt_track prev -> next, then back next -> prev from where it arrived;
 * a feature is kept only if it returns to where it started.  With the same
 * me_klt_params for both passes:
 *  1. (q, sf) = me_klt_track(prev, next, pts_in); pts_out = q, bit for bit,
 *     for every feature (those with sf = 0 included).
 *  2. (r, sb) = me_klt_track(next, prev, q): the template and its Scharr
 *     derivatives come from the next pyramid at every level, the search runs
 *     in the prev pyramid and starts at q (no initial guess).
 *  3. dx = (double)r.x - (double)pts_in.x, dy likewise; d2 = dx * dx + dy * dy
 *     in FP64, in this order, no contraction.
 *  4. status = 1 iff sf == 1 && sb == 1 && d2 <= fb_max * fb_max, else 0.
 *  5. fb_err = (float)sqrt(d2) (correctly rounded FP64 sqrt, round-to-nearest
 *     cast) when sf == 1 && sb == 1, else +inf.  fb_err may be NULL.
 * The backward pass of a feature with sf = 0 is skipped.  Arguments are those
 * of me_klt_track plus fb_max > 0 (NaN, 0 and negative values are rejected;
 * +inf accepts every feature both passes tracked); n = 0 is allowed; ME_HOST /
 * ME_DEVICE as in me_klt_track (asynchronous on the ctx stream in device
 * mode).  The definition is restated in numpy around any tracker in
 * pipeline.klt_fb_host (the checker, with oracle/klt.cpp as the tracker). */
int me_klt_track_fb(me_ctx* ctx, me_mem mem, const uint8_t* prev, const uint8_t* next, int width, int height,
                    int stride, const float* pts_in, float* pts_out, uint8_t* status, float* fb_err /* n, may be NULL */,
                    int n, const me_klt_params* p, double fb_max);

/* ---- A12f: guided KLT, an initial guess per feature (build-defined; no
 * reference) -- OpenCV's OPTFLOW_USE_INITIAL_FLOW on this tracker.  `guess`
 * holds n x 2 floats, level-0 pixel positions in `next`, in host or device
 * memory as `mem` says.  With sc = 2^-L the scale of the top pyramid level
 * L = max_level:
 *  - feature i has a usable guess iff both components are finite and
 *    0 <= gx < width and 0 <= gy < height, compared as floats;
 *  - its start is s_i = usable ? guess_i : pts_in_i;
 *  - the search of the top level starts at s_i * sc (me_klt_track starts it at
 *    pts_in_i * sc; sc is a power of two, so the product is exact);
 *  - the template (taken at pts_in_i * sc), its window test, the
 *    minimum-eigenvalue test, every iteration, the step from level to level
 *    and the status rule are me_klt_track's, unchanged.
 * A feature without a usable guess therefore gets me_klt_track's result bit
 * for bit, and so does one whose guess equals pts_in.
 *
 * me_klt_track_guided_fb is the forward-backward check (A12c) with the same
 * prior applied in reverse:
 *  1. (q, sf) = me_klt_track_guided(prev, next, pts_in, guess); pts_out = q for
 *     every feature.
 *  2. In float32, per component: e = s - pts_in, then b = q - e (two roundings,
 *     in this order).  (r, sb) = me_klt_track_guided(next, prev, q, b): the
 *     template at q in the next pyramid, the search in the prev pyramid from b
 *     under the same usability rule (b unusable: from q).  The pass of a
 *     feature with sf = 0 is skipped, as in A12c.
 *  3.-5. are A12c's, against pts_in.
 * With no usable guess anywhere the call equals me_klt_track_fb bit for bit,
 * fb_err included.  Arguments are checked as in the plain calls; a NULL guess
 * is ME_ERR_INVALID; n = 0 is allowed.  Kernel time is booked under ME_KT_KLT.
 * The definition is restated in numpy in uasl_motion_estimation_amd/klt_ref.py
 * (the checker; without a guess it is oracle/klt.cpp bit for bit). */
int me_klt_track_guided(me_ctx* ctx, me_mem mem, const uint8_t* prev, const uint8_t* next, int width, int height,
                        int stride, const float* pts_in, const float* guess, float* pts_out, uint8_t* status, int n,
                        const me_klt_params* p);
int me_klt_track_guided_fb(me_ctx* ctx, me_mem mem, const uint8_t* prev, const uint8_t* next, int width, int height,
                           int stride, const float* pts_in, const float* guess, float* pts_out, uint8_t* status,
                           float* fb_err /* n, may be NULL */, int n, const me_klt_params* p, double fb_max);

/* ---- A12b: corner detector (build-defined; no reference) ---------------
 * Where the VO loop starts new tracks: the pixels that maximise the quantity
 * the KLT tests before it accepts a window (the minimum eigenvalue of the
 * structure tensor, klt.hip).  Response R(x, y), FP64, of an 8-bit image for
 * an odd window `win` (3 <= win <= 31), half = (win - 1) / 2: dx, dy = the
 * KLT's level-0 Scharr derivatives (3/10/3, reflect-101); A11 = sum dx^2,
 * A12 = sum dx dy, A22 = sum dy^2 over the win x win pixels centred on
 * (x, y), exact integers; a = (double)A * 2^-20;
 *   R = (a22 + a11 - sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / (2.0 * win * win)
 * where the KLT would accept the window at level 0 (x - half >= 0,
 * y - half >= 0, x - half + win < width, y - half + win < height), else 0.0:
 * at an integer position R is the KLT's own minEig, bit for bit.  Pixel p is
 * a corner iff R(p) >= min_eig (> 0) and p beats its (up to) 8 neighbours
 * inside the image in the total order "larger R first, then smaller
 * row-major index y * width + x".  The definition is restated in numpy in
 * uasl_motion_estimation_amd/corners.py (the checker). */
typedef struct { int win; double min_eig; } me_corner_params;
void me_corner_default_params(me_corner_params* p);              /* 21, 1e-4 */
/* The response map (height x width doubles, row-major, no padding). */
int me_corner_response(me_ctx* ctx, me_mem mem, const uint8_t* img, int width, int height, int stride,
                       const me_corner_params* p, double* response);
/* New features of a keyframe from the corners of img: the grid and the good
   tracked features are those of me_vo_new_cells; a corner at integer (x, y)
   with margin <= x < width - margin, margin <= y < height - margin (compared
   as floats) belongs to the cell the same formula gives for (x, y); each cell
   keeps its best corner in the order above; the first max(0, n_feats - #good)
   cells in ascending order that are unoccupied and hold a corner emit
   ((float)x, (float)y), lo = d_min; *out_count = their number.  n = 0 with
   NULL uv / status / ok is allowed (the first keyframe).  Device memory,
   asynchronous on the ctx stream, like me_vo_new_cells. */
int me_vo_new_corners(me_ctx* ctx, const uint8_t* img, int width, int height, int stride, const float* uv,
                      const uint8_t* status, const uint8_t* ok, int n, float margin, int nx, int ny, double cw,
                      double ch, int n_feats, int d_min, const me_corner_params* p, float* out_uv, int32_t* out_lo,
                      int32_t* out_count);

/* ---- A12d: stereo rectification (build-defined; no reference) ------------
 * The reference assumes undistorted, row-aligned images of one size and one K
 * and leaves rectification to the caller.  Two primitives: me_rectify_map
 * builds a fixed-point map from a camera model, me_remap_q5 warps an 8-bit
 * image through any such map.  The numpy restatement is
 * uasl_motion_estimation_amd/rectify.py (rectify_map_ref, remap_ref), the
 * checker; both results are bit-exact.
 *
 * me_camera_model: the raw image size, fx fy cx cy, dist = {k1, k2, p1, p2, k3}
 * (Brown-Conrady) and R (row-major), the rotation from raw-camera to
 * rectified-camera coordinates (the R1 / R2 of a stereo calibration), used as
 * given and not re-orthonormalised.  me_rectified_model: the rectified size
 * and fx fy cx cy, shared by both cameras (the VO loop's K, width, height).
 *
 * Map: int32 map[height][width][2], the source coordinates in 1/32 pixel (Q5)
 * of the rectified pixel at integer (u, v).  FP64, every operation rounded
 * once, evaluated in the order written, never contracted; divisions are
 * correctly rounded:
 *   x  = (u - cx_r) / fx_r            y = (v - cy_r) / fy_r
 *   X  = (R[0]*x + R[3]*y) + R[6]     Y = (R[1]*x + R[4]*y) + R[7]
 *   W  = (R[2]*x + R[5]*y) + R[8]                               (R transposed)
 *   a  = X / W                        b = Y / W
 *   a2 = a*a    b2 = b*b    r2 = a2 + b2    tab = 2.0*(a*b)
 *   rad = 1.0 + r2*(k1 + r2*(k2 + r2*k3))
 *   xd = (a*rad + p1*tab) + p2*(r2 + 2.0*a2)
 *   yd = (b*rad + p1*(r2 + 2.0*b2)) + p2*tab
 *   us = fx*xd + cx                   vs = fy*yd + cy
 * The entry is the sentinel {INT32_MIN, INT32_MIN} ("no source") unless W > 0,
 * fabs(us) < 2^24 and fabs(vs) < 2^24 (all three false for NaN); otherwise
 * {(int32)rint(us*32.0), (int32)rint(vs*32.0)}, rint to nearest-even.
 *
 * Remap of an 8-bit source (src_w, src_h, src_stride) through a Q5 map of
 * dst_w x dst_h: for the entry {iu, iv}, sx = iu >> 5 (arithmetic shift:
 * floor), fxq = iu & 31, sy and fyq likewise; taps (sx, sy), (sx+1, sy),
 * (sx, sy+1), (sx+1, sy+1); a tap outside [0, src_w) x [0, src_h) has the
 * value `border` (0..255), each tap judged on its own;
 *   dst = (p00*(32-fxq)*(32-fyq) + p10*fxq*(32-fyq) + p01*(32-fxq)*fyq
 *          + p11*fxq*fyq + 512) >> 10.
 * A sentinel entry gives `border` (all four of its taps lie outside any
 * image).  Exact integer arithmetic: nothing depends on scheduling.  Bytes of
 * a row past its width (stride padding) are never read as pixels nor written.
 *
 * Arguments: non-finite model parameters, fx or fy <= 0, a size below 1,
 * border outside 0..255 and a stride below its width are ME_ERR_INVALID with
 * a message that names the argument; 1 x 1 images are legal on both sides;
 * width * height < 2^31 on every side.  ME_HOST: every pointer is host memory
 * and the call is synchronous; ME_DEVICE: every pointer is device memory (the
 * map 8-byte aligned) and the call is asynchronous on the ctx stream.  Both
 * are timed in the ME_KT_RECTIFY family. */
typedef struct me_camera_model {
  int width, height;          /* raw image */
  double fx, fy, cx, cy;
  double dist[5];             /* k1, k2, p1, p2, k3 */
  double R[9];                /* raw camera -> rectified camera, row-major */
} me_camera_model;
typedef struct {
  int width, height;
  double fx, fy, cx, cy;
} me_rectified_model;
int me_rectify_map(me_ctx* ctx, me_mem mem, const me_camera_model* cam, const me_rectified_model* rect,
                   int32_t* map /* rect->height * rect->width * 2 */);
/* me_remap_q5 works on tiles of *tw x *th destination pixels (row-major tile
   order, ceil(dst_w / tw) tiles per row), one workgroup each.  A tile takes
   one of two paths, chosen from the map's content alone: the bounding box of
   the taps of its entries that touch the image (taps clamped to [-1, src_w] x
   [-1, src_h]; x0 .. x1, y0 .. y1) is staged in LDS as
   rows = y1 - y0 + 1 rows of words = (x1 >> 2) - (x0 >> 2) + 1 aligned groups
   of four pixels with a row stride of (words + 1) | 1 words -- path 0 -- iff
   rows * ((words + 1) | 1) <= *stage_words (arithmetic shifts); otherwise
   every pixel of the tile reads its taps from global memory -- path 1.  A
   tile none of whose entries touches the image is path 0.  stage_words may be
   NULL. */
int me_remap_tile_dims(int* tw, int* th, int* stage_words);
/* tile_path (may be NULL): one byte per tile, the path it took (0 staged,
   1 global).  The output does not depend on the path. */
int me_remap_q5(me_ctx* ctx, me_mem mem, const uint8_t* src, int src_w, int src_h, int src_stride,
                const int32_t* map, int dst_w, int dst_h, int border, uint8_t* dst, int dst_stride,
                uint8_t* tile_path);

/* ---- A12e: local contrast equalisation, CLAHE (build-defined; no reference)
 * A thermal camera's image is low in contrast and steps in level with the
 * sensor's gain control; the KLT and the corner detector threshold a minimum
 * eigenvalue and starve on it.  me_clahe is a contrast-limited adaptive
 * histogram equalisation of an 8-bit image.  The definition is build-defined
 * and integer-only: OpenCV's float CLAHE is NOT restated and parity with it is
 * unpinned.  The numpy restatement is uasl_motion_estimation_amd/equalise.py
 * (clahe_ref), the checker; image and tables are bit-exact.
 *
 * Tiling: tw = ceil(width / tiles_x), th = ceil(height / tiles_y),
 * area = tw * th.  The image is extended to tw*tiles_x x th*tiles_y on the
 * right and bottom by reflect-101 (index i >= width reads 2*(width-1) - i);
 * tile (j, i) covers rows [j*th, (j+1)*th) and columns [i*tw, (i+1)*tw) of
 * the extended image (a tile may lie wholly in the mirrored margin).
 *
 * Clip limit, once, on the host, in FP64: lim = area when clip_limit == 0,
 * else lim = min(area, max(1, floor(clip_limit * area / 256))).
 *
 * Per tile, in exact integers:
 *   1. hist = the 256-bin histogram;
 *   2. excess = sum(max(hist - lim, 0)), hist = min(hist, lim);
 *   3. hist += excess / 256 for every bin;
 *   4. r = excess % 256; if r > 0: step = max(256 / r, 1) and the bins
 *      0, step, 2*step, ... (the first r of them) get +1;
 *   5. c = the inclusive prefix sum of hist (c[255] == area);
 *   6. lut[v] = (255*c[v] + area/2) / area.
 *
 * Per pixel (x, y) of value v:
 *   ax = 2x + 1 - tw; i0 = floor_div(ax, 2tw); fx = ax - i0*2tw (in [0, 2tw));
 *   i1 = clamp(i0 + 1) from the unclamped i0, then i0 = clamp(i0), both to
 *   [0, tiles_x - 1]; the same in y gives j0, j1, fy;
 *   top = lut[j0][i0][v]*(2tw - fx) + lut[j0][i1][v]*fx, bot likewise with j1;
 *   dst = (top*(2th - fy) + bot*fy + 2*tw*th) / (4*tw*th).
 * Every quantity fits in unsigned 32 bits for area <= 2^20; nothing depends on
 * scheduling.  Bytes of a row past its width (stride padding) are never read
 * as pixels nor written.
 *
 * ME_ERR_INVALID, with a message that names the argument: NULL src / dst /
 * params; width or height < 1; a stride below the width; a stride with
 * stride * height >= 2^31; tiles_x outside
 * 1 .. min(width, 16), tiles_y outside 1 .. min(height, 16); clip_limit
 * negative or non-finite; area > 2^20.  dst == src with equal strides is
 * allowed (in place); any other overlap is the caller's error.
 * lut_out (may be NULL): the tiles_y * tiles_x tables of 256 bytes, row-major
 * in (j, i), so that a test can tell a wrong table from a wrong blend.
 * ME_HOST: every pointer is host memory, the call is staged in a scratch slot
 * of its own and synchronous; dst is returned row by row, so the caller's row
 * padding keeps its bytes.  ME_DEVICE: every pointer is device memory and the
 * call is asynchronous on the ctx stream.  Both kernels (table, apply; in that
 * order, one launch each) are timed in the ME_KT_CLAHE family. */
typedef struct me_clahe_params { int tiles_x, tiles_y; double clip_limit; } me_clahe_params;
void me_clahe_default_params(me_clahe_params* p);                 /* 8, 8, 3.0 */
int  me_clahe(me_ctx* ctx, me_mem mem, const uint8_t* src, int width, int height, int src_stride,
              const me_clahe_params* p, uint8_t* dst, int dst_stride,
              uint8_t* lut_out /* tiles_y*tiles_x*256 bytes, may be NULL */);
/* The apply kernel works on workgroups of 64 x (16 * rows) pixels, rows = 4 on
   images large enough to keep every compute unit of the ctx busy that way,
   else 1.  Returns the rows me_clahe uses for a width x height image on this
   ctx (1 or 4; the output does not depend on it), so that a test can place a
   case on either side; ME_ERR_INVALID (negative) for a NULL ctx or a size
   below 1. */
int  me_clahe_apply_rows(me_ctx* ctx, int width, int height);

/* ---- A12g: 16-bit ingest, 16 -> 8-bit tone mapping (build-defined; no
 * reference) ---------------------------------------------------------------
 * A thermal core delivers 14 or 16 bits per pixel and a scene often spans a
 * few hundred counts of them; keeping the high byte leaves a handful of
 * levels.  me_tonemap16 maps a percentile window of the 16-bit image linearly
 * to 0..255; the window follows the scene through a temporal filter whose
 * state lives on the device.  The definition is this library's own, integer
 * only: it restates no OpenCV function and parity is unpinned.  The numpy
 * restatement is uasl_motion_estimation_amd/tonemap.py (tonemap_ref), the
 * checker; image and state are bit-exact.
 *
 * Input: uint16 image, width x height, stride in elements; N = width*height.
 * State (per camera): three int32 words lo_q8, hi_q8, frames.
 *   1. frame window.  h = the histogram of the N pixels over 0..65535, c its
 *      inclusive prefix sum.  k_lo = floor(lo_ppm*N / 10^6), k_hi =
 *      floor(hi_ppm*N / 10^6) (64-bit products).  lo = the smallest v with
 *      c[v] > k_lo; hi = the smallest v with c[v] >= N - k_hi.  lo <= hi since
 *      lo_ppm + hi_ppm < 10^6.
 *   2. minimum span.  s = hi - lo; if s < min_span: lo -= (min_span - s) / 2
 *      (C division); if lo < 0: lo = 0; hi = lo + min_span; if hi > 65535:
 *      hi = 65535, lo = 65535 - min_span.
 *   3. temporal filter (int64 intermediates, floor division = arithmetic
 *      shift).  frames == 0: lo_q8 = lo << 8, hi_q8 = hi << 8.  Otherwise
 *      x_q8 += floor(((x << 8) - x_q8) * alpha_q8 / 256) for both words.
 *      frames += 1, saturating at INT32_MAX.  alpha_q8 = 256: no memory.
 *   4. window used.  lo_u = lo_q8 >> 8, hi_u = (hi_q8 + 255) >> 8,
 *      span = max(1, hi_u - lo_u).
 *   5. map.  v < lo_u: 0.  Otherwise q = (min(v, hi_u) - lo_u)*255 + span/2
 *      and out = min(255, q / span).  Every product is below 2^24.
 * Nothing depends on scheduling.  Elements of a row past its width (stride
 * padding) are never read as pixels nor written.
 *
 * The defaults (1000, 1000, 256, 64: 0.1 % clipped at either end, at least
 * 256 counts, a quarter of the way to the new window per frame) are a choice,
 * not a measurement.
 *
 * ME_ERR_INVALID, with a message that names the argument: NULL ctx / src /
 * dst / params; width or height < 1; src_stride or dst_stride below the
 * width; lo_ppm or hi_ppm < 0, or lo_ppm + hi_ppm >= 10^6; min_span outside
 * 1..65535; alpha_q8 outside 1..256; src_stride * height or dst_stride *
 * height >= 2^30; a src that is not 2-byte aligned; a state of another ctx.
 * state = NULL: stateless, as frames = 0 (nothing is kept).  A state is used
 * by one call at a time, in stream order.
 * ME_DEVICE: src / dst are device memory; the call is asynchronous on the ctx
 * stream and nothing is read back: the window goes from the select kernels to
 * the apply kernel through device memory.  ME_HOST: src / dst are host memory,
 * the call is staged in a scratch slot of its own and synchronous; dst is
 * returned row by row, so the caller's row padding keeps its bytes.  The state
 * is device memory in both modes.  Three kernels (coarse select, fine select,
 * apply; one launch each) are timed in the ME_KT_TONEMAP family. */
typedef struct me_tonemap_params { int lo_ppm, hi_ppm, min_span, alpha_q8; } me_tonemap_params;
typedef struct me_tonemap_state me_tonemap_state;
void me_tonemap_default_params(me_tonemap_params* p);             /* 1000, 1000, 256, 64 */
int  me_tonemap_state_create(me_ctx* ctx, me_tonemap_state** st);  /* frames = 0 */
int  me_tonemap_state_destroy(me_tonemap_state* st);
/* Asynchronous on the state's ctx stream: frames = 0 (the next call starts a new window). */
int  me_tonemap_state_reset(me_tonemap_state* st);
/* Synchronous: out = {lo_q8, hi_q8, frames}. */
int  me_tonemap_state_read(me_tonemap_state* st, int32_t out[3]);
int  me_tonemap16(me_ctx* ctx, me_mem mem, const uint16_t* src, int width, int height, int src_stride,
                  uint8_t* dst, int dst_stride, const me_tonemap_params* params,
                  me_tonemap_state* state /* NULL: stateless, as frames = 0 */);

/* ---- A12h: rigid-motion gate of the tracked features (build-defined; no
 * reference symbol -- the reference's geometric test is the RANSAC inside
 * StereoVisualOdometry::process, A19, which takes host arrays, draws with the
 * host's rand() and returns synchronously).  The loop's three tests of a track
 * (KLT status, stereo match, margin) are photometric; this one asks whether
 * the track moved the way a rigid scene moves under one camera motion.  It
 * estimates that motion from the tracked stereo observations and clears the
 * ok byte of every track that does not move with it.
 *
 * Integer and FP64 arithmetic only; the FP64 operations are + - * / sqrt,
 * never contracted, each expression evaluated as written below (left to
 * right, parentheses first).  The numpy restatement is
 * motion_gate.motion_gate_ref.
 *
 * Inputs per feature k = 0 .. n - 1: prev_uv (u0, v0) and prev_xr x0 of
 * keyframe t - 1, cur_uv (u1, v1) and cur_xr x1 of keyframe t (float), the
 * status and ok bytes.  Scalars: f, cx, cy, baseline, the image size, margin,
 * the keyframe number t and the parameters.  fb = f * baseline,
 * g2 = gate_max * gate_max.
 *  1. good_k iff status_k == 1 && ok_k != 0 && u1 >= margin &&
 *     u1 < (float)width - margin && v1 >= margin && v1 < (float)height - margin
 *     (float comparisons: me_vo_new_cells' good).
 *  2. usable_k iff good_k && d0 >= min_disp && d1 >= min_disp with
 *     d0 = (double)u0 - (double)x0, d1 = (double)u1 - (double)x1.
 *  3. triangulation of a usable feature, P from keyframe t - 1 and Q from t:
 *     Z = fb / d, x = ((double)u - cx) * Z / f, y = ((double)v - cy) * Z / f.
 *  4. sampling: hypothesis h = 0 .. n_hyp - 1 fills slots s = 0, 1, 2; attempt
 *     a = 0 .. 7 of slot s draws i = (mix(key) * n) >> 32 (64-bit product) with
 *     key = t * 0x9E3779B1 + h * 0x85EBCA77 + (8 s + a) * 0xC2B2AE3D + seed
 *     (uint32, wrapping) and mix = lowbias32: x ^= x >> 16; x *= 0x7FEB352D;
 *     x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16.  The slot takes the first i
 *     that is usable and in no earlier slot; a slot without one voids h.
 *  5. hypothesis: with (a, b) = (P_1 - P_0, P_2 - P_0): aa = a.a, bb = b.b,
 *     c = a x b, cc = c.c; h is void unless cc > (1e-6 * aa) * bb;
 *     e1 = a / sqrt(aa), e3 = c / sqrt(cc), e2 = e3 x e1.  The same from Q gives
 *     f1, f2, f3 (void likewise).  x . y = (x0 y0 + x1 y1) + x2 y2 and
 *     x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0) everywhere.
 *     R_ij = (f1_i e1_j + f2_i e2_j) + f3_i e3_j,
 *     t_i = Q_0i - ((R_i0 P_00 + R_i1 P_01) + R_i2 P_02).
 *  6. residual of a usable feature under (R, t):
 *     Y_i = ((R_i0 P_0 + R_i1 P_1) + R_i2 P_2) + t_i; uh = f * Y_0 / Y_2 + cx,
 *     vh = f * Y_1 / Y_2 + cy, xh = uh - fb / Y_2; r = (uh - u1, vh - v1,
 *     xh - x1) against the observations as doubles; e2 = (r0 r0 + r1 r1) + r2 r2.
 *     inlier iff Y_2 > 0 && e2 <= g2.
 *  7. score: the number of inliers of a hypothesis that is not void; the
 *     winner is the first maximum.  No hypothesis: the gate abstains (9).
 *  8. refine: `refine` times, on the inliers of the current pose:
 *     a = f / Y_2, q = Y_2 * Y_2, g_0 = (a, 0, -(f * Y_0) / q),
 *     g_1 = (0, a, -(f * Y_1) / q), g_2 = (a, 0, (fb - f * Y_0) / q); Jacobian
 *     row m = (Y x g_m, g_m) (left perturbation dY = w x Y + dt).  The 27 sums
 *     H_ij = (J_0i J_0j + J_1i J_1j) + J_2i J_2j (i <= j, row-major) and
 *     b_i = (J_0i r_0 + J_1i r_1) + J_2i r_2 are taken in this order: a partial
 *     per chunk of 64 consecutive feature indices, started at +0.0 and adding
 *     the 64 slots' terms in index order (a slot without an inlier adds +0.0),
 *     then the partials in chunk order, started at +0.0.  H d = -b by a
 *     textbook Cholesky (column by column; L_jj = sqrt(H_jj - sum_k L_jk^2),
 *     L_ij = (H_ij - sum_k L_ik L_jk) / L_jj, subtractions in ascending k;
 *     forward and back substitution likewise, ascending k); a pivot that is
 *     not > 0 ends the refinement and keeps the pose.  d = (w, dt);
 *     c = 0.5 * w, cc = c.c, C = ((1 - cc) I + 2 c c^T + 2 [c]x) / (1 + cc)
 *     entry by entry ((1 - cc) + 2.0 * (c_i * c_i)) / (1 + cc) on the diagonal,
 *     (2.0 * (c_i * c_j) +- 2.0 * c_k) / (1 + cc) off it; R <- C R and
 *     t <- C t + dt with step 6's association.  No sin or cos anywhere.
 *  9. output: the final pose's inliers are counted.  Fewer than min_inliers
 *     (or no hypothesis): the gate abstains, ok_out = ok_in byte for byte.
 *     Else ok_out_k = 0 for a usable feature that is no inlier and the ok_in
 *     byte for every other feature: a feature that is not usable is never
 *     rejected.  ok_out may be ok_in.  err_out (n floats, may be NULL) =
 *     (float)sqrt(e2) under the final pose for usable features with Y_2 > 0,
 *     +inf for the others and when there is no pose.  info (128 bytes, 8-byte
 *     aligned, may be NULL): int32 n_usable, hypotheses not void, winner (-1:
 *     none), final inliers, abstained (0 / 1), three zero words, then R
 *     (row-major) and t as 12 doubles (zeros without a pose).
 * The defaults (2.0, 0.5, 256, 3, 10, 0) come from a prototype on synthetic
 * tracks, not from real data.  Parameter errors (gate_max, min_disp not finite
 * or <= 0, n_hyp outside 1 .. 1024, refine outside 0 .. 8, min_inliers < 3),
 * n < 0 or n > 2^24, a null array with n > 0, f or baseline not finite or <= 0,
 * t < 0 are ME_ERR_INVALID; n = 0 is allowed (info alone is written).  Device memory,
 * asynchronous on the ctx stream, three launches (the triangulations; a
 * workgroup per hypothesis; one workgroup for steps 7 - 9), timed in the
 * ME_KT_GATE family. */
typedef struct me_motion_gate_params {
  double gate_max, min_disp;
  int n_hyp, refine, min_inliers;
  uint32_t seed;
} me_motion_gate_params;
void me_motion_gate_default_params(me_motion_gate_params* p);
int  me_motion_gate(me_ctx* ctx, const float* prev_uv, const float* prev_xr, const float* cur_uv, const float* cur_xr,
                    const uint8_t* status, const uint8_t* ok_in, int n, double f, double cx, double cy,
                    double baseline, int width, int height, float margin, int t, const me_motion_gate_params* params,
                    uint8_t* ok_out, float* err_out /* may be NULL */, void* info /* may be NULL */);

/* ---- A12i: keyframe selection between the loop's keyframes (build-defined;
 * no reference symbol -- the reference's application, which would choose its
 * keyframes, is absent).  The caller owns the state of the n features seeded
 * at the last keyframe, all in device memory: ref_uv (n x 2 float, the
 * keyframe's positions, read only), cur_uv (n x 2 float, the carried
 * positions) and alive (n bytes), the last two updated in place.  One call per
 * frame pushed since that keyframe folds one tracker result into it -- new_uv
 * (n x 2 float) and status (n bytes) of a tracker call from the previous
 * pushed frame to this one started at cur_uv -- and takes the keyframe
 * decision.  gap is the number of frames pushed since the keyframe, this one
 * included.
 *
 * Exact integers and FP64; every FP64 operation is rounded once in the order
 * written and never contracted.  The numpy restatement is
 * keyframe.kf_update_ref.  For each feature k, with (u, v) = new_uv_k:
 *  1. a_k iff alive_k != 0 && status_k == 1 && isfinite(u) && isfinite(v) &&
 *     u >= margin && u < (float)width - margin && v >= margin &&
 *     v < (float)height - margin (float comparisons: the rule of the matcher's
 *     status gate and of me_vo_new_cells' good).
 *  2. if a_k: cur_uv_k = new_uv_k; otherwise cur_uv_k keeps its bits.
 *     alive_k = a_k (0 or 1).
 *  3. if a_k: dx = (double)cur_u - (double)ref_u, dy likewise with v,
 *     d2_k = (dx * dx) + (dy * dy).
 * Over all features: m = the number of a_k; med2 = the element of rank
 * (m - 1) >> 1 of the alive d2_k in ascending order (the lower median), 0.0
 * when m == 0.  flags: bit 0 ("few") iff 100 * (int64)m <
 * (int64)min_tracked_pct * n, or n == 0; bit 1 ("parallax") iff thr2 > 0 &&
 * med2 >= thr2, with thr2 = min_parallax * min_parallax formed once in FP64 on
 * the host (min_parallax = 0 switches the rule off, as 0 does the loop's other bounds);
 * bit 2 ("gap") iff gap >= max_gap.  The frame is a keyframe iff flags != 0.
 * info (32 bytes, 8-byte aligned, device memory): int32 n, m, rank
 * ((m - 1) >> 1: -1 when m == 0), flags; double med2; 8 zero bytes.
 * ref_uv is expected finite (a d2 that is NaN has no defined place in the
 * order).  Parameter errors (min_parallax not finite or < 0, min_tracked_pct
 * outside 0 .. 100, max_gap < 1), gap < 1, n < 0, a null array with n > 0 and
 * a null info are ME_ERR_INVALID; n = 0 is allowed.  The defaults are 12.0,
 * 60, 10.  Asynchronous on the ctx stream, one launch of one workgroup for
 * any n (the threads stride): the median is a radix select over the 64-bit
 * patterns of the d2 (monotone as unsigned integers), eight passes of 256-bin
 * LDS histograms; timed in the ME_KT_KEYFRAME family. */
typedef struct me_kf_params {
  double min_parallax;  /* pixels: a keyframe once the median displacement from the last keyframe reaches it */
  int min_tracked_pct;  /* a keyframe once fewer than this share (percent) of the seeded features is alive */
  int max_gap;          /* a keyframe at the latest this many frames after the last one */
} me_kf_params;
void me_kf_default_params(me_kf_params* p);
int  me_kf_update(me_ctx* ctx, const float* ref_uv, float* cur_uv, uint8_t* alive, const float* new_uv,
                  const uint8_t* status, int n, int width, int height, float margin, int gap,
                  const me_kf_params* params, void* info);

/* ---- A12j: frame pose, a pose-only refinement of every pushed frame
 * (build-defined; no reference symbol).  The rigid motion (R, t) that takes
 * points from the last keyframe's left-camera frame into the current frame's
 * (Y = R P + t), from the keyframe's stereo observations ref_uv (n x 2 float)
 * and ref_xr (n float) and the current frame's left-image positions cur_uv
 * (n x 2 float) with their alive bytes: the state me_kf_update carries, plus
 * the keyframe's x_r.  No RANSAC: an iteratively reweighted (Huber)
 * Gauss-Newton from a start pose, then an inlier count.
 *
 * A12h's rules: integer and FP64 + - * / sqrt only, never contracted, every
 * expression evaluated as written; frame_pose.frame_pose_ref restates this in
 * numpy and reproduces every output bit for bit.  Per feature k with
 * (u0, v0) = ref_uv_k, x0 = ref_xr_k, (u1, v1) = cur_uv_k:
 *  1. usable_k iff alive_k != 0 && isfinite(u1) && isfinite(v1) &&
 *     d0 >= min_disp with d0 = (double)u0 - (double)x0.
 *  2. P_k as A12h step 3: fb = f * baseline, Z = fb / d0,
 *     x = ((double)u0 - cx) * Z / f, y = ((double)v0 - cy) * Z / f.
 *  3. start pose: `start` non-NULL points at an info block of this call; its
 *     R, t are taken iff its valid word is 1.  Otherwise identity and zero.
 *     start == info is allowed: the block is read before it is written.
 *  4. the step, `iters` times, skipped altogether when fewer than 3 features
 *     are usable.  Under the current pose Y as A12h step 6,
 *     uh = f * Y_0 / Y_2 + cx, vh = f * Y_1 / Y_2 + cy,
 *     r = (uh - (double)u1, vh - (double)v1), e2 = r0 r0 + r1 r1;
 *     act_k iff usable_k && Y_2 > 0.  e = sqrt(e2); w = 1.0 if e <= huber,
 *     else huber / e.  g_0, g_1 and the Jacobian rows J_m = (Y x g_m, g_m),
 *     m = 0, 1, exactly as A12h step 8 (no third row).
 *     H_ij = w * (J_0i J_0j + J_1i J_1j) for i <= j, row-major, and
 *     b_i = w * (J_0i r_0 + J_1i r_1).  The 27 sums in A12h's order: a partial
 *     per chunk of 64 consecutive feature indices, from +0.0, in index order (a
 *     slot that is not act adds +0.0), then the partials in chunk order, from
 *     +0.0.  H d = -b by the same Cholesky; a pivot that is not > 0 ends the
 *     iterations and keeps the pose (NaN lands here too).  The same Cayley
 *     update R <- C R, t <- C t + dt.  steps counts the completed updates.
 *  5. final pass under the final pose: act and e2 as in 4,
 *     g2 = gate_max * gate_max, inlier iff act && e2 <= g2.
 *     valid = 1 iff steps == iters && n_inliers >= min_inliers.
 *     err_out_k (n floats, may be NULL) = (float)sqrt(e2) for act features,
 *     +inf otherwise.
 *  6. info (128 bytes, 8-byte aligned): int32 n_usable, n_act (final pass),
 *     n_inliers, steps, valid, three zero words, then R (row-major) and t as 12
 *     doubles: the final estimate whether valid or not, the start pose when no
 *     step ran.
 * The defaults (1.0, 2.0, 0.5, 6, 6) come from a prototype on synthetic
 * points, not from real data.  A parameter outside its range or not finite
 * (huber, gate_max, min_disp finite and > 0; iters 0 .. 16; min_inliers >= 3),
 * f or baseline not finite or <= 0, cx or cy not finite, n < 0 or n > 2^24, a
 * null array with n > 0 and a null info are ME_ERR_INVALID; n = 0 is allowed
 * (info alone is written, valid = 0).  Device memory, asynchronous on the ctx
 * stream; timed in the ME_KT_FRAMEPOSE family.  Launches: see csrc/frame_pose.hip. */
typedef struct me_frame_pose_params {
  double huber, gate_max, min_disp;   /* pixels; all finite and > 0 */
  int iters, min_inliers;             /* 0 .. 16; >= 3 */
} me_frame_pose_params;
void me_frame_pose_default_params(me_frame_pose_params* p);
int  me_frame_pose(me_ctx* ctx, const float* ref_uv, const float* ref_xr, const float* cur_uv,
                   const uint8_t* alive, int n, double f, double cx, double cy, double baseline,
                   const me_frame_pose_params* params, const void* start /* may be NULL */,
                   float* err_out /* may be NULL */, void* info /* 128 bytes, 8-aligned */);

/* ---- A11: non-maximum suppression ------------------------------------
 * Replaces std::vector<pt2D> me::nonMaxSupScanline3x3(const cv::Mat& input,
 * cv::Mat& output) (include/MotionEstimation/core/feature_types.h:270,
 * src/core/feature_types.cpp:253-351): response is CV_64F (h x w doubles),
 * mask_out h*w bytes (255 = maximum), maxima 2*cap doubles (row-major scan
 * order, (row+0.5+dr, col+0.5+dc)). */
int me_nms_scanline3x3(me_ctx* ctx, me_mem mem, const double* response, int width, int height, uint8_t* mask_out,
                       double* maxima, int cap, int* n_out);

/* ---- A19 / §8f-1: frame-to-frame stereo VO ---------------------------
 * Replaces bool me::StereoVisualOdometry::process(const std::vector<StereoOdoMatchesf>&,
 * cv::Mat init) (include/MotionEstimation/vo/StereoVisualOdometry.h:41,
 * src/vo/StereoVisualOdometry.cpp:34-92) with getMotion() (:331-342) and
 * getInliers_idx() (.h:47).  Parameters are StereoVisualOdometry::parameters
 * (StereoVisualOdometry.h:24-33 + VisualOdometry.h:19-33).  matches: n x 8
 * floats {f1.x, f1.y, f2.x, f2.y, f3.x, f3.y, f4.x, f4.y} (StereoOdoMatchesf:
 * previous left/right, current left/right).  The RANSAC triples come from
 * the context's glibc-compatible rand() stream (unseeded: as the
 * reference's rand(), reseed with me_vo_srand).  The reference's GN/LM loop
 * can run forever (StereoVisualOdometry.cpp:277); such a run is cut at
 * max_outer passes and reported as ME_ERR_STATE.  ok = process()'s result;
 * motion = getMotion() (4x4 row-major); state = the 6 state values
 * (Euler angles, translation); pts3d = getPts3D() (n x 4 homogeneous,
 * filled when n >= 6); inliers = getInliers_idx() (capacity n).  Any of
 * state, pts3d and inliers may be NULL. */
typedef struct {
  int method;                /* VisualOdometry::Method: 0 GN, 1 LM */
  double step_size, eps, e1, e2, e3, e4;
  int max_iter, nb_fixed_frames, ransac, n_ransac;
  double inlier_threshold;
  double baseline;
  int weighting;
  double fu1, fv1, fu2, fv2, cu1, cu2, cv1, cv2;
} me_vo_params;
void me_vo_default_params(me_vo_params* p);
int me_vo_srand(me_ctx* ctx, unsigned seed);
int me_vo_rand(me_ctx* ctx, int* out);  /* one draw of the context's rand() stream (tests) */
int me_vo_process(me_ctx* ctx, const float* matches, int n, const double* init6, const me_vo_params* p,
                  int max_outer, double* motion, double* state, double* pts3d, int* inliers, int* n_inliers,
                  int* ok);

/* ---- §8f-4: monocular VO -----------------------------------------------
 * Replaces bool me::MonoVisualOdometry::process(const std::vector<StereoMatch<
 * cv::Point2f>>&) (src/vo/MonoVisualOdometry.cpp:7-73) with getMotion(),
 * getEssentialMat(), getInliersIdx() (MonoVisualOdometry.h:35-41).  The
 * reference's OpenCV findEssentialMat (five-point + RANSAC at prob, or LMedS
 * when ransac = 0; threshold <= 0 -> 1 px) and recoverPose (distance 500) are
 * restated on the device (csrc/mono.hip; parity unpinned: OpenCV absent).
 * f1, f2: n (x, y) floats (StereoMatch f1 / f2; a match with f1.x <= 0 or
 * f2.x <= 0 is skipped as in the reference).  ok = process()'s result; Rt =
 * getMotion() (4x4 row-major, identity when ok = 0); E = getEssentialMat()
 * (3x3, zero when none; may be NULL); inliers = getInliersIdx() (indices into
 * the matches, capacity n; may be NULL). */
typedef struct {
  double fu, fv, cu, cv;     /* MonoVisualOdometry::parameters (MonoVisualOdometry.h:21-28) */
  double prob;               /* 0.99 */
  double inlier_threshold;   /* VisualOdometry::parameters: 2.0 */
  int ransac;                /* 1: RANSAC, 0: LMedS */
} me_mono_params;
void me_mono_default_params(me_mono_params* p);
int me_mono_vo_process(me_ctx* ctx, const float* f1, const float* f2, int n, const me_mono_params* p, double* Rt,
                       double* E, int32_t* inliers, int* n_inliers, int* ok);

#ifdef __cplusplus
}
#endif
#endif /* ME_HIP_H */
