// ba.hip — windowed stereo bundle adjustment on MI355X.
// Kernel map in ba_types.hpp; the kernels in the ba_*.hpp parts included
// below, one per stage.  Host side: problem upload + CSR build, the
// per-iteration launch sequence (LM control lives on the device: every kernel
// reads the State flags, so a whole solve can be enqueued — or captured in a
// hipGraph — without host round trips), and the landmark-sharded variant with
// a caller-provided all-reduce.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>
#include <hip/hip_ext.h>
#include "me_internal.hpp"
#include "ba_types.hpp"
#include "ba_reduce.hpp"
#include "ba_residual.hpp"
#include "ba_linearize.hpp"
#include "ba_schur.hpp"
#include "ba_assemble.hpp"
#include "ba_cam_solve.hpp"
#include "ba_step.hpp"
#include "ba_eval.hpp"
#include "ba_cov.hpp"
#include "ba_plan.hpp"
#include "ba_vo_chain.hpp"

using namespace ba;

namespace {

constexpr int kPtBlock = 64;   // per-point kernels: spread ~N/64 workgroups over the CUs

// The kernels whose dynamic LDS takes a raised ceiling (plan_build sets it once
// per context): the camera solve's three forms and every Schur instance.
const void* const kSolveKernels[] = {(const void*)cam_solve_kernel<0>, (const void*)cam_solve_kernel<1>,
                                     (const void*)cam_solve_kernel<2>};

// Every pt_schur_kernel instance, once: model (obs_dim) x tiles per wave x
// landmarks per sub-chunk.  NT = the wave's tile count, instantiated tight: an
// unused tile's accumulator costs 8 VGPRs, and at 512 threads (2 waves per
// SIMD) the budget is 256 registers -- up to 5 tiles nothing spills (9 tiles
// spilled 120 B); wider windows take more tile groups per run instead.
using SchurKernel = void (*)(Geo, Bufs, Opts, CamArgs);
struct SchurInstance {
  int od, nt, pts;
  SchurKernel kernel;
};
#define ME_SCHUR_I(D, N, PTS) {D, N, PTS, pt_schur_kernel<D, N, 512, PTS>}
#define ME_SCHUR_K(D, N) ME_SCHUR_I(D, N, kSchurPts), ME_SCHUR_I(D, N, kSchurPtsWide), ME_SCHUR_I(D, N, kSchurPtsSmall)
constexpr SchurInstance kSchurInstances[] = {ME_SCHUR_K(4, 2), ME_SCHUR_K(4, 3), ME_SCHUR_K(4, 4), ME_SCHUR_K(4, 5),
                                             ME_SCHUR_K(2, 2), ME_SCHUR_K(2, 3), ME_SCHUR_K(2, 4), ME_SCHUR_K(2, 5)};
#undef ME_SCHUR_K
#undef ME_SCHUR_I
static_assert(kSchurNtMax >= 3 && kSchurNtMax <= 5, "instantiated tile counts");
static_assert(schur_nt(16) == 2 && schur_nt(24) == 3 && schur_nt(32) == 4 && schur_nt(40) == 5, "schur_nt is this dispatch");
// the instance of a plan's geometry (ba_geometry: od 4 | 2, spts one of the three)
SchurKernel schur_instance(const Geo& g) {
  for (const SchurInstance& i : kSchurInstances)
    if (i.od == g.od && i.nt == schur_nt(g.stpw) && i.pts == g.spts) return i.kernel;
  return nullptr;
}

// ---------------------------------------------------------------- host plan
struct Plan {
  me_ctx* c = nullptr;
  Geo g;
  unsigned asm_gen = 0;  // fused-assembly launches since the plan cleared the claim words
  Bufs b;
  Opts o;
  double* colnorm = nullptr;
  double* gc_raw = nullptr;
  double* Uraw = nullptr;
  double* cpart = nullptr;  // camera assembly partials (27 per unit)
  double* host = nullptr;  // pinned staging (inputs in, State / results out)
  State* hstate[2] = {nullptr, nullptr};  // pinned slots of the pipelined State polls
  bool dev = false;        // problem arrays are device-resident
  bool copy_out = false;   // device-resident problem: the solved cams / pts also staged to the host (me_ba_wait_out)
  bool reserve_only = false;  // me_ba_reserve: size the scratch and staging, queue nothing
  size_t solve_lds = 0;
  size_t schur_lds = 0;
  int use_lds = 0;
  int solve_flags = 0;  // cam_solve_kernel `flags`: the ctx's test-hook bits the kernel reads (kFlag*)
  int n_enq = 0;      // linearisations queued so far (the first runs the camera assembly on its own)
  bool no_fused_asm = false;  // test hook kFlagSeparateAsm: S assembly in its own launch
  SchurKernel schur = nullptr;  // the pt_schur_kernel instance of this geometry (schur_instance)
  bool fused_lin = false;   // the plan's Schur instance linearises in its phase A: no linearize_kernel launch, no obsx
  bool full_S = false;      // assemble both block triangles of S (reduced-system / covariance read-back)
  size_t cov_off = 0;       // asynchronous plans: where the staging holds a covariance queued behind the solve (doubles)
  bool cov = false;         // me_ba_covariance_full: a device-resident problem's plan queues behind the asynchronous
                            // solves (no drain) and takes no host staging
  size_t check_off = 0;     // asynchronous plans: where the staging holds the flags of a residual check queued behind
                            // the solve (bytes; behind the covariance's part)
  int solve_cap = 0;        // co-resident cam_solve_kernel<2> workgroups on the ctx's CUs (0: not queried)
  me_comm* comm = nullptr;  // sharded solve: the exchange (null: one GPU)
  bool xmax_separate = false;  // ABI-v2 callback (no rank): the gradient max-norm travels in its own max all-reduce
};

inline long rup(long x, long m) { return (x + m - 1) / m * m; }
int blocks(long n, int bs) { return (int)std::max(1L, (n + bs - 1) / bs); }

// Geometry of the Schur pass (pt_schur_kernel) from the tile pairs, the
// landmarks and the padded row length; me_debug_ba_geometry and
// tests/test_host.py pin what it chooses.  The landmarks are cut into
// sub-chunks of spts, rsub sub-chunks make a run (at most ~256 runs), and a
// run's tiles are dealt to sgrp tile groups of stpw = 8 waves x NT <= 5 tiles;
// the grid is runs, in blocks of 8 (one per XCD) when a run has several
// groups, x sgrp (surplus groups and padding runs exit at once).
//  * spts: 32 whenever the Y block of 32 landmarks fits the LDS (Rpad <= 192):
//    half the partial tiles for the assembly to sum (config 4: -2% BA time;
//    the config-3 VO window of ~4 400 landmarks, where 16-landmark sub-chunks
//    outnumber 256 workgroups: BA_SCHUR 430 -> 340 us per keyframe).  Else 16,
//    or 8 beyond 100 pairs: the contraction is MFMA-bound per workgroup and
//    twice the workgroups spread it over more CUs (config 5: BA 5.2 -> 4.96 ms
//    per 10 iterations; config 3 is slower with 8).
//  * NT: 4 tiles per wave up to 100 pairs (config 4: 5 spill), 5 beyond (the
//    50-keyframe window: fewer tile groups per run recompute fewer Y blocks).
//    Few tiles and landmarks (at most 40 pairs and 256 x 16 landmarks; config
//    3: 28 pairs, 2 000 landmarks) take 2, so a 32-landmark run is split into
//    two tile groups: the same 48 MFMAs per wave as 16 landmarks x 4 tiles at
//    half the runs, the run's Y block formed twice (pt_schur 15.8 -> 14.9 us,
//    cam_solve 31.8 -> 31.4 us per iteration; undivided 32-landmark runs were
//    slower there than 16-landmark ones, 1.23 vs 1.19 ms per 10 iterations:
//    the longer per-workgroup chain).
//  * sorted: the runs in band order (plan_band / plan_order) beyond 40 pairs
//    (config 4: 66, config 5: 190); at config 3 the two plan launches cost
//    more than the partial traffic saves.
void schur_geometry(int npairs, int np, int Rpad, Geo& g) {
  const bool wide = schur_lds_bytes(kSchurPtsWide, Rpad) <= kSchurLdsCap;
  const bool split_wide = wide && npairs <= 40 && np <= 256 * kSchurPts;
  g.spts = wide ? kSchurPtsWide : npairs > 100 ? kSchurPtsSmall : kSchurPts;
  g.nsub = (int)std::max(1L, ((long)np + g.spts - 1) / g.spts);
  g.rsub = (int)std::max(1L, ((long)g.nsub + 255) / 256);
  g.rlen = g.spts * g.rsub;
  g.nruns = (int)std::max(1L, ((long)np + g.rlen - 1) / g.rlen);
  const int nt = split_wide ? 2 : npairs > 100 ? kSchurNtMax : std::min(kSchurNtMax, 4);
  g.stpw = 8 * std::min((npairs + 7) / 8, nt);
  g.sgrp = (npairs + g.stpw - 1) / g.stpw;
  g.ksplit = (g.sgrp > 1 ? (int)rup((long)g.nruns, 8) : g.nruns) * g.sgrp;
  g.sorted = npairs > 40 ? 1 : 0;
}

// The sizes that follow from the window alone: the camera system and the Schur pass's geometry.
void ba_geometry(Geo& g, int n_cams, int fixed_frames, int n_pts) {
  g.nc = n_cams;
  g.np = n_pts;
  g.nf = std::min(std::max(fixed_frames, 0), n_cams);
  g.m = g.nc - g.nf;
  g.n6 = 6 * g.m;
  g.Rpad = (int)rup(g.n6 + 1, 16);  // camera columns | z_p column n6 | zero padding
  g.T = g.Rpad / 16;
  g.Ts = (g.n6 + 1 + 15) / 16;
  g.npairs = g.T * (g.T + 1) / 2;
  schur_geometry(g.npairs, g.np, g.Rpad, g);
}

// camera-solve launch form by size alone: 0 = LDS, 1 = global memory, 2 = with workers
// (enqueue_iteration: 2 runs as 1 where the ctx's CUs can host no worker beside block 0)
constexpr size_t kSolveLdsCap = 150 * 1024;
inline int solve_form(int Ts) {
  if (8 * (solve_small_doubles(Ts) + solve_a_doubles(Ts)) <= kSolveLdsCap) return 0;
  return Ts >= kSolveMwMinTs ? 2 : 1;
}

// Host-only debug symbol (tests/test_host.py pins it; not part of the ABI).
// out[10]: spts, nsub, rsub, rlen, nruns, stpw, sgrp, ksplit, sorted, camera-solve form
extern "C" int me_debug_ba_geometry(int n_cams, int fixed_frames, int n_pts, int* out) {
  if (n_cams <= 0 || n_pts < 0 || !out) return ME_ERR_INVALID;
  Geo g;
  ba_geometry(g, n_cams, fixed_frames, n_pts);
  const int v[10] = {g.spts, g.nsub, g.rsub, g.rlen, g.nruns, g.stpw, g.sgrp, g.ksplit, g.sorted, solve_form(g.Ts)};
  std::memcpy(out, v, sizeof v);
  return ME_OK;
}

int ba_drain(me_ctx* c);

// async >= 0: the plan of a queued asynchronous solve, built in scratch and
// staging set `async` (0 or 1) while the other set may still be in flight;
// every other plan first completes the queued solves (they own the scratch)
int plan_build(me_ctx* c, const me_ba_problem* p, const me_ba_options* opt, Plan& P, int slot_base,
               int async = -1, me_comm* comm = nullptr) {
  const bool cov_dev = P.cov && p->mem == ME_DEVICE;
  if (async < 0 && !cov_dev) ME_TRY(ba_drain(c));
  ME_CHECK(c, p->n_cams > 0 && p->n_pts >= 0 && p->n_obs >= 0, "BA: bad sizes");
  ME_CHECK(c, p->n_cams <= kMaxScanCams, "BA: at most %d cameras per window", kMaxScanCams);
  ME_CHECK(c, p->obs_dim == 0 || p->obs_dim == 2 || p->obs_dim == 4, "BA: obs_dim must be 2 or 4 (Observation<M>)");
  const bool mono = p->obs_dim == 2;
  ME_CHECK(c, p->feat_var > 0 && (mono || p->baseline != 0.0), "BA: wrong calibration parameters (BundleAdjuster.h:147)");
  ME_CHECK(c, !mono || p->cam_id || p->n_obs == 0, "BA: obs_dim 2 needs cam_id (Observation::camID)");
  // BundleAdjuster<2>::optimise: a zero baseline is replaced by 0.5 (BundleAdjuster.h:389-390)
  const double baseline = mono && p->baseline == 0 ? 0.5 : p->baseline;
  ME_CHECK(c, p->mem == ME_HOST || p->mem == ME_DEVICE, "BA: bad memory kind");
  if (p->mem == ME_HOST) {  // device-resident input is validated on the device (State::bad_input)
    for (int i = 0; i < p->n_obs; ++i) {
      ME_CHECK(c, p->cam_idx[i] >= 0 && p->cam_idx[i] < p->n_cams && p->pt_idx[i] >= 0 && p->pt_idx[i] < p->n_pts,
               "BA: observation %d indexes outside the window", i);
    }
  }
  P.c = c;
  // the ctx's test-hook word (me_debug_solve_flags): the host-only bits are translated here
  int hook = c->dbg_solve_flags;
  if ((hook & kFlagFailEveryOther) && !P.cov && (c->dbg_solve_count++ & 1)) hook |= kFlagSolveFail;  // (solves only)
  P.no_fused_asm = (hook & kFlagSeparateAsm) != 0;
  P.solve_flags = hook & (kFlagAsmTimeout | kFlagSolveFail | kFlagRosterNow);
  Geo& g = P.g;
  ba_geometry(g, p->n_cams, p->fixed_frames, p->n_pts);
  g.no = p->n_obs;
  g.od = mono ? 2 : 4;
  // sharded: one gradient max-norm slot per rank (ABI-v2 callback without rank: one slot, max-reduced apart)
  P.comm = comm;
  P.xmax_separate = comm && comm->world == 0;
  g.xslots = comm && comm->world > 0 ? comm->world : 1;
  g.xrank = comm && comm->world > 0 ? comm->rank : 0;
  ME_CHECK(c, g.nruns <= kMaxRuns, "BA: %d Schur runs exceed %d", g.nruns, kMaxRuns);
  g.nblkp = blocks(std::max(g.np, 1), kBlock);
  ME_CHECK(c, g.npairs <= 8 * 24, "BA: %d variable cameras exceed the Schur tile budget", g.m);
  g.nblk_obs = (int)std::max(1L, rup(std::max(g.no, 1), kBlock) / kBlock);
  g.nblk_lin = (int)std::max(1L, rup(std::max(g.no, 1), lin_block(g.no)) / lin_block(g.no));
  g.nblk_pts = (int)std::max(1L, rup(std::max(g.np, 1), kPtBlock) / kPtBlock);
  // (band-sorted runs and runs of several sub-chunks keep the separate launch: the fused phase takes one sub-chunk
  // of consecutive landmarks; so do windows whose Y block leaves no LDS for its 512 x 9 sums)
  // Every tile group of a run repeats the run's linearisation.  That costs no time while the launch's workgroups
  // all run at once, one per CU (at most 128: the BA's half of the chip in the pipelined frame); a larger window
  // with several groups per run keeps the separate launch, which linearises every observation once.
  P.schur = schur_instance(g);
  ME_CHECK(c, P.schur, "BA: no Schur instance for obs_dim %d, %d tiles per wave, %d landmarks", g.od, schur_nt(g.stpw), g.spts);
  P.fused_lin = schur_fused_lin(g.od, schur_nt(g.stpw), g.spts) && g.rsub == 1 && !g.sorted &&
                (g.sgrp == 1 || g.ksplit <= 128) && schur_lds_bytes(g.spts, g.Rpad) + kSchurLinLds <= kSchurLdsCap;
  g.flin = P.fused_lin ? 1 : 0;
  g.ncost = P.fused_lin ? g.nruns : g.nblk_lin;  // (nruns <= ksplit <= pstride)
  g.jacobi = opt->jacobi_scaling ? 1 : 0;
  // camera-assembly units launched: the per-camera counts of a device-resident problem are unknown here, so the
  // bound on sum max(1, ceil(n_c / 256)); the plan's unit table marks the units past the total
  g.ncu = (int)(rup(std::max(g.no, 1), kBlock) / kBlock) + g.m;
  g.nblk_step = (int)std::max(1L, rup(std::max(g.np, 1), kStepPts) / kStepPts);
  g.pstride = std::max({g.nblk_obs, g.nblk_lin, g.nblk_pts, g.nblk_step, g.ksplit});
  std::memcpy(g.K0, p->K0, sizeof(g.K0));
  std::memcpy(g.K1, p->K1, sizeof(g.K1));
  g.baseline = baseline;
  g.sinv = 1.0 / std::sqrt(p->feat_var);
  const double Zmax = p->K0[0] * baseline / 0.1;
  const double Zmin = p->K0[0] * baseline / (2 * p->K0[2]);
  g.hi[0] = Zmax / p->K0[0] * p->K0[2];
  g.hi[1] = Zmax / p->K0[4] * p->K0[5];
  g.hi[2] = Zmax;
  g.lo[0] = -Zmax / p->K0[0] * p->K0[2];
  g.lo[1] = -Zmax / p->K0[4] * p->K0[5];
  g.lo[2] = Zmin;
  Opts& o = P.o;
  o.max_num_iterations = opt->max_num_iterations;
  o.function_tolerance = opt->function_tolerance;
  o.gradient_tolerance = opt->gradient_tolerance;
  o.parameter_tolerance = opt->parameter_tolerance;
  o.initial_radius = opt->initial_trust_region_radius;
  o.max_radius = opt->max_trust_region_radius;
  o.min_radius = opt->min_trust_region_radius;
  o.min_diag = opt->min_lm_diagonal;
  o.max_diag = opt->max_lm_diagonal;
  o.min_rel_decrease = opt->min_relative_decrease;
  o.max_invalid = opt->max_num_consecutive_invalid_steps;
  // The closing linearisation (the enqueue after max_num_iterations steps) leaves two things: x_cost, which the
  // last accepted step's decision already set to its candidate cost, and the gradient-tolerance test.  With the
  // tolerance off that test fires only on a gradient of exact zeros, so the pass is not queued and the last step's
  // decision ends the solve (close_t).  Without iterations it is the only linearisation (the initial cost): kept.
  o.close_in_decide = opt->gradient_tolerance > 0.0 || opt->max_num_iterations == 0 ? 0 : 1;
  const bool dev = p->mem == ME_DEVICE;
  // one arena; the five inputs first and contiguous (one H2D for host input)
  const long nb = g.pstride;
  Bufs& b = P.b;
  std::vector<std::pair<size_t, void**>> items;
  auto add = [&](size_t bytes, void* dst) { items.push_back({rup((long)std::max<size_t>(bytes, 8), 256), (void**)dst}); };
  add(8 * 6 * (size_t)g.nc, &b.cams[0]);
  add(8 * 3 * (size_t)g.np, &b.pts[0]);
  add(8 * g.od * (size_t)g.no, &b.obs);
  add(4 * (size_t)g.no, &b.cam_idx);
  add(4 * (size_t)g.no, &b.pt_idx);
  add(mono ? 4 * (size_t)g.no : 0, &b.cam_id);
  const size_t n_inputs = items.size();
  add(8 * 6 * (size_t)g.nc, &b.cams[1]);
  add(8 * 3 * (size_t)g.np, &b.pts[1]);
  add(4 * (size_t)(g.np + 1), &b.p_off);
  add(4 * (size_t)g.no, &b.p_obs);
  add(4 * (size_t)g.no, &b.pos);
  add(4 * (size_t)g.no, &b.p_cam);
  add(4 * (size_t)(g.m + 1), &b.c_off);
  add(4 * (size_t)g.no, &b.c_obs);
  add(4 * (size_t)g.no, &b.tmp_obs);
  add(4 * (size_t)g.no, &b.cpos);
  add(P.fused_lin ? 0 : 8 * kObsxStride * (size_t)g.no, &b.obsx);  // (fused: neither written nor read)
  add((size_t)g.no, &b.dup);
  add(8 * solve_a_doubles(g.Ts), &b.Abuf);
  add(8 * 18 * (size_t)g.no, &b.Wo);
  add(8 * (size_t)g.n6, &b.csc);
  add(8 * 3 * (size_t)g.np, &b.psc);
  add(8 * 36 * (size_t)g.m, &b.U);
  add(8 * (size_t)g.n6, &b.gcs);
  add(8 * 9 * (size_t)g.np, &b.V);
  add(8 * 3 * (size_t)g.np, &b.gps);
  add(8 * 9 * (size_t)g.np, &b.Lp);
  add(8 * 3 * (size_t)g.np, &b.zp);
  add(8 * 256 * (size_t)g.nruns * g.npairs, &b.Spart);
  add(4 * (size_t)std::max(g.np, 1), &b.order);
  add(4 * (size_t)std::max(g.np, 1), &b.pkey);
  add(4 * (size_t)std::max(g.np, 1), &b.prank);
  add(4 * (size_t)g.T * g.T * g.nblkp, &b.phist);
  add(8 * (size_t)g.nruns, &b.rband);
  add(4 * (size_t)g.npairs * g.nruns, &b.tl);
  add(4 * (size_t)g.npairs, &b.tcnt);
  add(8 * (size_t)g.n6 * g.n6 + 8 * (size_t)(2 * g.n6 + 2), &b.S);  // S | b | diagU | fail (contiguous for all-reduce)
  add(8 * (size_t)g.n6, &b.yc);
  add(8 * 3 * (size_t)g.np, &b.dp);
  add(8 * R_COUNT * (size_t)nb, &b.part);
  add(8 * (R_COUNT + 2), &b.scal);
  add(sizeof(State), &b.st);
  add(8 * (size_t)(g.n6 + 2), &P.colnorm);  // (+ the sharded first exchange's input flags)
  add(8 * (size_t)g.n6, &P.gc_raw);
  add(8 * 21 * (size_t)std::max(g.m, 1), &P.Uraw);
  add(8 * 27 * (size_t)g.ncu, &P.cpart);
  add(4 * (size_t)kCuStride * (size_t)rup(g.ncu, 8), &b.cunit);
  add(4 * (size_t)(g.m + 1 + 3 + 2), &b.cnt);  // counters: per camera (cam_assemble) | pt_step | solve sync (2) | fused assembly | roster (2)
  add(4 * (size_t)blocks((long)g.npairs * 256, kSolveBlock / kSaGroups), &b.asm_claim);  // (cleared with cnt)
  const size_t work_bytes = 4 * (2 * (size_t)g.np + (size_t)g.nblk_obs * g.nc + 4);
  add(work_bytes, &b.work);
  const size_t out_doubles = sizeof(State) / 8 + 6 * (size_t)g.nc + 3 * (size_t)g.np;
  add(8 * out_doubles, &b.out);
  b.xch = nullptr;
  if (comm) add(8 * (size_t)xo_total(g), &b.xch);
  // the rotation tables last: every other buffer keeps the offset it had without them (ahead of cams[1] the
  // config-5 solve measured 1.3 % behind the parent commit's, profiles/rot_tables_ab.txt)
  add(8 * kRotStride * (size_t)g.nc, &b.rot[0]);
  add(8 * kRotStride * (size_t)g.nc, &b.rot[1]);
  size_t total = 0, input_span = 0;
  for (size_t k = 0; k < items.size(); ++k) {
    total += items[k].first;
    if (k < n_inputs) input_span += items[k].first;
  }
  void* arena;
  ME_TRY(me_scratch(c, SLOT_COUNT + slot_base, total, &arena));
  char* ptr = (char*)arena;
  for (auto& it : items) {
    *it.second = ptr;
    ptr += it.first;
  }
  b.ssync = b.cnt + g.m + 1;
  b.roster = b.cnt + g.m + 4;
  b.bvec = b.S + (size_t)g.n6 * g.n6;
  b.diagU = b.bvec + g.n6;
  void* hp = nullptr;
  // (an asynchronous solve's staging also takes the window covariance queued behind it: cam | fail | pt blocks)
  const size_t cov_doubles = async >= 0 ? 36 * (size_t)g.nc + 1 + 9 * (size_t)g.np : 0;
  P.cov_off = out_doubles;
  // (and the flags of the residual check queued behind it: one byte per landmark)
  const size_t check_bytes = async >= 0 ? (size_t)rup(g.np, 8) : 0;
  P.check_off = 8 * (out_doubles + cov_doubles);
  const size_t stage = rup((long)std::max(P.check_off + check_bytes, dev ? (size_t)0 : input_span), 64);
  const size_t hbytes = stage + 2 * rup(sizeof(State), 64);
  if (async >= 0) {  // staging owned by the asynchronous solve (set `async` is free: its last solve was waited)
    if (c->ba_pinned_size[async] < hbytes) {
      if (c->ba_pinned[async]) ME_HIP(c, hipHostFree(c->ba_pinned[async]));
      c->ba_pinned[async] = nullptr;
      c->ba_pinned_size[async] = 0;
      ME_HIP(c, hipHostMalloc(&c->ba_pinned[async], std::max(hbytes, (size_t)4096), hipHostMallocDefault));
      c->ba_pinned_size[async] = std::max(hbytes, (size_t)4096);
    }
    hp = c->ba_pinned[async];
  } else if (!cov_dev) {
    ME_TRY(me_pinned(c, hbytes, &hp));
  }
  P.host = (double*)hp;
  if (P.reserve_only) return ME_OK;
  P.hstate[0] = (State*)((char*)hp + stage);
  P.hstate[1] = (State*)((char*)hp + stage + rup(sizeof(State), 64));
  P.dev = dev;
  hipStream_t s = c->stream;
  if (!dev) {
    // pack the inputs at their arena offsets in pinned memory: one H2D copy
    char* h = (char*)hp;
    const void* src[6] = {p->cams, p->pts, p->obs, p->cam_idx, p->pt_idx, p->cam_id};
    const size_t len[6] = {8 * 6 * (size_t)g.nc, 8 * 3 * (size_t)g.np, 8 * g.od * (size_t)g.no, 4 * (size_t)g.no,
                           4 * (size_t)g.no, mono ? 4 * (size_t)g.no : 0};
    size_t off = 0;
    for (int k = 0; k < 6; ++k) {
      if (len[k]) std::memcpy(h + off, src[k], len[k]);
      off += items[k].first;
    }
    ME_HIP(c, hipMemcpyAsync(b.cams[0], hp, input_span, hipMemcpyHostToDevice, s));
  } else {
    b.obs = p->obs;
    b.cam_idx = p->cam_idx;
    b.pt_idx = p->pt_idx;
    if (mono) b.cam_id = p->cam_id;
  }
  // cnt | work are adjacent in the arena: one fill clears both
  ME_HIP(c, hipMemsetAsync(b.cnt, 0, (size_t)((char*)b.work - (char*)b.cnt) + work_bytes, s));
  P.asm_gen = 0;  // (the claim words were just cleared)
  const double* cams_in = dev ? p->cams : b.cams[0];
  const double* pts_in = dev ? p->pts : b.pts[0];
  const long nthr = std::max({(long)g.nblk_obs * kBlock, (long)g.np, 6L * g.nc, 3L * g.np});
  hipLaunchKernelGGL(plan_count_kernel, dim3(blocks(nthr, kBlock) + 1), dim3(kBlock), 4 * (size_t)g.nc, s, g, b,
                     cams_in, pts_in);  // (+ 1: the rotation table's workgroup)
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, g, b, o);
  hipLaunchKernelGGL(plan_scatter_kernel, dim3(g.nblk_obs), dim3(kBlock), 0, s, g, b);
  hipLaunchKernelGGL(plan_segsort_kernel, dim3(blocks(std::max(g.np, 1), kSortBlock / 64)), dim3(kSortBlock), 0, s, g,
                     b);
  if (g.sorted) {
    hipLaunchKernelGGL(plan_band_kernel, dim3(g.nblkp), dim3(kBlock), 0, s, g, b);
    hipLaunchKernelGGL(plan_order_kernel, dim3(1), dim3(kScanBlock), 0, s, g, b);
  }
  ME_TRY(me_check_launch(c, "BA plan"));
  // LDS for the camera solve
  P.use_lds = solve_form(g.Ts) == 0 ? 1 : 0;
  P.solve_lds = 8 * (solve_small_doubles(g.Ts) + (P.use_lds ? solve_a_doubles(g.Ts) : 0));
  ME_CHECK(c, P.solve_lds <= kSolveLdsCap, "BA: %d variable cameras exceed the camera-solve workspace", g.m);
  P.schur_lds = schur_lds_bytes(g.spts, g.Rpad) + (P.fused_lin ? kSchurLinLds : 0);
  ME_CHECK(c, P.schur_lds <= kSchurLdsCap, "BA: %d variable cameras exceed the Schur workspace", g.m);
  // dynamic-LDS ceilings of the solve and Schur kernels: set once per context
  // at the cap every plan stays under (not per solve: ~36 runtime calls of
  // host time in front of every queued solve)
  if (!c->ba_lds_attr) {
    for (const void* k : kSolveKernels)
      ME_HIP(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSolveLdsCap));
    for (const SchurInstance& i : kSchurInstances)
      ME_HIP(c, hipFuncSetAttribute((const void*)i.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSchurLdsCap));
    c->ba_lds_attr = 1;
  }
  // the multi-workgroup camera solve deals its tiles over the workers that
  // joined its roster (roster.hpp), so residency is never assumed; the
  // workers launched are still capped by what fits on the ctx's CUs (more
  // could only join late and leave)
  if (!P.use_lds) {
    int per_cu = 0;
    ME_HIP(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cam_solve_kernel<2>, kSolveBlock, P.solve_lds));
    P.solve_cap = std::max(0, per_cu) * (c->cu_active > 0 ? c->cu_active : c->num_cu);
    if (P.comm && g.Ts >= kSolveMwMinTs) {
      // Sharded: every rank solves the camera system redundantly and must run
      // the same solve form (worker count) on the same operands, whatever its
      // own CU mask: the smallest capacity over the ranks (one max exchange of
      // -cap at plan time; the result is read back before any iteration).
      double* d = P.b.scal;  // (free until the first linearisation)
      const double v = -(double)P.solve_cap;
      ME_HIP(c, hipMemcpyAsync(d, &v, 8, hipMemcpyHostToDevice, c->stream));
      ME_TRY(me_comm_allreduce_impl(P.comm, d, 1, ME_COMM_MAX));
      double r = 0.0;
      ME_HIP(c, hipMemcpyAsync(&r, d, 8, hipMemcpyDeviceToHost, c->stream));
      ME_HIP(c, hipStreamSynchronize(c->stream));
      P.solve_cap = (int)-r;
    }
  }
  return ME_OK;
}

// all-reduce of n doubles on the ctx stream through the plan's communicator
#define ME_XCH(ptr, n, op) ME_TRY(me_comm_allreduce_impl(P.comm, (ptr), (long)(n), (op)))

// Linearisation stage (device-skipped when need_lin == 0)
int enqueue_linearize(Plan& P) {
  me_ctx* c = P.c;
  const Geo& g = P.g;
  hipStream_t s = c->stream;
  const bool sh = P.comm != nullptr;
  // (no launch when the plan's Schur instance linearises in its phase A: the
  // first pass is then cam_assemble -> Schur, every later one the Schur launch)
  if (!P.fused_lin) {
    me_ktimer t(c, ME_KT_BA_LINEARIZE);
    const bool small = lin_block(g.no) == kLinSmall;
    if (g.od == 4 && small)
      hipLaunchKernelGGL((linearize_kernel<4, kLinSmall>), dim3(g.nblk_lin), dim3(kLinSmall), 0, s, g, P.b);
    else if (g.od == 4)
      hipLaunchKernelGGL((linearize_kernel<4, kBlock>), dim3(g.nblk_lin), dim3(kBlock), 0, s, g, P.b);
    else if (small)
      hipLaunchKernelGGL((linearize_kernel<2, kLinSmall>), dim3(g.nblk_lin), dim3(kLinSmall), 0, s, g, P.b);
    else
      hipLaunchKernelGGL((linearize_kernel<2, kBlock>), dim3(g.nblk_lin), dim3(kBlock), 0, s, g, P.b);
  }
  // After the first linearisation the Jacobi scaling is fixed and the Schur
  // pass no longer needs the camera assembly: its unit workgroups then ride
  // in the Schur launch (one launch fewer per iteration; a second stream with
  // event fork/join measured slower).  Sharded runs too: a rank's U and g
  // blocks are then scaled by the fixed global scaling, and the exchange sums
  // them.
  const bool first = P.n_enq == 0;
  const bool fused = !first && g.m > 0;
  ++P.n_enq;
  CamArgs ca{P.cpart, P.colnorm, P.gc_raw, P.Uraw, fused ? 1 : 0, fused ? (g.ncu + 7) / 8 * 8 : 0};
  if (g.m > 0 && !fused)
    hipLaunchKernelGGL(cam_assemble_kernel, dim3(g.ncu), dim3(kBlock), 0, s, g, P.b, P.cpart, sh ? 1 : 0,
                       P.colnorm, P.gc_raw, P.Uraw);
  if (sh && !fused) {
    // the Jacobi scaling needs the global column norms: the first exchange
    // (with every rank's input flags behind them), then the local blocks scaled
    if (first) {
      hipLaunchKernelGGL(xch_flags_kernel, dim3(1), dim3(1), 0, s, g, P.b, P.colnorm);
      ME_XCH(P.colnorm, g.n6 + 2, ME_COMM_SUM);
    }
    hipLaunchKernelGGL(cam_finish_kernel, dim3(blocks(std::max(g.m, 1), 64)), dim3(64), 0, s, g, P.b,
                       (const double*)P.colnorm, (const double*)P.gc_raw, (const double*)P.Uraw, first ? 1 : 0);
  }
  {
    // point blocks + Schur partial tiles (BA_SCHUR family)
    me_ktimer t(c, ME_KT_BA_SCHUR, true);  // (sampled launches take the timer's events)
    hipExtLaunchKernelGGL(P.schur, dim3(g.ksplit + ca.ncam), dim3(512), P.schur_lds, s, t.a, t.b, 0, g, P.b, P.o, ca);
  }
  if (sh) {
    // this rank's reduced camera system, gradient and linearisation scalars
    // packed, then ONE sum over the ranks
    hipLaunchKernelGGL(s_assemble_kernel, dim3(blocks((long)g.npairs * 256, kSaElems) + 1), dim3(kBlock), 0, s, g,
                       P.b, P.o, (const double*)P.gc_raw, 0, (int)SA_PACK);
    if (P.xmax_separate) {
      ME_XCH(P.b.xch, xo_gmax(g), ME_COMM_SUM);
      ME_XCH(P.b.xch + xo_gmax(g), 1, ME_COMM_MAX);
    } else {
      ME_XCH(P.b.xch, xo_total(g), ME_COMM_SUM);
    }
  }
  return me_check_launch(c, "BA linearize");
}

// S / b assembly; its last workgroup closes the linearisation (lin_finalize).
// Sharded: S / b unpacked from the all-reduced exchange.
// img: the assembly writes the camera solve's image of [S + D; -b^T] (the
// solver's padded layout, s_assemble_body) into Abuf, so the solve that
// follows loads nothing: its element-wise load of S cost wg0 ~70 us at config
// 5 (tools/drivers.py solve_ts).  Not with full_S (S itself is read back).
int enqueue_assemble(Plan& P, bool img = false) {
  me_ctx* c = P.c;
  const Geo& g = P.g;
  const int mode = P.comm ? SA_UNPACK : SA_SUM;
  if (g.m > 0)
    hipLaunchKernelGGL(s_assemble_kernel, dim3(blocks((long)g.npairs * 256, kSaElems) + 1), dim3(kBlock), 0,
                       c->stream, g, P.b, P.o, (const double*)P.gc_raw, P.full_S ? 1 : 0, mode,
                       img && !P.full_S ? P.b.Abuf : nullptr);
  else
    hipLaunchKernelGGL(lin_finalize_kernel, dim3(1), dim3(kFinBlock), 0, c->stream, g, P.b, P.o,
                       (const double*)P.gc_raw);
  return me_check_launch(c, "BA assemble");
}

// `last`: the enqueue after max_num_iterations steps.  Its linearisation feeds
// only the closing gradient test and final cost, and its lin_finalize always
// ends the solve (iterations == max_num_iterations), so the camera solve and
// the point step that would follow are never run: they are not queued (two
// no-op launches fewer per solve; every rank of a sharded solve skips alike).
// A plan with Opts::close_in_decide queues no such pass at all (lin_passes).
int enqueue_iteration(Plan& P, bool last = false) {
  me_ctx* c = P.c;
  const Geo& g = P.g;
  hipStream_t s = c->stream;
  const bool sh = P.comm != nullptr;
  ME_TRY(enqueue_linearize(P));
  // camera-solve form: 0 = [S; -b^T] in LDS, 1 = global memory, 2 = global
  // memory with trailing-update workers.  Trailing-update workers pay once the
  // block steps are many and wide: config 5 (19 steps) 372 -> 274 us per
  // solve; config 4 (11 steps) is faster on one workgroup (118 vs 131 us: the
  // per-step hand-offs).  The workers are capped by what can be co-resident.
  const int np0 = (g.Ts - 1) * g.Ts / 2;
  int nwk = solve_form(g.Ts) == 2 ? std::min(64, std::max(1, (np0 + kSolveBlock / 64 - 1) / (kSolveBlock / 64))) : 0;
  nwk = std::max(0, std::min(nwk, P.solve_cap - 1));
  // S = U - sum of the Schur partials is assembled by wide workgroups
  // (coalesced, all CUs) rather than by the one-workgroup solve, whose
  // dependent cross-XCD loads would otherwise dominate the iteration.  Modes
  // 0 and 1 they ride in the camera-solve launch (fused assembly; sharded:
  // they unpack the exchanged system).
  const bool fuse = g.m > 0 && !P.full_S && !last && nwk == 0 && !P.no_fused_asm;
  const int nasm = fuse ? blocks((long)g.npairs * 256, kSolveBlock / kSaGroups) : 0;
  const bool img = !fuse && !last && g.m > 0 && !P.full_S && ME_SOLVE_IMG;
  if (!fuse) ME_TRY(enqueue_assemble(P, img));
  if (last) return me_check_launch(c, "BA iteration");
  if (g.m == 0) ME_HIP(c, hipMemsetAsync(P.b.scal + R_COUNT, 0, 8, s));
  {
    me_ktimer t(c, ME_KT_BA_SOLVE);
    const double* gc = P.gc_raw;
    const int sk = P.solve_flags | (img ? kFlagImg : 0);
    const unsigned gen = nasm > 0 ? ++P.asm_gen : 0u;  // fused assembly: this launch's claim generation
    if (P.use_lds)
      hipLaunchKernelGGL(cam_solve_kernel<0>, dim3(1 + nasm), dim3(kSolveBlock), P.solve_lds, s, g, P.b, P.o, sk, 0,
                         nasm, gc, gen);
    else if (nwk > 0)
#ifdef ME_COOP_LAUNCH  // measurement build only (tools/gpu.sh coop): the worker grid as a cooperative launch
    {
      int skv = sk, nwv = nwk, z = 0;
      unsigned gv = gen;
      void* args[] = {(void*)&g, (void*)&P.b, (void*)&P.o, &skv, &nwv, &z, (void*)&gc, &gv};
      ME_HIP(c, hipLaunchCooperativeKernel((const void*)cam_solve_kernel<2>, dim3(1 + nwk), dim3(kSolveBlock), args,
                                           (unsigned)P.solve_lds, s));
    }
#else
      hipLaunchKernelGGL(cam_solve_kernel<2>, dim3(1 + nwk), dim3(kSolveBlock), P.solve_lds, s, g, P.b, P.o, sk, nwk,
                         0, gc, gen);
#endif
    else
      hipLaunchKernelGGL(cam_solve_kernel<1>, dim3(1 + nasm), dim3(kSolveBlock), P.solve_lds, s, g, P.b, P.o, sk, 0,
                         nasm, gc, gen);
  }
  {
    me_ktimer t(c, ME_KT_BA_STEP);
    // (step partials reduced and, single-GPU, the step decided in its last workgroup)
    if (g.od == 4)
      hipLaunchKernelGGL(pt_step_kernel<4>, dim3(g.nblk_step + 1), dim3(kStepBlock), 0, s, g, P.b, P.o, sh ? 0 : 1);
    else
      hipLaunchKernelGGL(pt_step_kernel<2>, dim3(g.nblk_step + 1), dim3(kStepBlock), 0, s, g, P.b, P.o, sh ? 0 : 1);
  }
  if (sh) {
    ME_XCH(P.b.scal + R_MODEL, 5, ME_COMM_SUM);  // model change, candidate cost, step^2, |x|^2, failure count
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(64), 0, s, g, P.b, P.o);
  }
  return me_check_launch(c, "BA iteration");
}

// The enqueue_iteration calls of a whole solve: max_num_iterations iterations
// and, unless the last step's decision ends the solve (Opts::close_in_decide),
// the closing pass (`last`).  It follows from the options alone, so every rank
// of a sharded solve queues the same collectives.
inline int lin_passes(const Plan& P) {
  return P.o.max_num_iterations + (P.o.close_in_decide ? 0 : 1);
}

// Final state (and host parameters) -> pinned staging; enqueued behind the
// last chunk so the read-back does not wait for a host round trip.
int enqueue_output(Plan& P, me_ba_problem* p) {
  me_ctx* c = P.c;
  const Geo& g = P.g;
  constexpr size_t nst = sizeof(State) / 8;
  double* cams_dst = P.dev ? p->cams : P.b.out + nst;
  double* pts_dst = P.dev ? p->pts : P.b.out + nst + 6 * (size_t)g.nc;
  const long n = std::max({(long)nst, 6L * g.nc, 3L * g.np});
  hipLaunchKernelGGL(output_kernel, dim3(blocks(n, kBlock)), dim3(kBlock), 0, c->stream, g, P.b, cams_dst, pts_dst);
  ME_TRY(me_check_launch(c, "BA output"));
  const size_t bytes = 8 * (P.dev ? nst : nst + 6 * (size_t)g.nc + 3 * (size_t)g.np);
  ME_HIP(c, hipMemcpyAsync(P.host, P.b.out, bytes, hipMemcpyDeviceToHost, c->stream));
  if (P.dev && P.copy_out) {  // (staging holds State | cams | pts: out_doubles)
    ME_HIP(c, hipMemcpyAsync(P.host + nst, p->cams, 8 * 6 * (size_t)g.nc, hipMemcpyDeviceToHost, c->stream));
    if (g.np)
      ME_HIP(c, hipMemcpyAsync(P.host + nst + 6 * (size_t)g.nc, p->pts, 8 * 3 * (size_t)g.np, hipMemcpyDeviceToHost,
                               c->stream));
  }
  return ME_OK;
}

int finish(Plan& P, me_ba_problem* p, me_ba_summary* sum, bool output_queued = false, hipEvent_t done = nullptr) {
  me_ctx* c = P.c;
  const Geo& g = P.g;
  constexpr size_t nst = sizeof(State) / 8;
  static_assert(sizeof(State) % 8 == 0, "State is read back as doubles");
  if (!output_queued) ME_TRY(enqueue_output(P, p));
  if (done) ME_HIP(c, hipEventSynchronize(done));  // asynchronous solve: not the work queued after it
  else ME_HIP(c, hipStreamSynchronize(c->stream));
  State st;
  std::memcpy(&st, P.host, sizeof(State));
  std::memcpy(P.c->dbg, st.stamps, sizeof(st.stamps));
  if (!P.dev) {
    std::memcpy(p->cams, P.host + nst, 8 * 6 * (size_t)g.nc);
    if (g.np) std::memcpy(p->pts, P.host + nst + 6 * (size_t)g.nc, 8 * 3 * (size_t)g.np);
  }
  if (st.bad_input) return me_set_error(c, ME_ERR_INVALID, "BA: an observation indexes outside the window");
  if (st.spin_err)
    return me_set_error(c, ME_ERR_STATE,
                        "BA: a cross-workgroup hand-off of the camera solve timed out (workgroups not co-resident: "
                        "CU mask or concurrent persistent kernels; wait sites 0x%x: 1 worker roster, 2 worker step "
                        "poll, 4 fused assemblers, 8 LDS step flags, 16 workers' count, 32 backward flags, 0 the "
                        "step exchange)",
                        (unsigned)st.pad[0]);
  if (sum) {
    sum->termination = st.termination;
    sum->iterations = st.iterations;
    sum->successful_steps = st.successful;
    sum->initial_cost = st.initial_cost;
    sum->final_cost = st.x_cost;
    sum->status = st.termination == 2 ? 3 : 2;
    if (st.infeasible) {  // Ceres: infeasible start -> FAILURE, parameters untouched
      sum->iterations = 0;
      sum->successful_steps = 0;
      sum->initial_cost = sum->final_cost = NAN;
    }
  }
  return ME_OK;
}

int solve_impl(me_ctx* c, me_ba_problem* p, const me_ba_options* opt, me_comm* comm, me_ba_summary* sum) {
  me_range range_("me_ba_solve");
  if (!c || !p || !opt) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  Plan P;
  ME_TRY(plan_build(c, p, opt, P, 0, -1, comm));
  // Enqueue the solve in chunks of iterations.  The device State after each
  // chunk is copied to a pinned slot behind an event, and the host inspects
  // chunk k only after chunk k + 1 is queued, so the GPU never drains while
  // the host polls; after convergence at most one chunk of no-op launches
  // (every kernel tests State::done first) is left in the queue.
  const int chunk = 4;
  const int passes = lin_passes(P);
  int it = 0;
  auto enqueue_chunk = [&](int slot) -> int {
    for (int k = 0; k < chunk && it < passes; ++k, ++it)
      ME_TRY(enqueue_iteration(P, it == opt->max_num_iterations));
    ME_HIP(c, hipMemcpyAsync(P.hstate[slot], P.b.st, sizeof(State), hipMemcpyDeviceToHost, c->stream));
    ME_HIP(c, hipEventRecord(c->poll_ev[slot], c->stream));
    return ME_OK;
  };
  // once the last possible chunk is queued, the output follows it at once
  bool out_q = false;
  ME_TRY(enqueue_chunk(0));
  if (it >= passes) {
    ME_TRY(enqueue_output(P, p));
    out_q = true;
  }
  for (int cur = 0;; cur ^= 1) {
    const bool more = it < passes;
    if (more) {
      ME_TRY(enqueue_chunk(cur ^ 1));
      if (it >= passes) {
        ME_TRY(enqueue_output(P, p));
        out_q = true;
      }
    }
    ME_HIP(c, hipEventSynchronize(c->poll_ev[cur]));
    if (P.hstate[cur]->done || !more) break;
  }
  return finish(P, p, sum, out_q);
}

// Asynchronous solve: every possible iteration is queued at once (launches
// after convergence test State::done and return), then the output kernel and
// read-back behind an event.  The host is free as soon as it is queued.  Up
// to two solves may be queued on a ctx (each in its own scratch / staging
// set), so a caller can queue window t+1 behind window t without waiting:
// the device never idles while the host builds the next plan.
struct AsyncSolve {
  Plan P;
  me_ba_problem prob;  // copy: cams / pts are written back at completion
  hipEvent_t ev = nullptr;
  int set = 0;  // scratch / staging set
  bool completed = false;
  int rc = ME_OK;
  int cov = 0;  // window covariance queued behind the solve (solve_async_impl): staged at P.host + P.cov_off
  bool check = false;  // residual check queued behind the solve: its flags staged at P.host (bytes) + P.check_off
  me_ba_summary sum{};
};
constexpr int kBaQueue = 2;
// The queue may be used from two host threads at once: one queueing window
// t (me_ba_solve_async / me_vo_window_submit) while another waits for window
// t-1 (me_ba_wait_out).  The lock guards the FIFO only; the solve's own
// queueing and waiting run outside it.  The newest waited solve is retained
// (`last`) until a newer one is queued: window t may be chained from window
// t-1 (me_vo_ba_chain) after t-1 was waited.
struct AsyncQueue {
  AsyncSolve* q[kBaQueue] = {nullptr, nullptr};  // FIFO: q[0] oldest
  int n = 0;
  AsyncSolve* last = nullptr;  // newest waited solve (chain source)
  int last_set = 1;            // scratch / staging set of the newest queued solve
  std::mutex mu;
};

int ba_complete_one(me_ctx* c, AsyncSolve* A) {
  if (A->completed) return ME_OK;
  A->rc = finish(A->P, &A->prob, &A->sum, true, A->ev);
  A->completed = true;
  return ME_OK;
}

void ba_async_free(me_ctx* c) {
  auto* Q = (AsyncQueue*)c->ba_async;
  if (!Q) return;
  for (int i = 0; i < Q->n; ++i) {
    AsyncSolve* A = Q->q[i];
    if (!A->completed) hipEventSynchronize(A->ev);
    hipEventDestroy(A->ev);
    delete A;
  }
  delete Q->last;  // (its event was destroyed when it was waited)
  delete Q;
  c->ba_async = nullptr;
  c->ba_async_free = nullptr;
}

AsyncQueue* ba_queue(me_ctx* c) {
  if (!c->ba_async) {
    c->ba_async = new AsyncQueue;
    c->ba_async_free = ba_async_free;
  }
  return (AsyncQueue*)c->ba_async;
}

// Any other BA call on the ctx first completes the queued solves (their
// summaries stay readable by me_ba_wait, oldest first).
int ba_drain(me_ctx* c) {
  auto* Q = (AsyncQueue*)c->ba_async;
  if (!Q) return ME_OK;
  for (int i = 0; i < Q->n; ++i) ME_TRY(ba_complete_one(c, Q->q[i]));
  return ME_OK;
}

// the solve a new one is chained from: the newest queued, else the newest waited
AsyncSolve* ba_chain_source(AsyncQueue* Q) {
  std::lock_guard<std::mutex> lk(Q->mu);
  return Q->n ? Q->q[Q->n - 1] : Q->last;
}

// The window covariance's own scratch (beside the solves' sets 0 and 1, so a
// solve queued on the ctx may run behind it): the plan's arena in set 2, and
// Sigma_cc | camera blocks | the two failure words (one double) | landmark
// blocks: a host problem reads back from the camera blocks on, up to the
// failure words when no landmark block was asked for.
constexpr int kCovSet = 2, kCovOutSlot = SLOT_COUNT + 3;
// The residual check's outputs where the caller gives no device memory (a host problem's chi2 | flags, the flags
// of a check queued behind a solve): one slot, used in stream order.  A device-resident problem's stand-alone check
// builds its plan in the covariance's set.
constexpr int kCheckOutSlot = SLOT_COUNT + 4;
struct CovOut {
  double *Sig, *cam, *pt;
  int* fail;
};
int cov_out(me_ctx* c, const Geo& g, CovOut& o) {
  const size_t nsig = (size_t)g.n6 * g.n6, ncam = 36 * (size_t)g.nc, npt = 9 * (size_t)g.np;
  void* d;
  ME_TRY(me_scratch(c, kCovOutSlot, 8 * (nsig + ncam + 1 + npt) + 64, &d));
  o.Sig = (double*)d;
  o.cam = o.Sig + nsig;
  o.fail = (int*)(o.cam + ncam);
  o.pt = o.cam + ncam + 1;
  return ME_OK;
}

}  // namespace

// copy_out: a device-resident problem's solved cams / pts also read back
// into the staging behind the solve (me_vo_window_submit; me_ba_wait_out
// then returns them without touching the stream)
static int cov_enqueue(me_ctx* c, const me_ba_problem* p, bool want_pts, CovOut& out, Geo& gout);

// cov: 0 none, 1 the window covariance's camera blocks, 2 also its landmark blocks, queued behind the solve's
// output at the cams / pts it leaves and read back into the solve's staging (me_ba_wait_out_cov) ahead of its event
// check: the residual check (me_ba_point_check) behind both, over the solve's own plan (its CSR by point is intact
// until the set is built again), its flags read back the same way (me_ba_wait_out_check)
static int solve_async_impl(me_ctx* c, me_ba_problem* p, const me_ba_options* opt, bool copy_out, int cov = 0,
                            const me_ba_point_check_params* check = nullptr) {
  if (!c || !p || !opt) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  AsyncQueue* Q = ba_queue(c);
  auto* A = new AsyncSolve;
  {
    std::lock_guard<std::mutex> lk(Q->mu);
    if (Q->n >= kBaQueue) {
      delete A;
      return me_set_error(c, ME_ERR_STATE,
                          "me_ba_solve_async: %d solves already queued on this context (me_ba_wait first)", kBaQueue);
    }
    A->set = 1 - Q->last_set;  // never the set of the solve queued before (queued, or being read back)
    Q->last_set = A->set;
  }
  A->prob = *p;
  int rc = plan_build(c, p, opt, A->P, A->set, A->set);
  A->P.copy_out = copy_out && A->P.dev;
  if (rc == ME_OK) {
    for (int it = 0; it < lin_passes(A->P) && rc == ME_OK; ++it)
      rc = enqueue_iteration(A->P, it == opt->max_num_iterations);
  }
  if (rc == ME_OK) rc = enqueue_output(A->P, &A->prob);
  if (rc == ME_OK && cov && A->P.dev) {
    CovOut out;
    Geo g;
    rc = cov_enqueue(c, &A->prob, cov == 2, out, g);
    const size_t n = 36 * (size_t)g.nc + 1 + (cov == 2 ? 9 * (size_t)g.np : 0);
    if (rc == ME_OK && hipMemcpyAsync(A->P.host + A->P.cov_off, out.cam, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      rc = me_set_error(c, ME_ERR_HIP, "me_ba_solve_async: covariance read-back failed");
    A->cov = cov;
  }
  if (rc == ME_OK && check && A->P.dev) {
    const Geo& g = A->P.g;
    void* d = nullptr;
    rc = me_scratch(c, kCheckOutSlot, (size_t)std::max(g.np, 1), &d);
    if (rc == ME_OK) rc = me_ba_check_launch(c, g, A->P.b, A->prob.cams, A->prob.pts, check, nullptr, (uint8_t*)d);
    if (rc == ME_OK && g.np &&
        hipMemcpyAsync((char*)A->P.host + A->P.check_off, d, (size_t)g.np, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      rc = me_set_error(c, ME_ERR_HIP, "me_ba_solve_async: residual check read-back failed");
    A->check = true;
  }
  if (rc == ME_OK && hipEventCreateWithFlags(&A->ev, hipEventDisableTiming) != hipSuccess)
    rc = me_set_error(c, ME_ERR_HIP, "me_ba_solve_async: event creation failed");
  if (rc == ME_OK && hipEventRecord(A->ev, c->stream) != hipSuccess) {
    hipEventDestroy(A->ev);
    rc = me_set_error(c, ME_ERR_HIP, "me_ba_solve_async: event record failed");
  }
  if (rc != ME_OK) {
    hipStreamSynchronize(c->stream);  // nothing queued may outlive the plan
    delete A;
    return rc;
  }
  AsyncSolve* old = nullptr;
  {
    std::lock_guard<std::mutex> lk(Q->mu);
    Q->q[Q->n++] = A;
    std::swap(old, Q->last);  // a newer solve is queued: the retained chain source goes
  }
  delete old;
  return ME_OK;
}

extern "C" int me_ba_solve_async(me_ctx* c, me_ba_problem* p, const me_ba_options* opt) {
  me_range range_("me_ba_solve_async");
  return solve_async_impl(c, p, opt, false);
}

extern "C" int me_ba_wait_out(me_ctx* c, me_ba_summary* s, double* cams, double* pts) {
  return me_ba_wait_out_cov(c, s, cams, pts, nullptr, nullptr, nullptr);
}

extern "C" int me_ba_wait_out_cov(me_ctx* c, me_ba_summary* s, double* cams, double* pts, double* cam_cov,
                                  double* pt_cov, int* cov_ok) {
  return me_ba_wait_out_check(c, s, cams, pts, cam_cov, pt_cov, cov_ok, nullptr, nullptr);
}

extern "C" int me_ba_wait_out_check(me_ctx* c, me_ba_summary* s, double* cams, double* pts, double* cam_cov,
                                    double* pt_cov, int* cov_ok, uint8_t* flags, int* check_ok) {
  me_range range_("me_ba_wait");
  if (check_ok) *check_ok = 0;
  if (!c) return ME_ERR_INVALID;
  auto* Q = (AsyncQueue*)c->ba_async;
  AsyncSolve* A = nullptr;
  if (Q) {
    std::lock_guard<std::mutex> lk(Q->mu);
    if (Q->n) A = Q->q[0];
  }
  if (!A) return me_set_error(c, ME_ERR_STATE, "me_ba_wait: no asynchronous BA solve on this context");
  ME_HIP(c, hipSetDevice(c->device));
  ME_TRY(ba_complete_one(c, A));
  const int rc = A->rc;
  if (s && rc == ME_OK) *s = A->sum;
  if (rc == ME_OK && A->P.dev && (cams || pts)) {
    constexpr size_t nst = sizeof(State) / 8;
    const Geo& g = A->P.g;
    if (A->P.copy_out) {  // from the staging (read back behind the solve's event)
      if (cams) std::memcpy(cams, A->P.host + nst, 8 * 6 * (size_t)g.nc);
      if (pts && g.np) std::memcpy(pts, A->P.host + nst + 6 * (size_t)g.nc, 8 * 3 * (size_t)g.np);
    } else {  // (blocking copies on the null stream: the solve has completed; the ctx stream is not waited)
      if (cams) ME_HIP(c, hipMemcpy(cams, A->prob.cams, 8 * 6 * (size_t)g.nc, hipMemcpyDeviceToHost));
      if (pts && g.np) ME_HIP(c, hipMemcpy(pts, A->prob.pts, 8 * 3 * (size_t)g.np, hipMemcpyDeviceToHost));
    }
  }
  if (cov_ok) {  // the covariance queued behind the solve, from the same staging
    *cov_ok = 0;
    if (rc == ME_OK && A->cov) {
      const Geo& g = A->P.g;
      const double* h = A->P.host + A->P.cov_off;
      const size_t ncam = 36 * (size_t)g.nc;
      int fail[2];
      std::memcpy(fail, h + ncam, sizeof fail);
      if (!fail[0] && !fail[1]) {
        *cov_ok = A->cov;
        if (cam_cov) std::memcpy(cam_cov, h, 8 * ncam);
        if (pt_cov && A->cov == 2 && g.np) std::memcpy(pt_cov, h + ncam + 1, 8 * 9 * (size_t)g.np);
      }
    }
  }
  if (check_ok && rc == ME_OK && A->check && A->sum.termination != 2) {  // the check's flags, from the same staging
    *check_ok = 1;
    if (flags && A->P.g.np) std::memcpy(flags, (const char*)A->P.host + A->P.check_off, (size_t)A->P.g.np);
  }
  hipEventDestroy(A->ev);
  A->ev = nullptr;
  AsyncSolve* gone = A;
  {
    std::lock_guard<std::mutex> lk(Q->mu);
    for (int i = 1; i < Q->n; ++i) Q->q[i - 1] = Q->q[i];
    Q->q[--Q->n] = nullptr;
    if (Q->n == 0) {  // the newest: retained as the chain source until a newer one is queued
      std::swap(gone, Q->last);
    }
  }
  delete gone;
  return rc;
}

extern "C" int me_ba_wait(me_ctx* c, me_ba_summary* s) { return me_ba_wait_out(c, s, nullptr, nullptr); }

extern "C" int me_ba_reserve(me_ctx* c, int n_cams, int n_pts, int n_obs, int obs_dim, int fixed_frames) {
  me_range range_("me_ba_reserve");
  if (!c || n_cams < 1 || n_pts < 0 || n_obs < 0) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  auto* Q = (AsyncQueue*)c->ba_async;
  if (Q && Q->n > 0) return me_set_error(c, ME_ERR_STATE, "me_ba_reserve: asynchronous solves are queued");
  ME_TRY(ba_drain(c));
  // a problem of these sizes (no arrays: the plan stops once its memory is sized)
  static const int32_t zero = 0;
  me_ba_problem p{};
  p.n_cams = n_cams;
  p.n_pts = n_pts;
  p.n_obs = n_obs;
  p.obs_dim = obs_dim == 2 ? 2 : 4;
  p.fixed_frames = fixed_frames;
  p.mem = ME_DEVICE;
  p.cam_id = &zero;
  p.feat_var = 1.0;
  p.baseline = 1.0;
  const double K[9] = {1, 0, 1, 0, 1, 1, 0, 0, 1};
  std::memcpy(p.K0, K, sizeof(K));
  std::memcpy(p.K1, K, sizeof(K));
  me_ba_options o;
  me_ba_default_options(&o);
  for (int set = 0; set < kBaQueue; ++set) {  // the asynchronous solves' two sets
    Plan P;
    P.reserve_only = true;
    ME_TRY(plan_build(c, &p, &o, P, set, set));
  }
  {  // the window covariance's set and outputs (me_ba_covariance_full on a device-resident window)
    Plan P;
    P.reserve_only = true;
    P.cov = true;
    ME_TRY(plan_build(c, &p, &o, P, kCovSet));
    CovOut out;
    ME_TRY(cov_out(c, P.g, out));
    void* d;  // and the residual check's outputs (a host problem's chi2 | flags)
    ME_TRY(me_scratch(c, kCheckOutSlot, 9 * (size_t)std::max(n_pts, 1) + 8, &d));
  }
  Plan P;  // and the synchronous one
  P.reserve_only = true;
  return plan_build(c, &p, &o, P, 0);
}

extern "C" int me_vo_ba_chain(me_ctx* c, double* cams, int n_cams, double* pts, int n_pts, const int32_t* cam_src,
                              const int32_t* win_ids, const int32_t* prev_ids, int n_prev, int32_t new_from,
                              const me_vo_chain_args* a) {
  me_range range_("me_vo_ba_chain");
  if (!c || !a || n_cams < 1 || n_pts < 0 || n_prev < 0 || !cams || !cam_src ||
      (n_pts && (!pts || !win_ids)) || (n_prev && !prev_ids))
    return ME_ERR_INVALID;
  if (a->mode >= 0 && (a->k1 < 0 || a->k1 >= n_cams - 1 || (a->mode == 1 && (a->k0 < 0 || a->k0 >= n_cams - 1))))
    return me_set_error(c, ME_ERR_INVALID, "me_vo_ba_chain: prediction cameras %d, %d outside the window's first %d",
                        a->k1, a->k0, n_cams - 1);
  auto* Q = (AsyncQueue*)c->ba_async;
  AsyncSolve* A = Q ? ba_chain_source(Q) : nullptr;
  if (!A) return me_set_error(c, ME_ERR_STATE, "me_vo_ba_chain: no BA solve to chain from");
  if (!A->P.dev) return me_set_error(c, ME_ERR_STATE, "me_vo_ba_chain: the previous solve is not device-resident");
  ME_HIP(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(vo_chain_kernel, dim3(blocks(std::max(n_pts, 1), 256)), dim3(256), 48 * (size_t)n_cams, c->stream,
                     A->prob.cams, A->prob.pts, A->P.b.st, cams, n_cams, pts, n_pts, (const int*)cam_src,
                     (const int*)win_ids, (const int*)prev_ids, n_prev, (int)new_from, *a);
  return me_check_launch(c, "me_vo_ba_chain");
}

extern "C" int me_vo_window_submit(me_ctx* c, const me_vo_window* w, me_ba_problem* p, const me_ba_options* o) {
  me_range range_("me_vo_window_submit");
  if (!c || !w || !p || !o) return ME_ERR_INVALID;
  if (w->check)  // (refused before anything is queued)
    if (const char* why = me_ba_point_check_check(w->check))
      return me_set_error(c, ME_ERR_INVALID, "me_vo_window_submit: check: %s", why);
  ME_HIP(c, hipSetDevice(c->device));
  if (w->stage_bytes) ME_HIP(c, hipMemcpyAsync(w->dev, w->stage, w->stage_bytes, hipMemcpyHostToDevice, c->stream));
  if (w->chain)
    ME_TRY(me_vo_ba_chain(c, p->cams, p->n_cams, p->pts, p->n_pts, w->cam_src, w->win_ids, w->prev_ids, w->n_prev,
                          w->new_from, &w->args));
  // (the problem's index arrays are the caller's device buffers, filled here)
  ME_TRY(me_ba_window_indices(c, w->frame, w->ids, p->n_obs, w->first_frame, w->win_ids, p->n_pts,
                              const_cast<int32_t*>(p->cam_idx), const_cast<int32_t*>(p->pt_idx)));
  return solve_async_impl(c, p, o, true, w->cov == 1 || w->cov == 2 ? w->cov : 0, w->check);
}

extern "C" void me_ba_default_options(me_ba_options* o) {
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-3;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_relative_decrease = 1e-3;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
}

extern "C" int me_ba_solve(me_ctx* c, me_ba_problem* p, const me_ba_options* o, me_ba_summary* s) {
  return solve_impl(c, p, o, nullptr, s);
}

#ifdef ME_SOLVE_TS
extern "C" int me_solve_ts(long long* out, int reset) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(g_solve_ts), sizeof(g_solve_ts));
  if (reset) {
    long long z[24] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(g_solve_ts), z, sizeof(z));
  }
  return 0;
}
#endif

extern "C" int me_ba_solve_comm(me_ctx* c, me_ba_problem* p, const me_ba_options* o, me_comm* comm,
                                me_ba_summary* s) {
  if (!c) return ME_ERR_INVALID;
  if (!comm) return me_set_error(c, ME_ERR_INVALID, "me_ba_solve_comm: null communicator");
  if (comm->ctx != c) return me_set_error(c, ME_ERR_INVALID, "me_ba_solve_comm: the communicator belongs to another ctx");
  return solve_impl(c, p, o, comm, s);
}

// ABI-v2 form: a callback without rank information (world 0: one gradient
// max-norm slot, reduced by its own max all-reduce)
// Per-exchange estimate (µs) of the packed all-reduce at `world` ranks: the
// one-rank RCCL exchange measured on MI355X (~14 µs each, bench
// sharded_ba.rccl_1rank, r03) is the floor; every doubling of the ring adds a
// latency step over xGMI (an estimate until the driver's 8-GPU line measures it).
extern "C" double me_ba_shard_exchange_us(int world) {
  if (world <= 1) return 0.0;
  double us = 14.0;
  for (int w = 2; w <= world; w *= 2) us += 4.0;
  return us;
}

extern "C" int me_ba_shard_worthwhile(long n_obs, int world, double xch_us) {
  if (world <= 1 || n_obs <= 0) return 0;
  if (!(xch_us > 0.0)) xch_us = me_ba_shard_exchange_us(world);
  auto t = [](double n) { return std::max(ME_SHARD_FLOOR_US, n * ME_SHARD_OBS_NS * 1e-3); };
  const double saved = t((double)n_obs) - t(std::ceil((double)n_obs / world));
  return saved > 2.0 * xch_us ? 1 : 0;
}

extern "C" int me_ba_solve_sharded(me_ctx* c, me_ba_problem* p, const me_ba_options* o, me_allreduce_fn ar,
                                   void* user, me_ba_summary* s) {
  if (!c) return ME_ERR_INVALID;
  if (!ar) return me_set_error(c, ME_ERR_INVALID, "me_ba_solve_sharded: null allreduce");
  me_comm m;
  m.ctx = c;
  m.world = 0;
  m.rank = 0;
  m.ar = ar;
  m.user = user;
  return solve_impl(c, p, o, &m, s);
}

extern "C" int me_ba_cost(me_ctx* c, const me_ba_problem* p, double* cost) {
  if (!c || !p) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  me_ba_options o;
  me_ba_default_options(&o);
  Plan P;
  ME_CHECK(c, p->mem == ME_HOST, "BA: evaluation helpers take host arrays");
  int rc = plan_build(c, p, &o, P, 0);
  if (rc < 0) return rc;
  std::vector<double> part(P.g.nblk_obs);
  if (P.g.od == 4)
    hipLaunchKernelGGL(cost_kernel<4>, dim3(P.g.nblk_obs), dim3(kBlock), 0, c->stream, P.g, P.b, 0, P.b.part);
  else
    hipLaunchKernelGGL(cost_kernel<2>, dim3(P.g.nblk_obs), dim3(kBlock), 0, c->stream, P.g, P.b, 0, P.b.part);
  ME_TRY(me_check_launch(c, "cost_kernel"));
  ME_HIP(c, hipMemcpyAsync(part.data(), P.b.part, 8 * part.size(), hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  double s = 0;
  for (double v : part) s += v;
  *cost = s;
  return ME_OK;
}

extern "C" int me_ba_evaluate(me_ctx* c, const me_ba_problem* p, double* res, double* Jc, double* Jp) {
  if (!c || !p) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  me_ba_options o;
  me_ba_default_options(&o);
  Plan P;
  ME_CHECK(c, p->mem == ME_HOST, "BA: evaluation helpers take host arrays");
  int rc = plan_build(c, p, &o, P, 0);
  if (rc < 0) return rc;
  const int no = P.g.no;
  void* d;
  const size_t od = P.g.od;
  ME_TRY(me_scratch(c, SLOT_GENERIC, 8 * 10 * od * (size_t)std::max(no, 1), &d));
  double* dres = (double*)d;
  double* djc = dres + od * (size_t)no;
  double* djp = djc + 6 * od * (size_t)no;
  if (od == 4)
    hipLaunchKernelGGL(eval_kernel<4>, dim3(blocks(no, kBlock)), dim3(kBlock), 0, c->stream, P.g, P.b, dres, djc, djp);
  else
    hipLaunchKernelGGL(eval_kernel<2>, dim3(blocks(no, kBlock)), dim3(kBlock), 0, c->stream, P.g, P.b, dres, djc, djp);
  ME_TRY(me_check_launch(c, "eval_kernel"));
  ME_HIP(c, hipMemcpyAsync(res, dres, 8 * od * (size_t)no, hipMemcpyDeviceToHost, c->stream));
  if (Jc) ME_HIP(c, hipMemcpyAsync(Jc, djc, 8 * 6 * od * (size_t)no, hipMemcpyDeviceToHost, c->stream));
  if (Jp) ME_HIP(c, hipMemcpyAsync(Jp, djp, 8 * 3 * od * (size_t)no, hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  return ME_OK;
}

extern "C" int me_ba_reduced_system(me_ctx* c, const me_ba_problem* p, double radius, double* S, double* bout) {
  if (!c || !p) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  me_ba_options o;
  me_ba_default_options(&o);
  o.initial_trust_region_radius = radius;
  Plan P;
  ME_CHECK(c, p->mem == ME_HOST, "BA: evaluation helpers take host arrays");
  int rc = plan_build(c, p, &o, P, 0);
  if (rc < 0) return rc;
  P.full_S = true;
  const Geo& g = P.g;
  ME_TRY(enqueue_linearize(P));
  ME_TRY(enqueue_assemble(P));
  std::vector<double> Sh((size_t)g.n6 * g.n6 + 2 * g.n6);
  if (g.m > 0)
    ME_HIP(c, hipMemcpyAsync(Sh.data(), P.b.S, 8 * Sh.size(), hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  const int n = g.n6;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double v = Sh[(size_t)i * n + j];
      if (i == j) v += std::min(std::max(Sh[(size_t)n * n + n + i], o.min_lm_diagonal), o.max_lm_diagonal) / radius;
      S[(size_t)i * n + j] = v;
    }
  for (int i = 0; i < n; ++i) bout[i] = Sh[(size_t)n * n + i];
  return ME_OK;
}

extern "C" int me_ba_covariance(me_ctx* c, const me_ba_problem* p, double* cov, int* ok) {
  if (!c || !p || !cov || !ok) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  me_ba_options o;
  me_ba_default_options(&o);
  o.jacobi_scaling = 0;                  // S unscaled: its inverse is the covariance directly
  o.initial_trust_region_radius = INFINITY;  // D / radius = 0: no LM damping
  Plan P;
  ME_CHECK(c, p->mem == ME_HOST, "BA: evaluation helpers take host arrays");
  int rc = plan_build(c, p, &o, P, 0);
  if (rc < 0) return rc;
  P.full_S = true;
  const Geo& g = P.g;
  hipLaunchKernelGGL(cov_prep_kernel, dim3(1), dim3(1), 0, c->stream, P.b);
  ME_TRY(enqueue_linearize(P));
  ME_TRY(enqueue_assemble(P));
  void* d;
  const size_t nx = (size_t)g.n6 * g.n6;
  ME_TRY(me_scratch(c, SLOT_GENERIC, 8 * (nx + 36 * (size_t)g.nc) + 64, &d));
  double* X = (double*)d;
  double* dcov = X + nx;
  int* dok = (int*)(dcov + 36 * (size_t)g.nc);
  hipLaunchKernelGGL(cov_kernel, dim3(1), dim3(kCovBlock), 0, c->stream, g, P.b, X, dcov, dok);
  ME_TRY(me_check_launch(c, "cov_kernel"));
  std::vector<double> h(36 * (size_t)g.nc);
  int hok = 0;
  ME_HIP(c, hipMemcpyAsync(h.data(), dcov, 8 * h.size(), hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipMemcpyAsync(&hok, dok, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  *ok = hok;
  if (hok) std::memcpy(cov, h.data(), 8 * h.size());
  return ME_OK;
}

// The window covariance of p queued on the ctx stream into the covariance's scratch (out: camera blocks | failure
// words | landmark blocks when want_pts); the caller takes the blocks from there.  g: the plan's geometry.
static int cov_enqueue(me_ctx* c, const me_ba_problem* p, bool want_pts, CovOut& out, Geo& gout) {
  me_ba_options o;
  me_ba_default_options(&o);
  o.jacobi_scaling = 0;                      // as me_ba_covariance: S unscaled, no LM damping
  o.initial_trust_region_radius = INFINITY;
  Plan P;
  P.cov = true;
  const bool dev = p->mem == ME_DEVICE;
  int rc = plan_build(c, p, &o, P, dev ? kCovSet : 0);
  if (rc < 0) return rc;
  P.full_S = true;
  const Geo& g = P.g;
  gout = g;
  ME_CHECK(c, g.n6 <= kCovMaxN, "BA covariance: %d variable cameras exceed the factor's workspace", g.m);
  ME_TRY(cov_out(c, g, out));
  hipStream_t s = c->stream;
  ME_HIP(c, hipMemsetAsync(out.fail, 0, 2 * sizeof(int), s));
  hipLaunchKernelGGL(cov_prep_kernel, dim3(1), dim3(1), 0, s, P.b);
  ME_TRY(enqueue_linearize(P));
  ME_TRY(enqueue_assemble(P));
  if (g.n6 <= kCovLdsMaxN) {
    if (!c->ba_cov_lds_attr) {
      ME_HIP(c, hipFuncSetAttribute((const void*)cov_full_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)cov_lds_bytes(kCovLdsMaxN)));
      c->ba_cov_lds_attr = 1;
    }
    hipLaunchKernelGGL(cov_full_kernel<true>, dim3(1), dim3(kCovFullBlock), cov_lds_bytes(g.n6), s, g, P.b, out.Sig,
                       out.cam, out.fail);
  } else {
    hipLaunchKernelGGL(cov_full_kernel<false>, dim3(1), dim3(kCovFullBlock), 0, s, g, P.b, out.Sig, out.cam, out.fail);
  }
  if (want_pts && g.np > 0) {
    const int nb = blocks(g.np, kCovPtBlock / kCovPtLanes);
    if (g.od == 4)
      hipLaunchKernelGGL(cov_points_kernel<4>, dim3(nb), dim3(kCovPtBlock), 0, s, g, P.b, (const double*)out.Sig, P.b.Wo,
                         out.pt, out.fail);
    else
      hipLaunchKernelGGL(cov_points_kernel<2>, dim3(nb), dim3(kCovPtBlock), 0, s, g, P.b, (const double*)out.Sig, P.b.Wo,
                         out.pt, out.fail);
  }
  return me_check_launch(c, "BA covariance");
}

extern "C" int me_ba_covariance_full(me_ctx* c, const me_ba_problem* p, double* cam_cov, double* pt_cov, int* ok) {
  me_range range_("me_ba_covariance_full");
  if (!c || !p || !ok || (!cam_cov && !pt_cov)) return ME_ERR_INVALID;
  ME_HIP(c, hipSetDevice(c->device));
  CovOut out;
  Geo g;
  ME_TRY(cov_enqueue(c, p, pt_cov != nullptr, out, g));
  const bool dev = p->mem == ME_DEVICE, pts = pt_cov && g.np > 0;
  hipStream_t s = c->stream;
  const long ncam = 36L * g.nc, npt = pts ? 9L * g.np : 0;
  if (dev) {  // asynchronous: the caller's device arrays and ok word, behind everything queued here
    hipLaunchKernelGGL(cov_commit_kernel, dim3(blocks(std::max(ncam, npt), kBlock)), dim3(kBlock), 0, s,
                       (const int*)out.fail, (const double*)out.cam, cam_cov, ncam, (const double*)out.pt, pt_cov, npt,
                       ok);
    return me_check_launch(c, "cov_commit_kernel");
  }
  void* hp;  // (a larger staging than the plan's: me_pinned waits for the queued input copy before it reallocates)
  const size_t out_bytes = 8 * (size_t)(ncam + 1 + npt);  // cam | fail | the landmark blocks that were computed
  ME_TRY(me_pinned(c, out_bytes, &hp));
  const double* h = (const double*)hp;
  ME_HIP(c, hipMemcpyAsync(hp, out.cam, out_bytes, hipMemcpyDeviceToHost, s));
  ME_HIP(c, hipStreamSynchronize(s));
  int fail[2];
  std::memcpy(fail, h + ncam, sizeof fail);
  *ok = !fail[0] && !fail[1];
  if (*ok) {
    if (cam_cov) std::memcpy(cam_cov, h, 8 * (size_t)ncam);
    if (pts) std::memcpy(pt_cov, h + ncam + 1, 8 * (size_t)npt);
  }
  return ME_OK;
}

extern "C" int me_ba_point_check(me_ctx* c, const me_ba_problem* p, const me_ba_point_check_params* params, double* chi2,
                                 uint8_t* flags, int* n_flagged) {
  me_range range_("me_ba_point_check");
  if (!c || !p || !flags) return ME_ERR_INVALID;
  me_ba_point_check_params prm;
  me_ba_point_check_default_params(&prm);
  if (params) prm = *params;
  if (const char* why = me_ba_point_check_check(&prm)) return me_set_error(c, ME_ERR_INVALID, "me_ba_point_check: %s", why);
  const bool dev = p->mem == ME_DEVICE;
  ME_CHECK(c, !dev || !n_flagged, "me_ba_point_check: n_flagged is a host result (NULL for a device-resident problem)");
  ME_HIP(c, hipSetDevice(c->device));
  me_ba_options o;
  me_ba_default_options(&o);
  Plan P;
  P.cov = true;  // (as the covariance: a device-resident problem's plan in set kCovSet, no drain, no staging)
  ME_TRY(plan_build(c, p, &o, P, dev ? kCovSet : 0));
  const Geo& g = P.g;
  if (dev) return me_ba_check_launch(c, g, P.b, p->cams, p->pts, &prm, chi2, flags);
  if (n_flagged) *n_flagged = 0;
  if (g.np == 0) {
    ME_HIP(c, hipStreamSynchronize(c->stream));  // (the plan reads the caller's staging)
    return ME_OK;
  }
  void* d;
  ME_TRY(me_scratch(c, kCheckOutSlot, 9 * (size_t)g.np + 8, &d));
  double* dchi2 = (double*)d;
  uint8_t* dflags = (uint8_t*)(dchi2 + g.np);
  ME_TRY(me_ba_check_launch(c, g, P.b, P.b.cams[0], P.b.pts[0], &prm, dchi2, dflags));
  if (chi2) ME_HIP(c, hipMemcpyAsync(chi2, dchi2, 8 * (size_t)g.np, hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipMemcpyAsync(flags, dflags, (size_t)g.np, hipMemcpyDeviceToHost, c->stream));
  ME_HIP(c, hipStreamSynchronize(c->stream));
  if (n_flagged)
    for (int i = 0; i < g.np; ++i) *n_flagged += flags[i] != 0;
  return ME_OK;
}

extern "C" int me_ba_window_indices(me_ctx* c, const int32_t* frame, const int32_t* ids, int n_obs, int first_frame,
                                    const int32_t* win_ids, int n_pts, int32_t* cam_idx, int32_t* pt_idx) {
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, n_obs >= 0 && n_pts >= 0, "me_ba_window_indices: bad sizes");
  if (n_obs == 0) return ME_OK;
  ME_HIP(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(window_indices_kernel, dim3(blocks(n_obs, kBlock)), dim3(kBlock), 0, c->stream, frame, ids, n_obs,
                     first_frame, win_ids, n_pts, cam_idx, pt_idx);
  return me_check_launch(c, "window_indices_kernel");
}

// The test hook (not part of the drop-in ABI): the ctx's hook word, any
// combination of the kHookMask bits (me_internal.hpp); 0 clears it.  Any other
// bit is refused and leaves the word as it was.
//    512 kFlagAsmTimeout      the fused-assembly wait of the camera solve times out
//                             (tests/test_distributed.py: a hand-off timeout on one rank of a sharded solve)
//   1024 kFlagSolveFail       every camera solve fails: each LM step invalid, the solve ends with
//                             termination 2 after max_num_consecutive_invalid_steps
//   2048 kFlagFailEveryOther  that, for every second solve queued on the ctx
//                             (tests/test_pipeline.py: the chained window start after a failed BA)
//   8192 kFlagRosterNow       every roster on the ctx closes at once: the scale LM, the camera solve's
//                             workers and fused assemblers (tests/test_gpu_configs.py roster tests)
//  16384 kFlagSeparateAsm     S assembly in its own launch, not inside the camera solve's
//                             (tests/test_gpu_configs.py test_ba_fused_assembly_identical)
//  32768 kFlagMiLane          the one-lane-per-pair MI kernel instead of the quad kernel
//                             (tests/test_gpu_parity.py test_mi_lane_kernel_still_bit_exact)
extern "C" int me_debug_solve_flags(me_ctx* c, int flags) {
  if (!c) return ME_ERR_INVALID;
  ME_CHECK(c, (flags & ~kHookMask) == 0, "me_debug_solve_flags: 0x%x holds bits that are no test hook (accepted: 0x%x)",
           (unsigned)flags, (unsigned)kHookMask);
  c->dbg_solve_flags = flags;
  c->dbg_solve_count = 0;
  return ME_OK;
}

extern "C" int me_debug_read(me_ctx* c, long long* out, int n) {
  if (!c || n < 0 || n > 16) return ME_ERR_INVALID;
  std::memcpy(out, c->dbg, 8 * (size_t)n);
  return ME_OK;
}

#ifdef ME_CAM_TS
extern "C" int me_cam_ts(long long* out, int reset) {
  unsigned long long h[8];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_cam_ts), sizeof h) != hipSuccess) return -1;
  for (int i = 0; i < 8; ++i) out[i] = (long long)h[i];
  if (reset) {
    const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_cam_ts), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
// the unit whose workgroup is stamped (index into the plan's unit table)
extern "C" int me_cam_ts_unit(int unit) {
  if (unit < 0) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_cam_ts_unit), &unit, sizeof unit) == hipSuccess ? 0 : -1;
}
#endif

#ifdef ME_STEP_TS
extern "C" int me_step_ts(long long* out, int reset) {
  unsigned long long h[12];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_step_ts), sizeof h) != hipSuccess) return -1;
  for (int i = 0; i < 12; ++i) out[i] = (long long)h[i];
  if (reset) {
    const unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_step_ts), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif
