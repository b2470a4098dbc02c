"""GPU workload drivers for profiling and A/B timing (run on the GPU box,
usually through tools/gpu.sh): each subcommand runs one hot-path workload of
the bench's configurations and prints its timing; `--lib LIB` (or ME_LIB)
loads another build of libme_hip.so (tools/build_variant.sh).

  ba_wall [CONFIGS]      wall time of one 10-iteration BA solve (configs 3,4,5 or NFxW at 1280x720)
  klt [--reps --check]   klt_kernel on the config-3 frame (2000 features), bit-exact check vs the oracle
  mi [--pairs --reps --check]
                         batch MI kernel (1M 11x11 pairs), self-check vs the group kernel
  coop [--reps]          scale LM (config 3) and config-5 BA wall clocks (tools/gpu.sh coop: plain vs
                         cooperative launch build)
  solve_ts               cam_solve_kernel phase stamps (a -DME_SOLVE_TS build), configs 3 and 5
  scale_ts [--front F]   persistent scale LM phase split (a -DME_SCALE_TS build)
  schur_stamps           pt_schur_kernel workgroup-0 stamps (a -DME_SCHUR_STAMPS build)
  corners [--reps --loop N]
                         corner detector kernels (1280x720, 3840x2160) and the config-3 native loop with
                         detector 0 / 1, alternating
  klt_fb [--reps --repeats --check --loop N]
                         me_klt_track_fb beside me_klt_track on the config-3 frame (2000 features), alternating
                         in one process, and the config-3 native loop with klt_fb_max 0 / 0.5, alternating
  klt_guided [--reps --repeats --check --guess G --loop N --fast N]
                         me_klt_track_guided beside me_klt_track on the config-3 frame (2000 features; the guess is
                         the unguided result moved by up to 2 px), alternating in one process, the config-3
                         native loop with klt_predict off / on, alternating, and (--fast N, CPU only, no
                         device touched) the oracle-backend loop off / on over every 6th keyframe of the arc
  match_lr [--reps --repeats --check --loop N --plain-only]
                         me_mi_epipolar_match_lr beside me_mi_epipolar_match on a config-3 stereo pair (2000
                         tracked-form and 250 new-form features), alternating in one process, and the config-3
                         native loop with match_lr_max 0 / 1, alternating
  rectify [--reps --check --loop N]
                         me_rectify_map and me_remap_q5 (1280x720, 3840x2160) through a realistic camera's map,
                         beside the library's streaming copy of the same bytes, and the config-3 native loop
                         with the rectifier off / on (padded frames cropped back), alternating
  clahe [--reps --check --loop N]
                         me_clahe (1280x720, 3840x2160; noise and a 16-level low-contrast image, 8x8 tiles), the
                         table kernel and the apply kernel apart, beside the library's streaming copy of the same
                         bytes, and the config-3 native loop with the equaliser off / on, alternating
  tonemap [--reps --check --loop N]
                         me_tonemap16 (640x480, 1280x720, 3840x2160; 14-bit noise and a 16-level low-entropy
                         image), the coarse select apart from fine select + apply, beside the library's streaming
                         copy of the same bytes, and the config-3 native loop on the 8-bit stream / on its 16-bit
                         twin through me_vo_loop_process16, alternating
  motion_gate [--reps --repeats --check --loop N]
                         me_motion_gate on 2000 synthetic stereo tracks at 1280x720 (a fifth on a second body, 0.25 px
                         noise, the default parameters): HIP-event time of its three launches and the wall time per
                         call, and the config-3 native loop with the gate off / on, alternating
  frame_pose [--reps --repeats --check --trace --loop N]
                         me_frame_pose on 2000 synthetic features at 1280x720 (a fifth gross outliers, 0.3 px noise,
                         the default parameters): HIP-event time of a call's seven launches and the wall time per
                         call, me_kf_update and me_motion_gate on the same features beside it, and a config-3 push loop over N camera frames (three per keyframe
                         step of the arc) with the frame pose off / on, alternating.  --trace 1: the calls alone,
                         no event timing (the run rocprofv3 --kernel-trace --stats wraps)
  window_cov [CONFIGS --reps --repeats --trace --loop N]
                         me_ba_covariance beside me_ba_covariance_full (cameras only / with landmarks, host and
                         device-resident form) on the configs' windows (3,5) after a 10-iteration solve: wall time
                         per call, and the config-3 native loop with the covariance switch off / cameras /
                         cameras and landmarks, alternating.  --trace 1: the calls alone (under rocprofv3
                         --kernel-trace --stats)
  track_check [--repeats --loop N --kernel-time 0|1]
                         the config-3 native loop over N keyframes with the residual check behind every window
                         solve off / on, alternating, same build: keyframes/s, the ME_KT_BA_CHECK time per launch
                         and the tracks flagged
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup(lib):
    import torch  # noqa: F401  (device runtime up before the library)

    from uasl_motion_estimation_amd import _lib
    if lib:
        _lib.load_library(lib)
    from uasl_motion_estimation_amd._lib import Context
    return Context(0)


def _ba_problem(c):
    from uasl_motion_estimation_amd import synthetic as S
    if "x" in c:  # NFEATSxWINDOW at 1280x720
        nf, w = (int(v) for v in c.split("x"))
        return S.ba_problem(S.SEED0 * 7 + w, nf, w, 1280, 720)
    cfg = S.CONFIGS[int(c)]
    return S.ba_problem(S.SEED0 * 7 + int(c), cfg["n_feats"], cfg["window"], cfg["width"], cfg["height"])


def cmd_ba_wall(a):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions
    ctx = _setup(a.lib)
    out = {}
    for c in a.configs.split(","):
        d = DeviceBAProblem(_ba_problem(c), ctx)
        o = SolverOptions.fixed_iterations(10)
        for _ in range(3):
            d.reset()
            s = d.solve(o)
        best = []
        for _ in range(3):
            ctx.synchronize()
            w0 = time.perf_counter()
            for _ in range(20):
                d.reset()
                s = d.solve(o)
            ctx.synchronize()
            best.append((time.perf_counter() - w0) / 20 * 1e3)
        out[c] = {"ms": round(min(best), 4), "iterations": s["iterations"], "cost": s["final_cost"]}
    print(json.dumps(out))


def cmd_klt(a):
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd._lib import ME_DEVICE
    from uasl_motion_estimation_amd.klt import klt_params
    ctx = _setup(a.lib)
    W, H, N = 1280, 720, 2000
    scene, K, stream = S.stereo_stream(20261018, W, H, 2)
    pts = S.grid_features(np.random.default_rng(0), N, W, H, 12).astype(np.float32)
    dp, dn, din, dout, dst = ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(8 * N), ctx.malloc(8 * N), ctx.malloc(N)
    L0, L1 = np.ascontiguousarray(stream[0].left), np.ascontiguousarray(stream[1].left)
    ctx.h2d(dp, L0)
    ctx.h2d(dn, L1)
    ctx.h2d(din, pts)
    kp = klt_params()

    def run():
        ctx.check(ctx.lib.me_klt_track(ctx.h, ME_DEVICE, ctypes.c_void_p(dp), ctypes.c_void_p(dn), W, H, W,
                                       ctypes.c_void_p(din), ctypes.c_void_p(dout), ctypes.c_void_p(dst), N,
                                       ctypes.byref(kp)), "klt")
    for _ in range(3):
        run()
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing(True, ["KLT"])
    for _ in range(a.reps):
        run()
    ctx.synchronize()
    ctx.timing(False)
    cnt, ms = ctx.timing_read("KLT")
    print(f"klt_kernel: {1000 * ms / max(cnt, 1):.2f} us/launch ({N} features, {W}x{H})", flush=True)
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle as O  # checker only
        got, gst = np.zeros(2 * N, np.float32), np.zeros(N, np.uint8)
        ctx.d2h(got, dout)
        ctx.d2h(gst, dst)
        ref_pts, ref_st = O.klt(L0, L1, pts)
        same = np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref_pts, np.float32).ravel().view(np.uint32)) \
            and np.array_equal(gst, ref_st)
        print(f"klt parity vs oracle: {'bit-exact' if same else 'MISMATCH'}", flush=True)
        if not same:
            sys.exit(1)


def cmd_mi(a):
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd.mutual_information import mi_scores_device
    ctx = _setup(a.lib)
    cfg = S.CONFIGS[3]
    scene, K, stream = S.stereo_stream(S.SEED0 + 3, cfg["width"], cfg["height"], 2)
    L, R = np.ascontiguousarray(stream[1].left), np.ascontiguousarray(stream[1].right)
    H, W = L.shape
    n = a.pairs
    rng = np.random.default_rng(7)
    xyL = np.stack([rng.integers(0, W - 11, n), rng.integers(0, H - 11, n)], -1).astype(np.int32)
    xyR = xyL.copy()
    xyR[:, 0] = np.clip(xyL[:, 0] - rng.integers(0, 40, n), 0, W - 11)
    dLi, dRi = ctx.malloc(L.nbytes), ctx.malloc(R.nbytes)
    ctx.h2d(dLi, L)
    ctx.h2d(dRi, R)
    dL, dR, dout = ctx.malloc(xyL.nbytes), ctx.malloc(xyR.nbytes), ctx.malloc(4 * n)
    ctx.h2d(dL, xyL)
    ctx.h2d(dR, xyR)
    run = lambda: mi_scores_device(ctx, dLi, W, dRi, W, W, H, dL, dR, n, (11, 11), dout)  # noqa: E731
    run()
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing(True)
    for _ in range(a.reps):
        run()
    ctx.synchronize()
    ctx.timing(False)
    cnt, ms = ctx.timing_read("MI")
    avg = ms / cnt
    print("pairs %d  avg %.4f ms  %.3f Gpairs/s  %.1f GB/s (262 B/pair)  frac %.4f" %
          (n, avg, n / avg / 1e6, 262 * n / avg / 1e6, 262 * n / avg / 1e6 / 8000), flush=True)
    if a.check:
        got = np.zeros(n, np.float32)
        ctx.d2h(got, dout)
        m = min(n, 200000)
        ref = np.zeros(m, np.float32)
        for s in range(0, m, 30000):  # below the batch kernel's threshold: the group kernel (parity-tested)
            e = min(m, s + 30000)
            mi_scores_device(ctx, dLi, W, dRi, W, W, H, dL + 8 * s, dR + 8 * s, e - s, (11, 11), dout + 4 * s)
        ctx.synchronize()
        ctx.d2h(ref, dout)
        bad = np.flatnonzero(got[:m].view(np.uint32) != ref.view(np.uint32))
        print("self-check vs group kernel on %d pairs: %d mismatches" % (m, len(bad)))
        if len(bad):
            sys.exit(1)


def cmd_coop(a):
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd.optimisation import (DeviceBAProblem, OptimisationParams, SolverOptions,
                                                         scale_optimise)
    ctx = _setup(a.lib)
    cfg = S.CONFIGS[3]
    seed = S.SEED0 + 3
    scene, K, stream = S.stereo_stream(seed, cfg["width"], cfg["height"], 2)
    sp = S.scale_problem(seed, cfg["width"], cfg["height"], cfg["n_feats"], window=cfg["window"], w=5,
                         frames=stream[:2], scene=scene)
    out = {"lib": a.lib or os.environ.get("ME_LIB", "tree")}
    for _ in range(3):
        r = scale_optimise(sp, OptimisationParams(), ctx=ctx)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        r = scale_optimise(sp, OptimisationParams(), ctx=ctx)
    out["scale_lm_ms"] = round((time.perf_counter() - t0) / a.reps * 1e3, 4)
    out["scale_lm"] = {k: r[k] for k in ("iterations", "res_evals", "rejections")}
    d = DeviceBAProblem(_ba_problem("5"), ctx)
    o = SolverOptions.fixed_iterations(10)
    for _ in range(3):
        d.reset()
        s = d.solve(o)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        d.reset()
        s = d.solve(o)
    ctx.synchronize()
    out["ba_config5_ms"] = round((time.perf_counter() - t0) / a.reps * 1e3, 4)
    out["ba_config5_iterations"] = s["iterations"]
    print(json.dumps(out))


def cmd_solve_ts(a):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve
    ctx = _setup(a.lib)
    fn = ctx.lib.me_solve_ts
    fn.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 24)()
    names = {1: "lin_finalize", 2: "asm_wait", 11: "ts_asm_probe", 12: "load_issue", 13: "load_diag_barrier",
             3: "load_rest", 4: "factor", 5: "backward", 6: "tail", 8: "asm_last_exit", 9: "asm_first_entry",
             19: "f_diag0", 16: "f_w0_panel", 17: "f_w0_diag", 18: "f_barrier_wait"}
    names5 = {**names, 16: "m2_w0_diag", 17: "m2_count_wait", 18: "m2_panel", 19: "m2_drain_publish"}
    for c in a.configs.split(","):
        bp = _ba_problem(c)
        for _ in range(3):
            ba_solve(bp.copy(), SolverOptions.fixed_iterations(10), ctx=ctx)
        fn(buf, 1)
        for _ in range(20):
            ba_solve(bp.copy(), SolverOptions.fixed_iterations(10), ctx=ctx)
        fn(buf, 1)
        calls = max(buf[15], 1)
        us = {nm: round(buf[i] / calls / 100.0, 2) for i, nm in (names5 if c == "5" else names).items()}
        tot = sum(buf[i] for i in (1, 2, 3, 4, 5, 6, 11, 12, 13, 16, 17, 18, 19)) / calls / 100.0
        print(f"config {c}: calls {calls} us/launch {us} wg0 total {tot:.2f} us", flush=True)


def cmd_scale_ts(a):
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd._lib import cu_split
    from uasl_motion_estimation_amd.optimisation import OptimisationParams, ScaleCall
    import torch
    ctx = _setup(a.lib)
    if a.front:  # the bench's front-end share: front of every 16 CUs, whole XCDs
        ctx.set_cu_mask(cu_split(torch.cuda.get_device_properties(0).multi_processor_count, a.front)[0])
    fn = ctx.lib.me_scale_ts
    fn.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 16)()
    cfg = S.CONFIGS[3]
    W, H, N, win = cfg["width"], cfg["height"], cfg["n_feats"], cfg["window"]
    seed = S.SEED0 + 3
    scene, K, stream = S.stereo_stream(seed, W, H, 3)
    sp = S.scale_problem(seed, W, H, N, window=win, w=5, frames=stream[:2], scene=scene)
    params = OptimisationParams.fixed_iterations(10)
    for rep in range(2):
        fn(buf, 1)
        for _ in range(3 if rep == 0 else 20):
            c = ScaleCall(sp, params, ctx=ctx)
            c.run()
            r = c.result()
        evals = r["executed_evals"] * N
        fn(buf, 1)
    L = max(buf[1], 1)
    us = lambda k: round(buf[k] / L / 100.0, 2)  # noqa: E731
    print(f"front_cus {a.front or 16}/16: launches {buf[1]}, phases/launch {buf[0] / L:.1f} "
          f"(A/D {buf[7] / L:.1f}, B {buf[8] / L:.1f}, C {buf[9] / L:.1f}); executed track evaluations/launch {evals}")
    print(f"  wall {us(2)} us/launch: wg0 track work A/D {us(3)} B {us(4)} C {us(5)}; wg0 waits for control {us(6)}; "
          f"control (reduce + decide) {us(10)} over {buf[11] / L:.1f} reductions")
    n7 = max(buf[7], 1)
    print(f"  A/D controls: acquire {buf[12] / n7 / 100:.2f}, reduce {buf[13] / n7 / 100:.2f}, "
          f"control {buf[14] / n7 / 100:.2f}, publish {buf[15] / n7 / 100:.2f} us")
    print(f"  ns per executed track evaluation: {1e3 * buf[2] / L / 100.0 / max(evals, 1):.2f}")


def cmd_cam_ts(a):
    """One camera-assembly unit's workgroup phases (a -DME_CAM_TS=1 build): the
    slot pass (loads + residual/Jacobian + sums), block_sum<27>, partial stores +
    arrival, and (when last) the camera reduce; s_memtime ticks per execution.
    Reported for unit 0 (the first variable camera's first 256 slots: the
    lightest camera of a sliding window) and for the first unit of the heaviest
    camera (a full unit whose camera has the most partials to reduce)."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions
    ctx = _setup(a.lib)
    fn = ctx.lib.me_cam_ts
    fn.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 8)()
    bp = _ba_problem(a.config)
    counts = np.bincount(bp.cam_idx, minlength=len(bp.cams))[bp.fixed_frames:]
    units = np.maximum(1, -(-counts // 256))
    heavy = int(np.argmax(counts))
    first = np.concatenate([[0], np.cumsum(units)])
    d = DeviceBAProblem(bp, ctx)
    o = SolverOptions.fixed_iterations(10)
    out = {"camera_counts": counts.tolist(), "units": int(units.sum())}
    set_unit = getattr(ctx.lib, "me_cam_ts_unit", None)  # (a build from before the unit table stamps camera (0, 0) only)
    for tag, unit in (("unit0", 0), (f"heaviest_camera{heavy}_unit{int(first[heavy])}", int(first[heavy]))):
        if set_unit is None and unit:
            break
        if set_unit is not None and set_unit(unit) != 0:
            sys.exit("me_cam_ts_unit failed")
        for _ in range(3):
            d.reset()
            d.solve(o)
        ctx.synchronize()
        fn(buf, 1)
        for _ in range(20):
            d.reset()
            d.solve(o)
        ctx.synchronize()
        fn(buf, 0)
        n = max(buf[0], 1)
        out[tag] = {"executions": buf[0], "slot_pass": round(buf[1] / n), "block_sum27": round(buf[2] / n),
                    "store_arrive": round(buf[3] / n), "times_last": buf[5],
                    "reduce_when_last": round(buf[4] / max(buf[5], 1))}
    print(json.dumps(out))


def cmd_step_ts(a):
    """pt_step workgroup 0's phases and the finalizing workgroup's tail (a
    -DME_STEP_TS=1 build), s_memtime ticks per launch."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions
    ctx = _setup(a.lib)
    fn = ctx.lib.me_step_ts
    fn.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 12)()
    d = DeviceBAProblem(_ba_problem(a.config), ctx)
    o = SolverOptions.fixed_iterations(10)
    for _ in range(3):
        d.reset()
        d.solve(o)
    ctx.synchronize()
    fn(buf, 1)
    for _ in range(20):
        d.reset()
        d.solve(o)
    ctx.synchronize()
    fn(buf, 0)
    n = max(buf[0], 1)
    nf = max(buf[7], 1)
    names = ["issue", "slot_sums", "point_solve", "cand_cost", "blocksum_store"]
    out = {k: round(buf[i + 1] / n) for i, k in enumerate(names)}
    out["launches"] = buf[0]
    out["finalize"] = round(buf[6] / nf)
    out["fin_loads"], out["fin_blocksum"], out["fin_decide"] = (round(buf[k] / nf) for k in (8, 9, 10))
    print(json.dumps(out))


def cmd_schur_stamps(a):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve
    ctx = _setup(a.lib)
    ctx.lib.me_debug_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    for c in a.configs.split(","):
        ba_solve(_ba_problem(c), SolverOptions.fixed_iterations(10), ctx=ctx)
        buf = (ctypes.c_longlong * 16)()
        ctx.lib.me_debug_read(ctx.h, buf, 16)
        calls = max(buf[12], 1)
        print("config", c, "pt_schur wg0 ticks/launch:", {nm: round(buf[i] / calls) for i, nm in
              zip([6, 7, 8, 9, 10], ["loads", "sums+chol", "Y+barrier", "mfma", "tail+stores"])}, "launches", calls,
              flush=True)


def cmd_corners(a):
    """The corner detector (csrc/corners.hip): me_corner_response and
    me_vo_new_corners per launch (ME_KT_CORNERS events) at 1280x720 and
    3840x2160 with 2000 tracked features on the config-3 grid, then (--loop N)
    the native VO loop at config 3 over N keyframes with detector 0 and 1,
    alternating, two repeats each."""
    import math

    import torch

    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd._lib import ME_DEVICE
    from uasl_motion_estimation_amd.corners import corner_params
    ctx = _setup(a.lib)
    V = ctypes.c_void_p
    out = {"note": "algorithmic bytes = w*h read + 8*w*h written (the map); the kernels stage, difference and sum "
                   "in LDS and registers, so the expected bound is LDS / VALU, not HBM", "kernels": {}}
    for W, H in ((1280, 720), (3840, 2160)):
        _, fr = S.corridor_frames_torch(S.SEED0 + 3, W, H, 0, 1)
        L = fr[0][0].contiguous()
        torch.cuda.synchronize()
        n, nf = 2000, 2000
        aw, ah = W - 2 * PL.MARGIN, H - 2 * PL.MARGIN
        nx = max(1, int(round(math.sqrt(nf * aw / ah))))
        ny = max(1, int(math.ceil(nf / nx)))
        cw, ch = aw / nx, ah / ny
        rng = np.random.default_rng(0)
        uv = np.stack([rng.uniform(PL.MARGIN, W - PL.MARGIN, n), rng.uniform(PL.MARGIN, H - PL.MARGIN, n)], -1)
        d_map, d_uv, d_st, d_out = ctx.malloc(8 * W * H), ctx.malloc(8 * n), ctx.malloc(2 * n), ctx.malloc(16 + 12 * nf)
        ctx.h2d(d_uv, uv.astype(np.float32))
        st = np.ones(2 * n, np.uint8)
        st[:n:8] = 0  # every 8th track lost: its cell is free unless another feature holds it
        ctx.h2d(d_st, st)
        p = corner_params()

        def response():
            ctx.check(ctx.lib.me_corner_response(ctx.h, ME_DEVICE, V(L.data_ptr()), W, H, W, ctypes.byref(p),
                                                 V(d_map)), "me_corner_response")

        def new_corners():
            ctx.check(ctx.lib.me_vo_new_corners(ctx.h, V(L.data_ptr()), W, H, W, V(d_uv), V(d_st), V(d_st + n), n,
                                                float(PL.MARGIN), nx, ny, cw, ch, nf, 2, ctypes.byref(p),
                                                V(d_out + 16), V(d_out + 16 + 8 * nf), V(d_out)), "me_vo_new_corners")
        for name, fn in (("me_corner_response", response), ("me_vo_new_corners", new_corners)):
            for _ in range(5):
                fn()
            ctx.synchronize()
            ctx.timing_reset()
            ctx.timing(True, ["CORNERS"])
            for _ in range(a.reps):
                fn()
            ctx.synchronize()
            ctx.timing(False)
            cnt, ms = ctx.timing_read("CORNERS")
            us = 1000 * ms / max(cnt, 1)
            gbs = 9 * W * H / (us * 1e-6) / 1e9
            out["kernels"][f"{name} {W}x{H}"] = {"launches": cnt, "us_per_launch": round(us, 2),
                                                 "algorithmic_GBps": round(gbs, 1),
                                                 "fraction_of_8TBps": round(gbs / 8000, 4)}
            print(f"{name} {W}x{H}: {us:.2f} us/launch over {cnt} launches, {gbs:.0f} GB/s algorithmic "
                  f"({100 * gbs / 8000:.2f} % of 8 TB/s)", flush=True)
        cnt = np.zeros(1, np.int32)
        ctx.d2h(cnt, d_out)
        out["kernels"][f"me_vo_new_corners {W}x{H}"]["emitted"] = int(cnt[0])
        for d in (d_map, d_uv, d_st, d_out):
            ctx.free(d)
    if a.loop > 0:
        c, N = 3, a.loop
        arc = S.trajectory_arc(max(N, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, N, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, N - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for det in PL.DETECTORS:
                cfg = PL.PipelineConfig.from_config(c, detector=det)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(N if rep >= 0 else min(N, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"detector": det, "repeat": rep, "keyframes": N, "keyframes_per_s": round(N / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "new_mean": round(float(np.mean([q.n_new for q in res[2:]])), 1),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / N, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def cmd_klt_fb(a):
    """The forward-backward check (csrc/klt.hip, me_klt_track_fb) beside the
    plain tracker on cmd_klt's inputs: per call, the ME_KT_PYR events (pyramids
    and Scharr derivatives; the check adds the next pyramid's derivatives) and
    the ME_KT_KLT events (plain: klt_kernel; check: forward pass, backward
    pass and gate under one event pair), --repeats blocks of --reps calls
    each, the two entry points alternating.  Then (--loop N) the native VO
    loop at config 3 over N corridor keyframes with klt_fb_max 0 and 0.5,
    alternating, two repeats each."""
    import torch

    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd._lib import ME_DEVICE
    from uasl_motion_estimation_amd.klt import klt_params
    ctx = _setup(a.lib)
    V = ctypes.c_void_p
    W, H, N = 1280, 720, 2000
    scene, K, stream = S.stereo_stream(20261018, W, H, 2)
    pts = S.grid_features(np.random.default_rng(0), N, W, H, 12).astype(np.float32)
    dp, dn, din, dout, dst, derr = (ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(8 * N), ctx.malloc(8 * N),
                                    ctx.malloc(N), ctx.malloc(4 * N))
    L0, L1 = np.ascontiguousarray(stream[0].left), np.ascontiguousarray(stream[1].left)
    ctx.h2d(dp, L0)
    ctx.h2d(dn, L1)
    ctx.h2d(din, pts)
    kp = klt_params()

    def plain():
        ctx.check(ctx.lib.me_klt_track(ctx.h, ME_DEVICE, V(dp), V(dn), W, H, W, V(din), V(dout), V(dst), N,
                                       ctypes.byref(kp)), "me_klt_track")

    def fb():
        ctx.check(ctx.lib.me_klt_track_fb(ctx.h, ME_DEVICE, V(dp), V(dn), W, H, W, V(din), V(dout), V(dst), V(derr), N,
                                          ctypes.byref(kp), a.fb_max), "me_klt_track_fb")
    out = {"inputs": f"{W}x{H}, {N} features, fb_max {a.fb_max}", "reps": a.reps, "calls": []}
    for fn in (plain, fb):
        for _ in range(5):
            fn()
    ctx.synchronize()
    for rep in range(a.repeats):
        for name, fn in (("me_klt_track", plain), ("me_klt_track_fb", fb)):
            ctx.timing_reset()
            ctx.timing(True, ["KLT", "PYR"])
            w0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            ctx.synchronize()
            wall = (time.perf_counter() - w0) / a.reps * 1e6
            ctx.timing(False)
            r = {"call": name, "repeat": rep, "wall_us_per_call": round(wall, 2)}
            for fam in ("PYR", "KLT"):
                cnt, ms = ctx.timing_read(fam)
                r[f"{fam}_us_per_call"] = round(1000 * ms / max(cnt, 1), 2)
                r[f"{fam}_timed"] = cnt
            out["calls"].append(r)
            print(json.dumps(r), flush=True)
    got, gst, gerr = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8), np.zeros(N, np.float32)
    ctx.d2h(got, dout)
    ctx.d2h(gst, dst)
    ctx.d2h(gerr, derr)
    out["accepted"] = int(gst.sum())
    out["both_passes_tracked"] = int(np.isfinite(gerr).sum())
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle as O  # checker only
        fwd, fst = O.klt(L0, L1, pts)
        q, st, err = PL.klt_fb_host(O.klt, L0, L1, pts, a.fb_max)
        same = (np.array_equal(got.view(np.uint32), q.view(np.uint32)) and np.array_equal(gst, st)
                and np.array_equal(gerr.view(np.uint32), err.view(np.uint32)))
        out["forward_tracked"] = int(fst.sum())
        print(f"klt_fb parity vs oracle: {'bit-exact' if same else 'MISMATCH'} (forward {int(fst.sum())}, both passes "
              f"{out['both_passes_tracked']}, accepted {out['accepted']} of {N})", flush=True)
        if not same:
            sys.exit(1)
    for d in (dp, dn, din, dout, dst, derr):
        ctx.free(d)
    if a.loop > 0:
        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for fb_max in (0.0, a.fb_max):
                cfg = PL.PipelineConfig.from_config(c, klt_fb_max=fb_max)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"klt_fb_max": fb_max, "repeat": rep, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "new_mean": round(float(np.mean([q.n_new for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def _fast_sequence_cpu(n):
    """The oracle-backend loop (CPU) with klt_predict off and on over a fast
    sequence: every 6th pose of the arc (3 m and 1.8 deg per keyframe) rendered
    at config-1 size; mean tracked features and the final centre drift."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from pipeline_oracle import OracleBackend  # checker only

    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    c = 1
    cfg0 = S.CONFIGS[c]
    W, H = cfg0["width"], cfg0["height"]
    K = S.intrinsics(W, H)
    scene = S.CorridorScene(S.SEED0 + c, S.arc_radius())
    arc = S.trajectory_arc(6 * n)[::6]
    truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
    lut = S.tone_map()
    frames = [(S.render_corridor(scene, K, R, t, W, H, 0.0), lut[S.render_corridor(scene, K, R, t, W, H, S.BASELINE)])
              for (R, t) in arc]
    runs = []
    for on in (False, True):
        cfg = PL.PipelineConfig.from_config(c, klt_predict=on)
        vo = PL.WindowedStereoVO(cfg, OracleBackend(), K, truth[0], truth[1] - truth[0])
        for t in range(n):
            vo.process(t, *frames[t])
        vo.finish()
        drift = float(np.linalg.norm(PL.camera_centre(vo.poses[n - 1]) - PL.camera_centre(truth[n - 1])))
        r = {"cpu_oracle_backend": True, "klt_predict": on, "keyframes": n,
             "tracked_mean": round(float(np.mean([q.n_tracked for q in vo.results[1:]])), 1),
             "tracked": [q.n_tracked for q in vo.results], "final_centre_drift_m": round(drift, 4)}
        runs.append(r)
        print(json.dumps(r), flush=True)
    return runs


def cmd_klt_guided(a):
    """The guided tracker (csrc/klt.hip, me_klt_track_guided) beside the plain
    one on cmd_klt's inputs, the guess being the unguided result moved by the
    +-2 px pattern of tests/klt_guided_cases.py: ME_KT_KLT and ME_KT_PYR
    events per call, --repeats blocks of --reps calls each, the two entry
    points alternating.  Then (--loop N) the native VO loop at config 3 over N
    corridor keyframes with klt_predict off and on, alternating, two repeats
    each.  --fast N alone (no device touched) runs the CPU comparison of
    _fast_sequence_cpu."""
    if a.fast > 0:
        print(json.dumps({"fast_sequence_cpu": _fast_sequence_cpu(a.fast)}))
        return
    import torch

    from uasl_motion_estimation_amd import klt_ref as KR
    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd._lib import ME_DEVICE
    from uasl_motion_estimation_amd.klt import klt_params
    ctx = _setup(a.lib)
    V = ctypes.c_void_p
    W, H, N = 1280, 720, 2000
    scene, K, stream = S.stereo_stream(20261018, W, H, 2)
    pts = S.grid_features(np.random.default_rng(0), N, W, H, 12).astype(np.float32)
    dp, dn, din, dg, dout, dst = (ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(8 * N), ctx.malloc(8 * N),
                                  ctx.malloc(8 * N), ctx.malloc(N))
    L0, L1 = np.ascontiguousarray(stream[0].left), np.ascontiguousarray(stream[1].left)
    ctx.h2d(dp, L0)
    ctx.h2d(dn, L1)
    ctx.h2d(din, pts)
    kp = klt_params()

    def plain():
        ctx.check(ctx.lib.me_klt_track(ctx.h, ME_DEVICE, V(dp), V(dn), W, H, W, V(din), V(dout), V(dst), N,
                                       ctypes.byref(kp)), "me_klt_track")

    def guided():
        ctx.check(ctx.lib.me_klt_track_guided(ctx.h, ME_DEVICE, V(dp), V(dn), W, H, W, V(din), V(dg), V(dout), V(dst),
                                              N, ctypes.byref(kp)), "me_klt_track_guided")
    plain()
    ctx.synchronize()
    unguided, ust = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8)
    ctx.d2h(unguided, dout)
    ctx.d2h(ust, dst)
    k = np.arange(N)
    if a.guess == "pts":  # the plain tracker's own start: the guided instance doing the plain one's work
        guess = pts.copy()
    else:
        e = np.stack([((7 * k) % 9 - 4) / 2.0, ((5 * k) % 9 - 4) / 2.0], -1)
        guess = (unguided.astype(np.float64) + (e if a.guess == "result2px" else 0.0)).astype(np.float32)
    ctx.h2d(dg, guess)
    out = {"inputs": f"{W}x{H}, {N} features, guess = {a.guess}", "reps": a.reps, "calls": []}
    for fn in (plain, guided):
        for _ in range(5):
            fn()
    ctx.synchronize()
    for rep_ in range(a.repeats):
        for name, fn in (("me_klt_track", plain), ("me_klt_track_guided", guided)):
            ctx.timing_reset()
            ctx.timing(True, ["KLT", "PYR"])
            w0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            ctx.synchronize()
            wall = (time.perf_counter() - w0) / a.reps * 1e6
            ctx.timing(False)
            r = {"call": name, "repeat": rep_, "wall_us_per_call": round(wall, 2)}
            for fam in ("PYR", "KLT"):
                cnt, ms = ctx.timing_read(fam)
                r[f"{fam}_us_per_call"] = round(1000 * ms / max(cnt, 1), 2)
                r[f"{fam}_timed"] = cnt
            out["calls"].append(r)
            print(json.dumps(r), flush=True)
    got, gst = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8)
    ctx.d2h(got, dout)
    ctx.d2h(gst, dst)
    out["tracked_unguided"], out["tracked_guided"] = int(ust.sum()), int(gst.sum())
    both = (ust == 1) & (gst == 1)
    out["max_px_between_guided_and_unguided"] = round(float(np.abs(got[both] - unguided[both]).max()), 4)
    if a.check:
        ref, rst = KR.klt_track_ref(L0, L1, pts, guess)
        same = np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and np.array_equal(gst, rst)
        print(f"klt_guided parity vs the restatement: {'bit-exact' if same else 'MISMATCH'} (tracked: unguided "
              f"{out['tracked_unguided']}, guided {out['tracked_guided']} of {N})", flush=True)
        if not same:
            sys.exit(1)
    for d in (dp, dn, din, dg, dout, dst):
        ctx.free(d)
    if a.loop > 0:
        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep_ in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, klt_predict=on)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep_ >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep_ < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"klt_predict": on, "repeat": rep_, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "new_mean": round(float(np.mean([q.n_new for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def cmd_match_lr(a):
    """The left-right check (csrc/mi.hip, me_mi_epipolar_match_lr) beside the
    plain matcher on a config-3 stereo pair, in the loop's two forms: 2000
    tracked-form features (nd = 13 around the synthetic disparity, unique = 0)
    and 250 new-form features (nd = 127 from d_min, unique = 1).  Per call the
    ME_KT_MI events (plain: scores and pick; check: both passes under one event
    pair) and the host wall time, --repeats blocks of --reps calls each, the
    two entry points alternating (--plain-only: the plain one alone, for an
    A/B of two builds).  Then (--loop N) the native VO loop at config 3 over N
    corridor keyframes with match_lr_max 0 and --lr-max, alternating, two
    repeats each."""
    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    ctx = _setup(a.lib)
    V = ctypes.c_void_p
    W, H, D_MIN, D_MAX = 1280, 720, 2, 128
    scene, K, stream = S.stereo_stream(20261018, W, H, 1)
    L, R = np.ascontiguousarray(stream[0].left), np.ascontiguousarray(stream[0].right)
    dL, dR = ctx.malloc(W * H), ctx.malloc(W * H)
    ctx.h2d(dL, L)
    ctx.h2d(dR, R)
    forms = {}
    for name, n, nd, unique, seed in (("tracked", 2000, 13, 0, 0), ("new", 250, 127, 1, 1)):
        uv = S.grid_features(np.random.default_rng(seed), n, W, H, PL.MARGIN).astype(np.float32)
        if unique:
            lo = np.full(n, D_MIN, np.int32)
        else:  # the loop's window: +-6 px around the predicted (here: the true) disparity
            z, _ = S.depth_at(scene, K, stream[0].R, stream[0].t, uv[:, 0].astype(np.float64),
                              uv[:, 1].astype(np.float64))
            lo = np.clip(np.rint(K[0, 0] * S.BASELINE / z).astype(np.int64) - 6, D_MIN, D_MAX).astype(np.int32)
        d = {"n": n, "nd": nd, "unique": unique, "uv": uv, "lo": lo, "duv": ctx.malloc(8 * n), "dlo": ctx.malloc(4 * n),
             "dxr": ctx.malloc(4 * n), "dok": ctx.malloc(n), "derr": ctx.malloc(4 * n)}
        ctx.h2d(d["duv"], uv)
        ctx.h2d(d["dlo"], lo)
        forms[name] = d

    def plain(d):
        ctx.check(ctx.lib.me_mi_epipolar_match(ctx.h, V(dL), V(dR), W, H, W, V(d["duv"]), V(d["dlo"]), None, None,
                                               d["n"], d["nd"], PL.PATCH, D_MAX, d["unique"], 1.2, float(PL.MARGIN),
                                               V(d["dxr"]), V(d["dok"])), "me_mi_epipolar_match")

    def lr(d):
        ctx.check(ctx.lib.me_mi_epipolar_match_lr(ctx.h, V(dL), V(dR), W, H, W, V(d["duv"]), V(d["dlo"]), None, None,
                                                  d["n"], d["nd"], PL.PATCH, D_MAX, d["unique"], 1.2, float(PL.MARGIN),
                                                  a.lr_max, V(d["dxr"]), V(d["dok"]), V(d["derr"])),
                  "me_mi_epipolar_match_lr")
    calls = [("me_mi_epipolar_match", plain)] + ([] if a.plain_only else [("me_mi_epipolar_match_lr", lr)])
    out = {"inputs": f"{W}x{H}, tracked 2000 x 13 (unique 0), new 250 x 127 (unique 1), lr_max {a.lr_max}",
           "reps": a.reps, "calls": []}
    for _, fn in calls:
        for d in forms.values():
            for _ in range(5):
                fn(d)
    ctx.synchronize()
    for rep in range(a.repeats):
        for name, fn in calls:
            for form, d in forms.items():
                ctx.timing_reset()
                ctx.timing(True, ["MI"])
                w0 = time.perf_counter()
                for _ in range(a.reps):
                    fn(d)
                ctx.synchronize()
                wall = (time.perf_counter() - w0) / a.reps * 1e6
                ctx.timing(False)
                cnt, ms = ctx.timing_read("MI")
                r = {"call": name, "form": form, "repeat": rep, "wall_us_per_call": round(wall, 2),
                     "MI_us_per_call": round(1000 * ms / max(cnt, 1), 2), "MI_timed": cnt}
                out["calls"].append(r)
                print(json.dumps(r), flush=True)
    same = True
    for form, d in forms.items():
        n = d["n"]
        (lr if not a.plain_only else plain)(d)
        ctx.synchronize()
        gxr, gok, gerr = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.full(n, np.inf, np.float32)
        ctx.d2h(gxr, d["dxr"])
        ctx.d2h(gok, d["dok"])
        if not a.plain_only:
            ctx.d2h(gerr, d["derr"])
        counts = {"features": n, "accepted": int(gok.sum())}
        if not a.plain_only:
            counts.update(both_passes_matched=int(np.isfinite(gerr).sum()), within_1px=int((gerr <= 1.0).sum()))
        if a.check:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from pipeline_oracle import OracleBackend  # checker only
            ob = OracleBackend()
            oimgs = ob.frame_images(0, L, R)
            lo64 = d["lo"].astype(np.int64)
            if a.plain_only:
                xr, ok = PL.match_host(ob, oimgs, d["uv"], lo64, d["nd"], None, bool(d["unique"]), D_MAX)
                ok_f, eq = ok, np.array_equal(gok, ok.astype(np.uint8))
            else:
                xr, ok, err, ok_f, ok_b = PL.match_lr_host(ob, oimgs, d["uv"], lo64, d["nd"], None, bool(d["unique"]),
                                                           D_MAX, a.lr_max)
                eq = (np.array_equal(gok, ok.astype(np.uint8))
                      and np.array_equal(gerr.view(np.uint32), err.view(np.uint32)))
                counts.update(forward_accepted=int(ok_f.sum()))
            eq = eq and np.array_equal(gxr.view(np.uint32)[ok_f], xr.view(np.uint32)[ok_f])
            print(f"match_lr parity vs the restatement, {form}: {'bit-exact' if eq else 'MISMATCH'} {counts}",
                  flush=True)
            same = same and eq
        out[form] = counts
    for d in forms.values():
        for k in ("duv", "dlo", "dxr", "dok", "derr"):
            ctx.free(d[k])
    ctx.free(dL)
    ctx.free(dR)
    if not same:
        sys.exit(1)
    if a.loop > 0 and not a.plain_only:
        import torch

        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(Rm)]) for (Rm, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for lr_max in (0.0, a.lr_max):
                cfg = PL.PipelineConfig.from_config(c, match_lr_max=lr_max)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"match_lr_max": lr_max, "repeat": rep, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "new_mean": round(float(np.mean([q.n_new for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def _realistic_camera(w, h):
    """A plausible raw camera for a w x h rectified image: k1 -0.3, k2 0.1, small tangential terms,
    rotations of a degree or two about every axis, slightly different focal lengths and centre."""
    import math

    from uasl_motion_estimation_amd.rectify import CameraModel, RectifiedModel

    def rot(axis, deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        R = np.eye(3)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        return R

    rect = RectifiedModel(w, h, 0.9 * w, 0.9 * w, w / 2.0, h / 2.0)
    R = rot(0, 1.0) @ rot(1, -1.5) @ rot(2, 0.7)
    cam = CameraModel(w, h, 0.92 * w, 0.91 * w, w / 2.0 + 3.5, h / 2.0 - 2.25, (-0.3, 0.1, 5e-4, -3e-4, 0.0),
                      tuple(R.ravel()))
    return cam, rect


def cmd_rectify(a):
    """The rectifier (csrc/rectify.hip): me_rectify_map once and me_remap_q5
    --reps times per size (1280x720, 3840x2160) through the map of a realistic
    camera, HIP-event times of the ME_KT_RECTIFY family; the share of tiles on
    each path; the rate in algorithmic bytes (8 map + 1 source + 1 destination
    per pixel) beside me_hbm_copy_gbs moving the same number of bytes.  With
    --check both results are compared with the numpy restatement at full size.
    Then the config-3 native loop over --loop corridor keyframes, rectifier off
    (plain frames) and on (the frames padded by (8, 5) and the camera that
    crops them back: the same pixels reach the loop), alternating, two timed
    runs each.  With --lib a -DME_REMAP_NO_STAGE build times the global path
    alone on the same maps."""
    ctx = _setup(a.lib)
    from uasl_motion_estimation_amd import pipeline as PL, rectify as RC, synthetic as S

    V = ctypes.c_void_p
    out = {"lib": a.lib or "in-tree", "reps": a.reps}
    ok = True
    for (W, H) in ((1280, 720), (3840, 2160)):
        cam, rect = _realistic_camera(W, H)
        npx = W * H
        src = np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8)
        tx, ty = RC.tile_grid(W, H)
        d_src, d_map, d_dst, d_tp = ctx.malloc(npx), ctx.malloc(8 * npx), ctx.malloc(npx), ctx.malloc(tx * ty)
        ctx.h2d(d_src, src)
        cc, rc = cam.to_c(), rect.to_c()

        def build_map():
            ctx.check(ctx.lib.me_rectify_map(ctx.h, 1, ctypes.byref(cc), ctypes.byref(rc), V(d_map)), "me_rectify_map")

        def warp(tp):
            ctx.check(ctx.lib.me_remap_q5(ctx.h, 1, V(d_src), W, H, W, V(d_map), W, H, 0, V(d_dst), W,
                                          V(d_tp) if tp else None), "me_remap_q5")

        build_map()
        warp(True)
        ctx.synchronize()
        ctx.timing(True, ["RECTIFY"])
        ctx.timing_reset()
        for _ in range(5):
            build_map()
        ctx.synchronize()
        n_map, ms_map = ctx.timing_read("RECTIFY")
        for _ in range(20):
            warp(False)
        ctx.synchronize()
        ctx.timing_reset()
        for _ in range(a.reps):
            warp(False)
        ctx.synchronize()
        n, ms = ctx.timing_read("RECTIFY")
        ctx.timing(False)
        gbs = ctypes.c_double()
        ctx.check(ctx.lib.me_hbm_copy_gbs(ctx.h, 5 * npx, 50, ctypes.byref(gbs)), "me_hbm_copy_gbs")
        tp = np.zeros(tx * ty, np.uint8)
        ctx.d2h(tp, d_tp)
        us = 1e3 * ms / n
        rate = 10.0 * npx / (us * 1e-6) / 1e9
        r = {"size": f"{W}x{H}", "rectify_map_us": round(1e3 * ms_map / n_map, 2), "remap_us": round(us, 2),
             "launches": n, "tiles": int(tp.size), "tiles_global_path": int(tp.sum()),
             "algorithmic_bytes_per_pixel": 10, "remap_algorithmic_gbs": round(rate, 1),
             "copy_same_bytes_gbs": round(gbs.value, 1), "fraction_of_copy": round(rate / gbs.value, 3)}
        if a.check:
            m = np.zeros((H, W, 2), np.int32)
            got = np.zeros((H, W), np.uint8)
            ctx.d2h(m, d_map)
            ctx.d2h(got, d_dst)
            mref = RC.rectify_map_ref(cam, rect)
            r["map_bit_exact"] = bool(np.array_equal(m, mref))
            r["remap_bit_exact"] = bool(np.array_equal(got, RC.remap_ref(src, mref, 0)))
            ok = ok and r["map_bit_exact"] and r["remap_bit_exact"]
        for p in (d_src, d_map, d_dst, d_tp):
            ctx.free(p)
        out[r["size"]] = r
        print(json.dumps(r), flush=True)
    if not ok:
        sys.exit(1)
    if a.loop > 0:
        import torch

        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(Rm)]) for (Rm, t) in arc]
        K = S.intrinsics(1280, 720)
        px, py = 8, 5
        rect = RC.RectifiedModel.from_K(1280, 720, K)
        cam = RC.CameraModel(1280 + 2 * px, 720 + 2 * py, rect.fx, rect.fy, rect.cx + px, rect.cy + py)
        rig = RC.StereoRectifier(cam, cam, rect, border=0)
        frames, padded = [], []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            for (Lk, Rk, _, _) in fr:
                frames.append((Lk.contiguous(), Rk.contiguous()))
                padded.append(tuple(torch.nn.functional.pad(im, (px, px, py, py), value=77).contiguous()
                                    for im in (Lk, Rk)))
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs, poses = [], {}
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, rectify=rig if on else None)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                seq = padded if on else frames
                t0 = time.perf_counter()
                for t in range(NK if rep >= 0 else min(NK, 30)):
                    vo.process(t, *seq[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                poses[on] = np.stack([q.pose for q in res])
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"rectify": on, "repeat": rep, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
        out["loop_poses_bit_equal"] = bool(np.array_equal(poses[False].view(np.uint64), poses[True].view(np.uint64)))
    print(json.dumps(out))


def _low_contrast(w, h, seed=5):
    """A 16-level image: uniform noise smoothed twice with the 5-point cross average, 100 + v // 16."""
    a = np.random.default_rng(seed).random((h, w))
    for _ in range(2):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    v = np.rint(255.0 * (a - a.min()) / (a.max() - a.min())).astype(np.int64)
    return (100 + v // 16).astype(np.uint8)


def cmd_clahe(a):
    """The equaliser (csrc/clahe.hip): me_clahe --reps times after 20 warm-up
    calls per size (1280x720, 3840x2160) and image (noise; the 16-level
    low-contrast image, on which the lanes of a wave meet on a few histogram
    words), 8 x 8 tiles, clip 3.0, HIP-event times of the ME_KT_CLAHE family.
    A call launches the table kernel, then the apply kernel: one timed run
    takes every launch (table + apply), a second one every other launch
    (me_timing_sample(2): the table kernels), the apply kernel is the
    difference.  The yardstick is me_hbm_copy_gbs moving the same algorithmic
    bytes: one read pass for the table, one read and one write per pixel for
    the apply.  With --check image and tables are compared with the numpy
    restatement at full size.  Then the config-3 native loop over --loop
    corridor keyframes, equaliser off and on, alternating, two timed runs each."""
    ctx = _setup(a.lib)
    from uasl_motion_estimation_amd import equalise as EQ, pipeline as PL, synthetic as S

    V = ctypes.c_void_p
    out = {"lib": a.lib or "in-tree", "reps": a.reps}
    ok = True
    params = EQ.Clahe()
    pc = params.to_c()
    for (W, H) in ((1280, 720), (3840, 2160)):
        npx = W * H
        nlut = params.tiles_x * params.tiles_y * 256
        gb_t, gb_a = ctypes.c_double(), ctypes.c_double()
        # (the copy reads and writes its buffer once: npx / 2 bytes move npx, npx bytes move 2 npx)
        ctx.check(ctx.lib.me_hbm_copy_gbs(ctx.h, npx // 2, 50, ctypes.byref(gb_t)), "me_hbm_copy_gbs")
        ctx.check(ctx.lib.me_hbm_copy_gbs(ctx.h, npx, 50, ctypes.byref(gb_a)), "me_hbm_copy_gbs")
        for name in ("noise", "low"):
            src = (np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8) if name == "noise"
                   else _low_contrast(W, H))
            d_src, d_dst, d_lut = ctx.malloc(npx), ctx.malloc(npx), ctx.malloc(nlut)
            ctx.h2d(d_src, src)

            def call():
                ctx.check(ctx.lib.me_clahe(ctx.h, 1, V(d_src), W, H, W, ctypes.byref(pc), V(d_dst), W, V(d_lut)),
                          "me_clahe")

            for _ in range(20):
                call()
            ctx.synchronize()
            ctx.timing(True, ["CLAHE"])
            res = []
            for every in (1, 2):
                ctx.timing_sample(every)
                ctx.timing_reset()
                for _ in range(a.reps):
                    call()
                ctx.synchronize()
                res.append(ctx.timing_read("CLAHE"))
            ctx.timing_sample(1)
            ctx.timing(False)
            (n_all, ms_all), (n_tab, ms_tab) = res
            assert n_all == 2 * a.reps and n_tab == a.reps, (n_all, n_tab)
            both_us, table_us = 1e3 * ms_all / a.reps, 1e3 * ms_tab / n_tab
            apply_us = both_us - table_us
            copy_t, copy_a = npx / gb_t.value * 1e-3, 2.0 * npx / gb_a.value * 1e-3  # us
            r = {"size": f"{W}x{H}", "image": name, "calls": a.reps, "table_us": round(table_us, 2),
                 "apply_us": round(apply_us, 2), "both_us": round(both_us, 2),
                 "copy_same_bytes_table_us": round(copy_t, 2), "copy_same_bytes_apply_us": round(copy_a, 2),
                 "table_fraction_of_copy": round(copy_t / table_us, 3),
                 "apply_fraction_of_copy": round(copy_a / apply_us, 3)}
            if a.check:
                got, lut = np.zeros((H, W), np.uint8), np.zeros((params.tiles_y, params.tiles_x, 256), np.uint8)
                ctx.d2h(got, d_dst)
                ctx.d2h(lut, d_lut)
                want, want_lut = EQ.clahe_ref(src, params)
                r["lut_bit_exact"] = bool(np.array_equal(lut, want_lut))
                r["image_bit_exact"] = bool(np.array_equal(got, want))
                ok = ok and r["lut_bit_exact"] and r["image_bit_exact"]
            for p in (d_src, d_dst, d_lut):
                ctx.free(p)
            out[f"{r['size']}_{name}"] = r
            print(json.dumps(r), flush=True)
    if not ok:
        sys.exit(1)
    if a.loop > 0:
        import torch

        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(Rm)]) for (Rm, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            for (Lk, Rk, _, _) in fr:
                frames.append((Lk.contiguous(), Rk.contiguous()))
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, equalise=params if on else None)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"equalise": on, "repeat": rep, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def cmd_tonemap(a):
    """The 16-bit ingest (csrc/tonemap.hip): me_tonemap16 on one state --reps
    times after 20 warm-up calls per size (640x480, 1280x720, 3840x2160) and
    image (14-bit noise; the low-entropy image 100*64 + v // 16, on which the
    lanes of a wave meet on a few histogram words), default parameters,
    HIP-event times of the ME_KT_TONEMAP family.  A call launches the coarse
    select, the fine select and the apply kernel: one timed run takes every
    launch, a second one every third (me_timing_sample(3): the coarse
    selects); fine select + apply is the difference (the family's sampling
    cannot part those two).  The yardstick is me_hbm_copy_gbs moving the same
    algorithmic bytes: 2 B read per pixel for each select pass, 2 B read + 1 B
    written for the apply.  With --check image and state are compared with the
    numpy restatement at full size.  Then the config-3 native loop over --loop
    corridor keyframes, the 8-bit stream through me_vo_loop_process against
    its 16-bit twin 7000 + 2 v through me_vo_loop_process16, alternating, two
    timed runs each."""
    ctx = _setup(a.lib)
    from uasl_motion_estimation_amd import pipeline as PL, synthetic as S, tonemap as TM

    V = ctypes.c_void_p
    out = {"lib": a.lib or "in-tree", "reps": a.reps}
    ok = True
    params = TM.ToneMap()
    pc = params.to_c()
    for (W, H) in ((640, 480), (1280, 720), (3840, 2160)):
        npx = W * H
        gb_1, gb_2 = ctypes.c_double(), ctypes.c_double()
        # (the copy reads and writes its buffer once: npx bytes move 2 npx, 2.5 npx bytes move 5 npx)
        ctx.check(ctx.lib.me_hbm_copy_gbs(ctx.h, npx, 50, ctypes.byref(gb_1)), "me_hbm_copy_gbs")
        ctx.check(ctx.lib.me_hbm_copy_gbs(ctx.h, 5 * npx // 2, 50, ctypes.byref(gb_2)), "me_hbm_copy_gbs")
        for name in ("noise", "low"):
            src = (np.random.default_rng(5).integers(0, 1 << 14, (H, W), dtype=np.uint16) if name == "noise"
                   else (100 * 64 + (_low_contrast(W, H).astype(np.uint16) - 100)).astype(np.uint16))
            d_src, d_dst = ctx.malloc(2 * npx), ctx.malloc(npx)
            ctx.h2d(d_src, src)
            st = TM.ToneMapState(ctx)

            def call():
                ctx.check(ctx.lib.me_tonemap16(ctx.h, 1, V(d_src), W, H, W, V(d_dst), W, ctypes.byref(pc), st.h),
                          "me_tonemap16")

            for _ in range(20):
                call()
            ctx.synchronize()
            ctx.timing(True, ["TONEMAP"])
            res = []
            for every in (1, 3):
                ctx.timing_sample(every)
                ctx.timing_reset()
                for _ in range(a.reps):
                    call()
                ctx.synchronize()
                res.append(ctx.timing_read("TONEMAP"))
            ctx.timing_sample(1)
            ctx.timing(False)
            (n_all, ms_all), (n_co, ms_co) = res
            assert n_all == 3 * a.reps and n_co == a.reps, (n_all, n_co)
            all_us, coarse_us = 1e3 * ms_all / a.reps, 1e3 * ms_co / n_co
            rest_us = all_us - coarse_us
            copy_1, copy_2 = 2.0 * npx / gb_1.value * 1e-3, 5.0 * npx / gb_2.value * 1e-3  # us
            r = {"size": f"{W}x{H}", "image": name, "calls": a.reps, "coarse_us": round(coarse_us, 2),
                 "fine_plus_apply_us": round(rest_us, 2), "all_us": round(all_us, 2),
                 "copy_same_bytes_coarse_us": round(copy_1, 2), "copy_same_bytes_fine_plus_apply_us": round(copy_2, 2),
                 "coarse_fraction_of_copy": round(copy_1 / coarse_us, 3),
                 "fine_plus_apply_fraction_of_copy": round(copy_2 / rest_us, 3)}
            if a.check:
                st.reset()
                call()
                got = np.zeros((H, W), np.uint8)
                ctx.d2h(got, d_dst)
                want, want_st = TM.tonemap_ref(src, params)
                r["state_bit_exact"] = bool(st.read() == want_st)
                r["image_bit_exact"] = bool(np.array_equal(got, want))
                ok = ok and r["state_bit_exact"] and r["image_bit_exact"]
            st.close()
            for p in (d_src, d_dst):
                ctx.free(p)
            out[f"{r['size']}_{name}"] = r
            print(json.dumps(r), flush=True)
    if not ok:
        sys.exit(1)
    if a.loop > 0:
        import torch

        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(Rm)]) for (Rm, t) in arc]
        K = S.intrinsics(1280, 720)
        frames, wide = [], []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            for (Lk, Rk, _, _) in fr:
                frames.append((Lk.contiguous(), Rk.contiguous()))
                wide.append(tuple((7000 + 2 * im.to(torch.int32)).to(torch.uint16).contiguous() for im in frames[-1]))
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep in range(-1, 2):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, tonemap=params if on else None)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                src = wide if on else frames
                t0 = time.perf_counter()
                for t in range(NK if rep >= 0 else min(NK, 30)):
                    vo.process(t, *src[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"tonemap": on, "repeat": rep, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def cmd_motion_gate(a):
    """me_motion_gate alone (ME_KT_GATE events: three launches per call) and inside the config-3 native loop."""
    import torch

    from uasl_motion_estimation_amd import motion_gate as MG
    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S

    ctx = _setup(a.lib)
    W, H, N = 1280, 720, 2000
    f, cx, cy, b = 0.9 * W, W / 2.0, H / 2.0, S.BASELINE
    rng = np.random.default_rng(11)
    Z = rng.uniform(3.0, 40.0, N)
    u, v = rng.uniform(30, W - 30, N), rng.uniform(30, H - 30, N)
    P = np.stack([(u - cx) * Z / f, (v - cy) * Z / f, Z], 1)
    Q = P @ S.aa_to_R(np.array([0.004, -0.02, 0.002])).T + np.array([0.03, -0.01, -0.5])
    mov = rng.random(N) < 0.2
    Q[mov] = P[mov] @ S.aa_to_R(np.array([0.0, 0.03, 0.0])).T + np.array([0.6, 0.0, 0.3])

    def proj(X):
        return np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy, f * (X[:, 0] - b) / X[:, 2] + cx], 1)

    prev = (proj(P) + rng.normal(0, 0.25, (N, 3))).astype(np.float32)
    cur = (proj(Q) + rng.normal(0, 0.25, (N, 3))).astype(np.float32)
    ones = np.ones(N, np.uint8)
    p = MG.MotionGate()
    cam = (f, cx, cy, b, W, H, PL.MARGIN)
    out = {"inputs": f"{W}x{H}, {N} tracks, {int(mov.sum())} on a second body, 0.25 px noise, defaults", "reps": a.reps,
           "calls": []}
    parts = [np.ascontiguousarray(prev[:, :2]), np.ascontiguousarray(prev[:, 2]), np.ascontiguousarray(cur[:, :2]),
             np.ascontiguousarray(cur[:, 2]), ones, ones, ones]
    offs = [int(x) for x in np.cumsum([0] + [q.nbytes for q in parts])]
    host = np.concatenate([q.view(np.uint8).ravel() for q in parts])
    d = ctx.malloc(host.nbytes)
    ctx.h2d(d, host)

    def call():
        MG.motion_gate_device(ctx, p, d + offs[0], d + offs[1], d + offs[2], d + offs[3], d + offs[4], d + offs[5], N,
                              *cam, 7, d + offs[6])

    for rep_ in range(a.repeats):
        for _ in range(5):
            call()
        ctx.synchronize()
        ctx.timing(True, ["GATE"])
        ctx.timing_reset()
        w0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        ctx.synchronize()
        wall = (time.perf_counter() - w0) / a.reps * 1e6
        ctx.timing(False)
        cnt, ms = ctx.timing_read("GATE")
        r = {"call": "me_motion_gate", "repeat": rep_, "wall_us_per_call": round(wall, 2),
             "GATE_us_per_call": round(1000 * ms / max(cnt // 3, 1), 2), "GATE_launches_timed": cnt}
        out["calls"].append(r)
        print(json.dumps(r), flush=True)
    ctx.free(d)
    if a.check:
        ok, err, info = MG.motion_gate_ref(prev, cur[:, :2], cur[:, 2], ones, ones, *cam, 7, p)
        gok, gerr, ginfo = MG.motion_gate(prev, cur[:, :2], cur[:, 2], ones, ones, *cam, 7, p, ctx=ctx)
        same = (np.array_equal(gok, ok) and np.array_equal(gerr.view(np.uint32), err.view(np.uint32))
                and np.array_equal(ginfo["words"], MG.info_words(info)))
        usable = np.isfinite(err) | (ok != gok)
        out["n_usable"], out["n_inliers"] = info["n_usable"], info["n_inliers"]
        out["movers_kept"] = int((mov & (ok != 0) & np.isfinite(err)).sum())
        out["static_dropped"] = int((~mov & (ok == 0) & usable).sum())
        print(f"motion_gate parity vs the restatement: {'bit-exact' if same else 'MISMATCH'} (usable "
              f"{info['n_usable']}, inliers {info['n_inliers']}, movers kept {out['movers_kept']}, static dropped "
              f"{out['static_dropped']})", flush=True)
        if not same:
            sys.exit(1)
    if a.loop > 0:
        c, NK = 3, a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + c, 1280, 720, c0, min(50, NK - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
            print(f"rendered {len(frames)} keyframes", flush=True)
        runs = []
        for rep_ in range(-1, a.repeats):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, motion_gate=p if on else None)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep_ >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                if rep_ < 0:
                    vo.close()
                    continue
                st = vo._stats()
                res = vo.results
                vo.close()
                names = ["klt_match", "first_match", "scale_submit", "window_submit", "ba_result", "scale_result"]
                r = {"motion_gate": on, "repeat": rep_, "keyframes": NK, "keyframes_per_s": round(NK / dt, 2),
                     "tracked_mean": round(float(np.mean([q.n_tracked for q in res[2:]])), 1),
                     "new_mean": round(float(np.mean([q.n_new for q in res[2:]])), 1),
                     "host_s": round(st[0], 4), "blocked_s": round(st[1], 4),
                     "wait_ms_per_keyframe": {k: round(1e3 * st[3 + i] / NK, 4) for i, k in enumerate(names)}}
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["loop_config3"] = runs
    print(json.dumps(out))


def cmd_frame_pose(a):
    """me_frame_pose alone (ME_KT_FRAMEPOSE events: seven launches per call) and inside the config-3 native push loop."""
    import torch

    from uasl_motion_estimation_amd import frame_pose as FP
    from uasl_motion_estimation_amd import keyframe as KF
    from uasl_motion_estimation_amd import motion_gate as MG
    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S

    ctx = _setup(a.lib)
    W, H, N = 1280, 720, 2000
    f, cx, cy, b = 0.9 * W, W / 2.0, H / 2.0, S.BASELINE
    rng = np.random.default_rng(11)
    Z = rng.uniform(3.0, 40.0, N)
    u, v = rng.uniform(30, W - 30, N), rng.uniform(30, H - 30, N)
    P = np.stack([(u - cx) * Z / f, (v - cy) * Z / f, Z], 1)
    Q = P @ S.aa_to_R(np.array([0.004, -0.02, 0.002])).T + np.array([0.03, -0.01, -0.5])

    def proj(X):
        return np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy, f * (X[:, 0] - b) / X[:, 2] + cx], 1)

    ref = (proj(P) + rng.normal(0, 0.3, (N, 3))).astype(np.float32)
    cur = (proj(Q) + rng.normal(0, 0.3, (N, 3))).astype(np.float32)
    gross = rng.random(N) < 0.2
    cur[gross, :2] += rng.uniform(-40, 40, (int(gross.sum()), 2)).astype(np.float32)
    ones = np.ones(N, np.uint8)
    p = FP.FramePose()
    out = {"inputs": f"{W}x{H}, {N} features, {int(gross.sum())} gross outliers, 0.3 px noise, defaults, start NULL",
           "reps": a.reps, "calls": []}
    # ref_uv | ref_xr | cur_uv | cur_xr | new_uv | alive | status | ok | ok_out | info (128) + kf info (32) |
    # me_kf_update's own cur_uv and alive (it updates them in place: the pose's inputs stay what they are)
    parts = [np.ascontiguousarray(ref[:, :2]), np.ascontiguousarray(ref[:, 2]), np.ascontiguousarray(cur[:, :2]),
             np.ascontiguousarray(cur[:, 2]), np.ascontiguousarray(cur[:, :2]), ones, ones, ones, ones,
             np.zeros(128 + 32, np.uint8), np.ascontiguousarray(cur[:, :2]), ones]
    offs = [int(16 * ((x + 15) // 16)) for x in np.cumsum([0] + [q.nbytes + 16 for q in parts])]
    host = np.zeros(offs[-1], np.uint8)
    for q, o in zip(parts, offs):
        host[o:o + q.nbytes] = q.view(np.uint8).ravel()
    d = ctx.malloc(host.nbytes)
    ctx.h2d(d, host)
    o = [d + x for x in offs]
    gp, kp = MG.MotionGate(), KF.KeyframeSelect()

    def pose_call():
        FP.frame_pose_device(ctx, p, o[0], o[1], o[2], o[5], N, f, cx, cy, b, o[9])

    def kf_call():
        KF.kf_update_device(ctx, kp, o[0], o[10], o[11], o[4], o[6], N, W, H, PL.MARGIN, 1, o[9] + 128)

    def gate_call():
        MG.motion_gate_device(ctx, gp, o[0], o[1], o[2], o[3], o[6], o[7], N, f, cx, cy, b, W, H, PL.MARGIN, 7, o[8])

    if a.trace:
        for _ in range(a.reps):
            pose_call()
            kf_call()
            gate_call()
        ctx.synchronize()
        ctx.free(d)
        print(json.dumps({"traced_calls": a.reps}))
        return
    for rep_ in range(a.repeats):
        rows = [("me_frame_pose", "FRAMEPOSE", 1 + p.iters, pose_call), ("me_kf_update", "KEYFRAME", 1, kf_call),
                ("me_motion_gate", "GATE", 3, gate_call)]
        for name, fam, per, call in rows:
            for _ in range(5):
                call()
            ctx.synchronize()
            w0 = time.perf_counter()
            for _ in range(a.reps):
                call()
            ctx.synchronize()
            wall = (time.perf_counter() - w0) / a.reps * 1e6  # (no event timing in this window)
            ctx.timing(True, [fam])
            ctx.timing_reset()
            for _ in range(a.reps):
                call()
            ctx.synchronize()
            ctx.timing(False)
            cnt, ms = ctx.timing_read(fam)
            r = {"call": name, "repeat": rep_,
                 "wall_us_per_call": round(wall, 2), f"{fam}_us_per_call": round(1000 * ms / max(cnt // per, 1), 2),
                 f"{fam}_launches_timed": cnt}
            out["calls"].append(r)
            print(json.dumps(r), flush=True)
    ctx.free(d)
    if a.check:
        err, info = FP.frame_pose_ref(ref, cur[:, :2], ones, f, cx, cy, b, p)
        gerr, ginfo = FP.frame_pose(ref, cur[:, :2], ones, f, cx, cy, b, p, ctx=ctx)
        same = (np.array_equal(gerr.view(np.uint32), err.view(np.uint32))
                and np.array_equal(ginfo["words"], FP.info_words(info)))
        out.update(n_usable=info["n_usable"], n_inliers=info["n_inliers"], steps=info["steps"], valid=info["valid"])
        print(f"frame_pose parity vs the restatement: {'bit-exact' if same else 'MISMATCH'} (usable "
              f"{info['n_usable']}, inliers {info['n_inliers']}, steps {info['steps']}, valid {info['valid']}, "
              f"t {[round(float(x), 4) for x in info['t']]})", flush=True)
        if not same:
            sys.exit(1)
    if a.loop > 0:
        c, NF, SUB = 3, a.loop, 3
        poses = S.trajectory_arc(NF, sub=SUB)
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in poses]
        K = S.intrinsics(1280, 720)
        scene = S.CorridorScene(S.SEED0 + c, S.arc_radius())
        lut = torch.as_tensor(S.tone_map(), device="cuda")
        frames = []
        for (R, t) in poses:
            L = S.render_corridor_torch(scene, K, R, t, 1280, 720, 0.0, "cuda")
            Rr = lut[S.render_corridor_torch(scene, K, R, t, 1280, 720, S.BASELINE, "cuda").long()]
            frames.append((L.contiguous(), Rr.contiguous()))
        torch.cuda.synchronize()
        print(f"rendered {len(frames)} camera frames, {SUB} per keyframe step of the arc", flush=True)
        vel = SUB * (truth[1] - truth[0])  # per keyframe step; the loop's prediction is not scaled by the gap
        runs = []
        for rep_ in range(-1, a.repeats):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for on in (False, True):
                cfg = PL.PipelineConfig.from_config(c, keyframe_select=kp, frame_pose=p if on else None)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], vel, log_events=False, overlap=True)
                t0 = time.perf_counter()
                nf = NF if rep_ >= 0 else min(NF, 30)
                kts = [vo.push(*frames[i]) for i in range(nf)]
                vo.finish()
                dt = time.perf_counter() - t0
                log = vo.frame_pose_log if on else []
                vo.close()
                if rep_ < 0:
                    continue
                nk = sum(1 for t in kts if t >= 0)
                r = {"frame_pose": on, "repeat": rep_, "frames": nf, "keyframes": nk, "frames_per_s": round(nf / dt, 2),
                     "keyframes_per_s": round(nk / dt, 2)}
                if on:
                    r.update(poses=len(log), valid=sum(q["pose_valid"] for q in log),
                             inliers_mean=round(float(np.mean([q["n_inliers"] for q in log])), 1))
                runs.append(r)
                print(json.dumps(r), flush=True)
        out["push_loop_config3"] = runs
    print(json.dumps(out))


def cmd_window_cov(a):
    """me_ba_covariance (cameras, the one-workgroup global-memory factor) beside me_ba_covariance_full (cameras only /
    with landmarks; host form and the queued device-resident form) on a config's window after 10 LM iterations: wall
    time per call, the plan and linearisation included (the same for every entry).  The kernels' own times come from
    a rocprofv3 --kernel-trace --stats run of --trace 1 (few calls, nothing timed)."""
    from uasl_motion_estimation_amd.optimisation import (DeviceBAProblem, SolverOptions, ba_covariance,
                                                         ba_covariance_full, ba_solve)
    ctx = _setup(a.lib)
    for c in a.configs.split(","):
        bp = _ba_problem(c)
        bp.cams, bp.pts, _ = ba_solve(bp, SolverOptions.fixed_iterations(10), ctx=ctx)
        dev = DeviceBAProblem(bp, ctx)
        calls = {
            "me_ba_covariance": lambda: ba_covariance(bp, ctx=ctx),
            "me_ba_covariance_full[cameras]": lambda: ba_covariance_full(bp, ctx=ctx, landmarks=False),
            "me_ba_covariance_full[cameras+landmarks]": lambda: ba_covariance_full(bp, ctx=ctx),
            "me_ba_covariance_full[device, cameras]": lambda: dev.covariance_full_async(landmarks=False),
            "me_ba_covariance_full[device, cameras+landmarks]": lambda: dev.covariance_full_async(),
        }
        nf = min(max(bp.fixed_frames, 0), len(bp.cams))
        shape = {"config": c, "cams": len(bp.cams), "pts": len(bp.pts), "obs": len(bp.obs), "n6": 6 * (len(bp.cams) - nf)}
        for name, f in calls.items():
            r = f()
            ctx.synchronize()
            ok = dev.covariance_read()[0] if "device" in name else int(r is not None)
            if a.trace:
                for _ in range(a.reps):
                    f()
                ctx.synchronize()
                continue
            for rep in range(a.repeats):
                ctx.synchronize()
                w0 = time.perf_counter()
                for _ in range(a.reps):
                    f()
                ctx.synchronize()
                print(json.dumps(dict(shape, call=name, repeat=rep, ok=ok,
                                      wall_us_per_call=round((time.perf_counter() - w0) / a.reps * 1e6, 2))), flush=True)
        dev.close()
    if a.loop > 0 and not a.trace:  # the config-3 native loop with the switch off / cameras / cameras and landmarks
        import torch

        from uasl_motion_estimation_amd import pipeline as PL
        from uasl_motion_estimation_amd import synthetic as S
        from uasl_motion_estimation_amd.ba_cov import WindowCovariance
        NK = a.loop
        arc = S.trajectory_arc(max(NK, 2))
        truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
        K = S.intrinsics(1280, 720)
        frames = []
        for c0 in range(0, NK, 50):
            _, fr = S.corridor_frames_torch(S.SEED0 + 3, 1280, 720, c0, min(50, NK - c0))
            frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
            torch.cuda.synchronize()
        for rep_ in range(-1, a.repeats):  # (-1: a short untimed run, the first loop of a process pays the allocations)
            for name, cov in (("off", None), ("cameras", WindowCovariance(landmarks=False)),
                              ("cameras+landmarks", WindowCovariance())):
                cfg = PL.PipelineConfig.from_config(3, covariance=cov)
                vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
                t0 = time.perf_counter()
                for t in range(NK if rep_ >= 0 else min(NK, 30)):
                    vo.process(t, *frames[t])
                vo.finish()
                dt = time.perf_counter() - t0
                okc = vo.pose_cov_ok()
                vo.close()
                if rep_ >= 0:
                    print(json.dumps({"covariance": name, "repeat": rep_, "keyframes": NK,
                                      "keyframes_per_s": round(NK / dt, 2), "us_per_keyframe": round(1e6 * dt / NK, 1),
                                      "windows_ok": int(sum(okc.values())), "windows": len(okc)}), flush=True)


def cmd_track_check(a):
    """The config-3 native loop with and without the residual check behind every window solve
    (PipelineConfig(track_check=TrackCheck())), same build, the two interleaved: keyframes/s, the ME_KT_BA_CHECK
    time per launch (event timing of that family alone, on the BA context) and the number of tracks flagged."""
    import torch

    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd import synthetic as S
    from uasl_motion_estimation_amd.track_check import TrackCheck
    ctx = _setup(a.lib)
    NK = a.loop
    arc = S.trajectory_arc(max(NK, 2))
    truth = [np.concatenate([t, S.R_to_aa_robust(R)]) for (R, t) in arc]
    K = S.intrinsics(1280, 720)
    frames = []
    for c0 in range(0, NK, 50):
        _, fr = S.corridor_frames_torch(S.SEED0 + 3, 1280, 720, c0, min(50, NK - c0))
        frames += [(Lk.contiguous(), Rk.contiguous()) for (Lk, Rk, _, _) in fr]
        torch.cuda.synchronize()
    for rep_ in range(-1, a.repeats):  # (-1: a short untimed run, the first loop of a process pays the allocations)
        for name, chk in (("off", None), ("on", TrackCheck())):
            timed = a.kernel_time and rep_ >= 0
            if timed:
                ctx.timing(True, ["BA_CHECK"])
                ctx.timing_sample(1)
                ctx.timing_reset()
            cfg = PL.PipelineConfig.from_config(3, track_check=chk)
            vo = PL.NativeStereoVO(cfg, ctx, K, truth[0], truth[1] - truth[0], log_events=False, overlap=True)
            t0 = time.perf_counter()
            for t in range(NK if rep_ >= 0 else min(NK, 30)):
                vo.process(t, *frames[t])
            vo.finish()
            dt = time.perf_counter() - t0
            fl = vo.flagged()
            n_active = [r.n_active for r in vo.results]
            vo.close()
            launches, ms = (0, 0.0)
            if timed:
                ctx.synchronize()
                launches, ms = ctx.timing_read("BA_CHECK")
                ctx.timing(False)
            if rep_ >= 0:
                print(json.dumps({"track_check": name, "repeat": rep_, "keyframes": NK,
                                  "keyframes_per_s": round(NK / dt, 2), "us_per_keyframe": round(1e6 * dt / NK, 1),
                                  "check_launches": launches,
                                  "check_us_per_launch": round(1e3 * ms / launches, 2) if launches else None,
                                  "flag_entries": len(fl), "tracks_flagged": len({i for _, i, _ in fl}),
                                  "mean_n_active": round(float(np.mean(n_active)), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=os.environ.get("ME_LIB"))
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("ba_wall")
    p.add_argument("configs", nargs="?", default="3,4,5")
    p = sub.add_parser("klt")
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--check", type=int, default=1)
    p = sub.add_parser("mi")
    p.add_argument("--pairs", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--check", type=int, default=1)
    p = sub.add_parser("coop")
    p.add_argument("--reps", type=int, default=20)
    p = sub.add_parser("solve_ts")
    p.add_argument("configs", nargs="?", default="3,5")
    p = sub.add_parser("scale_ts")
    p.add_argument("--front", type=int, default=0)
    p = sub.add_parser("step_ts")
    p.add_argument("--config", default="3")
    p = sub.add_parser("cam_ts")
    p.add_argument("--config", default="3")
    p = sub.add_parser("schur_stamps")
    p.add_argument("configs", nargs="?", default="3,4")
    p = sub.add_parser("corners")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("klt_fb")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--fb-max", dest="fb_max", type=float, default=0.5)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("klt_guided")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p.add_argument("--guess", choices=("result2px", "result", "pts"), default="result2px",
                   help="the guess: the unguided result moved by up to 2 px, the unguided result, or pts_in")
    p.add_argument("--fast", type=int, default=0,
                   help="> 0: only the CPU comparison on every 6th keyframe of the arc, this many keyframes")
    p = sub.add_parser("match_lr")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--lr-max", dest="lr_max", type=float, default=1.0)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p.add_argument("--plain-only", dest="plain_only", action="store_true",
                   help="me_mi_epipolar_match alone (works on a build without the check: A/B of two trees)")
    p = sub.add_parser("rectify")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("clahe")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("tonemap")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("motion_gate")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("frame_pose")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--check", type=int, default=1)
    p.add_argument("--trace", type=int, default=0, help="1: the calls alone, no event timing (under rocprofv3)")
    p.add_argument("--loop", type=int, default=200, help="camera frames of the config-3 native push loop per run (0: skip)")
    p = sub.add_parser("window_cov")
    p.add_argument("configs", nargs="?", default="3,5")
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--trace", type=int, default=0, help="1: the calls alone, nothing timed (under rocprofv3)")
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run (0: skip)")
    p = sub.add_parser("track_check")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--loop", type=int, default=200, help="keyframes of the config-3 native loop per run")
    p.add_argument("--kernel-time", dest="kernel_time", type=int, default=1,
                   help="1: event timing of ME_KT_BA_CHECK (two event records per window on the BA stream); 0: none")
    a = ap.parse_args()
    globals()["cmd_" + a.cmd](a)


if __name__ == "__main__":
    main()
