"""Window covariance on the device (me_ba_covariance_full): the camera and
landmark blocks against window_cov_ref and the existing me_ba_covariance, the
host and device-resident forms bit for bit, and the ok = 0 cases.  Bar:
window_cov_cases.py.  The shapes take both forms of the factor: the LDS one
(n6 = 6 x variable cameras <= 126) and the global-memory one (26 cameras)."""
import ctypes

import numpy as np
import pytest

import window_cov_cases as C
from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

# name -> (builder(fixed), LM iterations before the covariance)
SHAPES = {
    "stereo_200x8": (lambda f: S.ba_problem(48, 200, 8, 640, 480, fixed=f), 5),
    "mono_200x8": (lambda f: S.ba_problem_mono(49, 200, 8, 640, 480, fixed=f), 5),
    "stereo_60x5": (lambda f: S.ba_problem(42, 60, 5, 640, 480, fixed=f), 0),
    # (seed 56: every camera keeps at least 7 observations, so the window is well conditioned at fixed = 1 too)
    "stereo_100x26_global": (lambda f: S.ba_problem(56, 100, 26, 640, 480, fixed=f), 0),
}
_cache = {}


def window(ctx, oracle, name, fixed):
    """(problem at the parameters the covariance is taken at, window_cov_ref of it), computed once."""
    key = (name, fixed)
    if key not in _cache:
        from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

        build, iters = SHAPES[name]
        bp = build(fixed)
        if iters:
            bp.cams, bp.pts, _ = ba_solve(bp, SolverOptions.fixed_iterations(iters), ctx=ctx)
        ref = C.ref_covariance(oracle, bp)
        assert ref is not None
        _cache[key] = (bp, ref)
    return _cache[key]


@pytest.mark.parametrize("fixed", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_full_covariance_matches_reference(ctx, oracle, name, fixed):
    from uasl_motion_estimation_amd.optimisation import ba_covariance, ba_covariance_full

    bp, (rcam, rpt) = window(ctx, oracle, name, fixed)
    n6 = 6 * (len(bp.cams) - fixed)
    assert (n6 > 126) == name.endswith("global")
    got = ba_covariance_full(bp, ctx=ctx)
    assert got is not None
    cam, pt = got
    assert not cam[:fixed].any()
    C.assert_cam_blocks(cam, rcam)
    C.assert_pt_blocks(pt, rpt)
    old = ba_covariance(bp, ctx=ctx)
    assert old is not None
    C.assert_cam_blocks(cam, old)
    # cameras alone: the same blocks, no landmark stage
    cam_only, none = ba_covariance_full(bp, ctx=ctx, landmarks=False)
    assert none is None and np.array_equal(cam_only, cam)


@pytest.mark.parametrize("name", ["stereo_200x8", "mono_200x8", "stereo_100x26_global"])
def test_host_and_device_forms_identical_and_repeatable(ctx, oracle, name):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, ba_covariance_full

    bp, _ = window(ctx, oracle, name, 2)
    cam, pt = ba_covariance_full(bp, ctx=ctx)
    cam2, pt2 = ba_covariance_full(bp, ctx=ctx)
    assert np.array_equal(cam, cam2) and np.array_equal(pt, pt2)
    dev = DeviceBAProblem(bp, ctx)
    try:
        dev.covariance_full_async()
        ok, dcam, dpt = dev.covariance_read()
        assert ok == 1
        assert np.array_equal(dcam, cam) and np.array_equal(dpt, pt)
        dev.covariance_full_async()
        ok, dcam2, dpt2 = dev.covariance_read()
        assert ok == 1 and np.array_equal(dcam2, cam) and np.array_equal(dpt2, pt)
        # cameras alone: the same camera blocks, the landmark array left as it was
        dev.covariance_outputs(cam_fill=3.25, pt_fill=-1.5)
        dev.covariance_full_async(landmarks=False)
        ok, dcam3, dpt3 = dev.covariance_read()
        assert ok == 1 and np.array_equal(dcam3, cam) and np.all(dpt3 == -1.5)
    finally:
        dev.close()


def _raw_host_call(ctx, bp, cam, pt):
    from uasl_motion_estimation_amd.optimisation import ba_struct

    keep = []
    p, _, _ = ba_struct(bp, keep)
    ok = ctypes.c_int(7)
    rc = ctx.lib.me_ba_covariance_full(ctx.h, ctypes.byref(p), cam.ctypes.data if cam is not None else None,
                                       pt.ctypes.data if pt is not None else None, ctypes.addressof(ok))
    return rc, ok.value


def _failing(kind):
    if kind == "landmark_without_observations":
        bp = S.ba_problem(50, 40, 4, 640, 480)
        bp.pts = np.vstack([bp.pts, [[0.5, 0.2, 10.0]]])
        return bp
    bp = S.ba_problem(44, 30, 4, 640, 480)  # the last (variable) camera loses all its observations
    return C.keep_obs(bp, bp.cam_idx != 3)


@pytest.mark.parametrize("kind", ["landmark_without_observations", "camera_without_observations"])
def test_ok_zero_agrees_and_leaves_outputs_untouched(ctx, oracle, kind):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, ba_covariance, ba_covariance_full

    bp = _failing(kind)
    assert ba_covariance(bp, ctx=ctx) is None and C.ref_covariance(oracle, bp) is None
    assert ba_covariance_full(bp, ctx=ctx) is None
    cam = np.full(36 * len(bp.cams), 3.25)
    pt = np.full(9 * len(bp.pts), -1.5)
    rc, ok = _raw_host_call(ctx, bp, cam, pt)
    assert rc == 0 and ok == 0
    assert np.all(cam == 3.25) and np.all(pt == -1.5)
    dev = DeviceBAProblem(bp, ctx)
    try:
        dev.covariance_outputs(cam_fill=3.25, pt_fill=-1.5)
        dev.covariance_full_async()
        ok, dcam, dpt = dev.covariance_read()
        assert ok == 0 and np.all(dcam == 3.25) and np.all(dpt == -1.5)
        # cameras alone: the landmark array is not the call's to write, whatever the outcome
        dev.covariance_full_async(landmarks=False)
        ok, dcam, dpt = dev.covariance_read()
        assert ok == 0 and np.all(dcam == 3.25) and np.all(dpt == -1.5)
    finally:
        dev.close()


def test_both_outputs_null_is_invalid(ctx):
    rc, _ = _raw_host_call(ctx, S.ba_problem(42, 60, 5, 640, 480), None, None)
    assert rc != 0


def test_fixed_camera_only_landmark_is_inverse_of_V(ctx, oracle):
    from uasl_motion_estimation_amd.ba_cov import huber_row_scale
    from uasl_motion_estimation_amd.optimisation import ba_covariance_full

    bp = C.fixed_only_landmark(S.ba_problem(48, 200, 8, 640, 480))
    o = int(np.nonzero(bp.pt_idx == 0)[0][0])
    r, _, Jp = oracle.ba_evaluate(bp)
    J = huber_row_scale(r)[o] * Jp[o]
    Vinv = np.linalg.inv(J.T @ J)
    cam, pt = ba_covariance_full(bp, ctx=ctx)
    # (the device's own Jacobian agrees with the oracle's to 1e-9, tests/test_gpu_parity.py: the project's bar here)
    np.testing.assert_allclose(pt[0], Vinv, rtol=C.RTOL, atol=C.ATOL * np.abs(Vinv).max())
    rcam, rpt = C.ref_covariance(oracle, bp)
    C.assert_cam_blocks(cam, rcam)
    C.assert_pt_blocks(pt, rpt)


def test_failed_covariance_does_not_leak_into_a_queued_solve(ctx):
    """The covariance has a scratch set of its own and queues without waiting:
    a solve queued behind a failed one runs as if alone."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions

    good = S.ba_problem(48, 200, 8, 640, 480)
    opts = SolverOptions.fixed_iterations(5)
    alone = DeviceBAProblem(good, ctx)
    bad = DeviceBAProblem(_failing("landmark_without_observations"), ctx)
    behind = DeviceBAProblem(good, ctx)
    try:
        s0 = alone.solve(opts)
        c0, p0 = alone.download()
        bad.covariance_full_async()
        behind.solve_async(opts)
        behind.covariance_full_async()  # and one queued behind the unfinished solve, at the cams / pts it leaves
        s1 = behind.wait()
        ok_bad = bad.covariance_read()[0]
        ok, cam, pt = behind.covariance_read()
        c1, p1 = behind.download()
        assert ok_bad == 0 and ok == 1
        assert s1 == s0 and np.array_equal(c1, c0) and np.array_equal(p1, p0)
        # the covariance queued behind the solve saw the solved parameters
        alone.covariance_full_async()
        ok2, cam2, pt2 = alone.covariance_read()
        assert ok2 == 1 and np.array_equal(cam, cam2) and np.array_equal(pt, pt2)
    finally:
        for d in (alone, bad, behind):
            d.close()


def test_covariance_after_reserve(ctx, oracle):
    """me_ba_reserve sizes the covariance's set too; a window inside the reserved sizes is computed as before."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem

    bp, (rcam, rpt) = window(ctx, oracle, "stereo_60x5", 2)
    ctx.check(ctx.lib.me_ba_reserve(ctx.h, 30, 400, 4000, 4, 2), "me_ba_reserve")
    dev = DeviceBAProblem(bp, ctx)
    try:
        dev.covariance_full_async()
        ok, cam, pt = dev.covariance_read()
        assert ok == 1
        C.assert_cam_blocks(cam, rcam)
        C.assert_pt_blocks(pt, rpt)
    finally:
        dev.close()


def test_cpp_mirror_prints_the_python_blocks(ctx, tmp_path):
    """tests/cpp/ba_cov_cli (BundleAdjuster<M> of the C++ mirror with compute_cov: getPosesCovariance and
    getPointsCovariance), compiled here with one compiler command, against the Python entry points."""
    import os
    import struct
    import subprocess

    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_covariance_full, ba_solve

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = str(tmp_path / "ba_cov_cli")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "ba_cov_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True, timeout=120)
    for bp in (S.ba_problem(42, 60, 5, 640, 480), S.ba_problem_mono(51, 60, 5, 640, 480)):
        od = getattr(bp, "obs_dim", 4)
        payload = struct.pack("<iiiii", len(bp.cams), len(bp.pts), len(bp.obs), bp.fixed_frames, od)
        payload += np.asarray(bp.K0, np.float64).tobytes() + np.asarray(bp.K1, np.float64).tobytes()
        payload += struct.pack("<dd", bp.baseline, bp.feat_var)
        payload += np.ascontiguousarray(bp.cams, np.float64).tobytes() + np.ascontiguousarray(bp.pts).tobytes()
        payload += np.ascontiguousarray(bp.obs, np.float64).tobytes()
        payload += np.ascontiguousarray(bp.cam_idx, np.int32).tobytes() + np.ascontiguousarray(bp.pt_idx).tobytes()
        if od == 2:
            payload += np.ascontiguousarray(bp.cam_id, np.int32).tobytes()
        fin, fout = tmp_path / f"in{od}.bin", tmp_path / f"out{od}.bin"
        fin.write_bytes(payload)
        # a missing or short input is an error message, not a read past the buffer
        short = tmp_path / f"short{od}.bin"
        short.write_bytes(payload[:len(payload) // 2])
        for bad in (str(short), str(tmp_path / "absent.bin")):
            p = subprocess.run([exe, bad, str(fout), "5"], capture_output=True, text=True, timeout=120)
            assert p.returncode in (1, 2) and "ba_cov_cli:" in p.stderr, (p.returncode, p.stderr)
        p = subprocess.run([exe, str(fin), str(fout), "5"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        out = fout.read_bytes()
        nc, npt = len(bp.cams), len(bp.pts)
        (status,) = struct.unpack_from("<i", out)
        off = 4
        cams = np.frombuffer(out, np.float64, 6 * nc, off).reshape(-1, 6)
        off += 48 * nc
        pts = np.frombuffer(out, np.float64, 3 * npt, off).reshape(-1, 3)
        off += 24 * npt
        (n,) = struct.unpack_from("<i", out, off)
        assert n == nc
        ccov = np.frombuffer(out, np.float64, 36 * n, off + 4).reshape(-1, 6, 6)
        off += 4 + 288 * n
        (n,) = struct.unpack_from("<i", out, off)
        assert n == npt
        pcov = np.frombuffer(out, np.float64, 9 * n, off + 4).reshape(-1, 3, 3)
        assert status == 2  # Status::SUCCESSFUL
        solved = bp.copy()
        solved.cams, solved.pts, _ = ba_solve(bp, SolverOptions.fixed_iterations(5), ctx=ctx)
        assert np.array_equal(cams, solved.cams) and np.array_equal(pts, solved.pts)
        rcam, rpt = ba_covariance_full(solved, ctx=ctx)
        C.assert_cam_blocks(ccov, rcam)
        C.assert_pt_blocks(pcov, rpt)


def test_bundle_adjuster_points_covariance(ctx, oracle):
    """BundleAdjuster fills getPointsCovariance beside getPosesCovariance when compute_cov is set."""
    from uasl_motion_estimation_amd.feature_types import CamPose, WBA_Point
    from uasl_motion_estimation_amd.optimisation import BundleAdjuster, CalibrationParameters, SolverOptions
    from uasl_motion_estimation_amd.rotation_utils import exp_map_Quat

    bp = S.ba_problem_mono(51, 60, 5, 640, 480)
    first_id = 100
    cams = [CamPose(first_id + i, exp_map_Quat(c[3:]), np.array(c[:3])) for i, c in enumerate(bp.cams)]
    tracks = []
    for j in range(len(bp.pts)):
        sel = np.nonzero(bp.pt_idx == j)[0]
        t = WBA_Point((float(bp.obs[sel[0], 0]), float(bp.obs[sel[0], 1])), first_id + int(bp.cam_idx[sel[0]]),
                      int(bp.cam_id[sel[0]]))
        for o in sel[1:]:
            t.addMatch((float(bp.obs[o, 0]), float(bp.obs[o, 1])), first_id + int(bp.cam_idx[o]))
        t.set3DLocation(np.array([*bp.pts[j], 1.0]))
        tracks.append(t)
    for compute_cov in (False, True):
        calib = CalibrationParameters([bp.K0], bp.feat_var, bp.baseline, compute_cov=compute_cov)
        ba = BundleAdjuster(calib, cams, tracks, ctx=ctx, options=SolverOptions.fixed_iterations(6))
        assert ba.optimise(bp.fixed_frames).name == "SUCCESSFUL"
        covs = ba.getPointsCovariance()
        if not compute_cov:
            assert covs == []
            continue
        assert len(covs) == len(bp.pts)
        solved = bp.copy()
        solved.cams, solved.pts = np.array(ba.m_camera_params), np.array(ba.m_point_params)
        rcam, rpt = C.ref_covariance(oracle, solved)
        C.assert_pt_blocks(np.array(covs), rpt)
        C.assert_cam_blocks(np.array(ba.getPosesCovariance()), rcam)
