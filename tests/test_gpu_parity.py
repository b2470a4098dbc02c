"""GPU parity tests: libme_hip.so (through the C ABI) vs the CPU restatement.

Bars (north star):
  * MI scores, histograms, NMS maxima/order, KLT positions/status, ROI
    decisions of the scale optimiser: bit-exact;
  * BA pose / point parameters: 1e-6 relative (FP64, reduction order differs);
  * scale optimiser: identical stop condition and scale within 1e-9.
"""
import numpy as np
import pytest

from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ MI (A1/A2)
@pytest.mark.parametrize("patch", [(11, 11), (10, 10), (15, 15), (3, 7), (1, 1)])
def test_mi_scores_bit_exact(ctx, oracle, patch):
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    pw, ph = patch
    L, R, xyL, xyR = S.random_patches(100 + pw, 320, 240, 4099, pw, ph)
    got = mi_scores(L, R, xyL, xyR, patch, ctx=ctx)
    ref = oracle.mi_scores(L, R, xyL, xyR, pw, ph)
    assert np.array_equal(bits(got), bits(ref)), np.flatnonzero(bits(got) != bits(ref))[:10]


@pytest.mark.parametrize("patch", [(11, 11), (10, 10), (12, 12), (13, 13), (3, 7), (1, 1), (12, 15), (9, 14)])
def test_mi_large_batch_bit_exact(ctx, oracle, patch):
    """>= 32768 pairs take the four-lanes-per-pair table-driven batch kernel
    (11x11, 10x10 compiled shapes; any other <= 12 px wide shape the generic
    instance, taller ones included); corners hug the right / bottom image edges
    so the realigned row loads hit their bounds."""
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    pw, ph = patch
    W, H = 161, 97
    L, R, xyL, xyR = S.random_patches(200 + pw, W, H, 40000, pw, ph)
    xyL[:500, 0] = W - pw
    xyL[500:1000, 1] = H - ph
    xyR[1000:1500] = [W - pw, H - ph]
    got = mi_scores(L, R, xyL, xyR, patch, ctx=ctx)
    ref = oracle.mi_scores(L, R, xyL, xyR, pw, ph)
    assert np.array_equal(bits(got), bits(ref)), np.flatnonzero(bits(got) != bits(ref))[:10]


@pytest.mark.parametrize("patch", [(11, 11), (12, 16), (5, 3), (13, 13)])
def test_mi_small_batch_edges_bit_exact(ctx, oracle, patch):
    """< 32768 pairs take the 16-lane group kernel: its row form loads each
    patch row as a 16-byte window (inside both images), else per-pixel bytes;
    corners on the last row / column and the image's last byte exercise the
    bound (odd width: rows not 4-byte aligned)."""
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    pw, ph = patch
    W, H = 97, 61
    L, R, xyL, xyR = S.random_patches(400 + pw, W, H, 3000, pw, ph)
    xyL[:200, 0] = W - pw
    xyL[200:400, 1] = H - ph
    xyR[400:600] = [W - pw, H - ph]
    xyL[600:800] = [W - pw, H - ph]
    got = mi_scores(L, R, xyL, xyR, patch, ctx=ctx)
    ref = oracle.mi_scores(L, R, xyL, xyR, pw, ph)
    assert np.array_equal(bits(got), bits(ref)), np.flatnonzero(bits(got) != bits(ref))[:10]


def _tile_patterns(patterns, W, H, n, rng):
    """Images holding the given 11x11 (L, R) patch patterns side by side, and
    n corner pairs that each select one pattern (both images at the same spot)."""
    L = rng.integers(0, 256, (H, W)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W)).astype(np.uint8)
    per_row = W // 11
    corners = []
    for i, (pl, pr) in enumerate(patterns):
        y, x = 11 * (i // per_row), 11 * (i % per_row)
        L[y:y + 11, x:x + 11] = pl
        R[y:y + 11, x:x + 11] = pr
        corners.append((x, y))
    pick = rng.integers(0, len(corners), n)
    xy = np.array(corners, np.int32)[pick]
    return L, R, np.ascontiguousarray(xy), np.ascontiguousarray(xy.copy())


def test_mi_batch_extreme_bin_patterns(ctx, oracle):
    """The batch kernel's bounds: a pair with 121 distinct joint bins (a lane
    run of 31 terms, the register array's limit), every one of the 20 rows
    populated (the row table full, its two sentinels right after), a single
    bin (one lane does all), one bin per row down the diagonal, and random
    pairs, mixed in every 16-pair wave (>= 32768 pairs: the quad kernel)."""
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    rng = np.random.default_rng(11)
    mid = lambda b: np.uint8(min(255, (64 * b + 63) // 5))  # noqa: E731  a value in bin b ((5 v) >> 6 == b)
    assert all((5 * int(mid(b))) >> 6 == b for b in range(20))
    pats = []
    codes = rng.permutation(400)[:121]  # 121 distinct joint bins
    pats.append((np.array([mid(c // 20) for c in codes], np.uint8).reshape(11, 11),
                 np.array([mid(c % 20) for c in codes], np.uint8).reshape(11, 11)))
    rows = np.concatenate([np.arange(20).repeat(6), [19]])  # all 20 rows, 6-7 pixels each, random columns
    pats.append((np.array([mid(r) for r in rows], np.uint8).reshape(11, 11),
                 np.array([mid(c) for c in rng.integers(0, 20, 121)], np.uint8).reshape(11, 11)))
    pats.append((np.full((11, 11), mid(7), np.uint8), np.full((11, 11), mid(13), np.uint8)))  # one bin
    diag = np.array([mid(r) for r in rows], np.uint8).reshape(11, 11)
    pats.append((diag, diag.copy()))  # 20 rows, one bin each
    for _ in range(4):
        pats.append((rng.integers(0, 256, (11, 11)).astype(np.uint8), rng.integers(0, 256, (11, 11)).astype(np.uint8)))
    L, R, xyL, xyR = _tile_patterns(pats, 11 * 8, 11 * 2, 40000, rng)
    got = mi_scores(L, R, xyL, xyR, (11, 11), ctx=ctx)
    ref = oracle.mi_scores(L, R, xyL, xyR, 11, 11)
    assert np.array_equal(bits(got), bits(ref)), np.flatnonzero(bits(got) != bits(ref))[:10]


def test_mi_edge_patches(ctx, oracle):
    from uasl_motion_estimation_amd.mutual_information import computeEntropy, computeMutualInformation

    rng = np.random.default_rng(5)
    cases = [np.full((11, 11), 200, np.uint8), np.zeros((11, 11), np.uint8), rng.integers(0, 256, (11, 11)),
             rng.integers(0, 256, (10, 10)), rng.integers(0, 256, (37, 53)), rng.integers(0, 256, (480, 640))]
    for A in cases:
        A = A.astype(np.uint8)
        B = np.roll(A, 3, axis=1)
        for X, Y in ((A, B), (A, A), (B, 255 - A)):
            got = computeMutualInformation(X, Y, ctx)
            assert np.float32(got).view(np.uint32) == np.float32(oracle.mutual_information(X, Y)).view(np.uint32)
        assert np.float32(computeEntropy(A, ctx)) == np.float32(oracle.entropy(A))


def test_mi_batch_empty_and_single(ctx, oracle):
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    L, R, xyL, xyR = S.random_patches(3, 64, 48, 1, 11, 11)
    assert mi_scores(L, R, xyL[:0], xyR[:0], (11, 11), ctx=ctx).shape == (0,)
    got = mi_scores(L, R, xyL, xyR, (11, 11), ctx=ctx)
    assert np.array_equal(bits(got), bits(oracle.mi_scores(L, R, xyL, xyR, 11, 11)))


def test_mi_rejects_out_of_image(ctx):
    from uasl_motion_estimation_amd import MEError
    from uasl_motion_estimation_amd.mutual_information import mi_scores

    L = np.zeros((20, 20), np.uint8)
    with pytest.raises(MEError):
        mi_scores(L, L, np.array([[15, 0]], np.int32), np.array([[0, 0]], np.int32), (11, 11), ctx=ctx)


# ------------------------------------------------------------------ ScaleState (A4-A8)
@pytest.fixture(scope="module")
def scale_prob():
    return S.scale_problem(3, 640, 480, 300)


def test_scale_residuals_bit_exact(ctx, oracle, scale_prob):
    from uasl_motion_estimation_amd.optimisation import scale_residuals

    got = scale_residuals(scale_prob, ctx=ctx)
    ref = oracle.scale_residuals(scale_prob)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:10]


def test_scale_residuals_with_mask_and_weighting(ctx, oracle, scale_prob):
    import dataclasses

    from uasl_motion_estimation_amd.optimisation import scale_residuals

    n = len(scale_prob.X_left) + len(scale_prob.X_right)
    mask = (np.random.default_rng(1).random(n) < 0.8).astype(np.uint8)
    sp = dataclasses.replace(scale_prob, mask=mask)
    try:
        ref = oracle.scale_residuals(sp)
    except RuntimeError:
        pytest.skip("mask selects fewer rows than tracks (reference UB)")
    got = scale_residuals(sp, ctx=ctx)
    assert np.array_equal(got, ref)
    got_w = scale_residuals(scale_prob, weighting=True, ctx=ctx)
    ref_w = oracle.scale_residuals(scale_prob, weighting=1)
    assert np.array_equal(got_w, ref_w)


def test_scale_normal_equations(ctx, oracle, scale_prob):
    from uasl_motion_estimation_amd.optimisation import scale_normal_equations

    r = oracle.scale_residuals(scale_prob)
    JJ, e = scale_normal_equations(scale_prob, r, ctx=ctx)
    rJJ, re = oracle.scale_normal_equations(scale_prob, r)
    np.testing.assert_allclose([JJ, e], [rJJ, re], rtol=1e-12)


def test_scale_jacobian(ctx, oracle, scale_prob):
    from uasl_motion_estimation_amd.optimisation import scale_jacobian

    np.testing.assert_allclose(scale_jacobian(scale_prob, ctx=ctx), oracle.scale_jacobian(scale_prob), rtol=1e-12)


@pytest.mark.parametrize("seed,scale0", [(3, 1.02), (4, 0.97), (5, 1.0)])
def test_scale_optimise(ctx, oracle, seed, scale0):
    import dataclasses

    from uasl_motion_estimation_amd.optimisation import scale_optimise

    sp = dataclasses.replace(S.scale_problem(seed, 640, 480, 300), scale=scale0)
    got = scale_optimise(sp, ctx=ctx)
    ref = oracle.scale_optimise(sp)
    assert int(got["stop"]) == ref["stop"]
    assert got["iterations"] == ref["iterations"]
    np.testing.assert_allclose(got["scale"], ref["scale"], rtol=1e-9)
    np.testing.assert_allclose(got["trace"], ref["trace"], rtol=1e-9)


def test_scale_optimise_test_mode(ctx, oracle, scale_prob):
    from uasl_motion_estimation_amd.optimisation import scale_optimise

    got = scale_optimise(scale_prob, test=True, ctx=ctx)
    ref = oracle.scale_optimise(scale_prob, test=1)
    assert int(got["stop"]) == ref["stop"] and got["iterations"] == ref["iterations"]
    np.testing.assert_allclose(got["scale"], ref["scale"], rtol=1e-12)


def test_scale_inliers(ctx, oracle, scale_prob):
    from uasl_motion_estimation_amd.optimisation import scale_inliers

    assert np.array_equal(scale_inliers(scale_prob, 1.5, ctx=ctx), oracle.scale_inliers(scale_prob, 1.5))


# ------------------------------------------------------------------ BA (A13-A17)
@pytest.fixture(scope="module")
def ba_small():
    return S.ba_problem(21, 250, 8, 640, 480)


def test_ba_residuals_and_jacobians(ctx, oracle, ba_small):
    from uasl_motion_estimation_amd.optimisation import ba_evaluate

    r, Jc, Jp = ba_evaluate(ba_small, ctx=ctx)
    rr, rJc, rJp = oracle.ba_evaluate(ba_small)
    np.testing.assert_allclose(r, rr, rtol=1e-12, atol=1e-9)
    scale_c = np.abs(rJc).max()
    scale_p = np.abs(rJp).max()
    np.testing.assert_allclose(Jc, rJc, rtol=1e-9, atol=1e-12 * scale_c)
    np.testing.assert_allclose(Jp, rJp, rtol=1e-9, atol=1e-12 * scale_p)


def test_ba_cost(ctx, oracle, ba_small):
    from uasl_motion_estimation_amd.optimisation import ba_cost

    np.testing.assert_allclose(ba_cost(ba_small, ctx=ctx), oracle.ba_cost(ba_small), rtol=1e-12)


def test_ba_reduced_system(ctx, oracle, ba_small):
    from uasl_motion_estimation_amd.optimisation import ba_reduced_system

    S_, b = ba_reduced_system(ba_small, 1e4, ctx=ctx)
    rS, rb, rc = oracle.ba_reduced_system(ba_small, 1e4)
    assert rc == 0
    np.testing.assert_allclose(S_, rS, rtol=1e-9, atol=1e-9 * np.abs(rS).max())
    np.testing.assert_allclose(b, rb, rtol=1e-9, atol=1e-9 * np.abs(rb).max())


@pytest.mark.parametrize("seed,n,w,fixed", [(21, 250, 8, 2), (22, 120, 5, 2), (23, 400, 12, 1), (24, 60, 4, 0)])
def test_ba_solve_default_options(ctx, oracle, seed, n, w, fixed):
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = S.ba_problem(seed, n, w, 640, 480, fixed=fixed)
    cams, pts, s = ba_solve(bp, ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp)
    assert s["iterations"] == rs["iterations"] and s["termination"] == rs["termination"], (s, rs)
    assert s["status"] == rs["status"] == 2
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(s["final_cost"], rs["final_cost"], rtol=1e-9)


def test_ba_fixed_iterations_config2(ctx, oracle):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    c = S.CONFIGS[2]
    bp = S.ba_problem(S.SEED0 + 2, c["n_feats"], c["window"], c["width"], c["height"])
    cams, pts, s = ba_solve(bp, SolverOptions.fixed_iterations(10), ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp, max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0,
                                 parameter_tolerance=0.0)
    assert s["iterations"] == rs["iterations"] == 10
    assert s["successful_steps"] == rs["successful_steps"]
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)


def test_ba_infeasible_start_fails(ctx):
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = S.ba_problem(25, 30, 4, 320, 240)
    bp.pts[0, 2] = 1e9  # beyond Zmax -> Ceres refuses the problem
    cams, pts, s = ba_solve(bp, ctx=ctx)
    assert s["status"] == 3
    assert np.array_equal(cams, bp.cams)


# ------------------------------------------------------------------ NMS (A11)
@pytest.mark.parametrize("kind", ["smooth", "plateaus", "ties", "tiny"])
def test_nms_bit_exact(ctx, oracle, kind):
    from uasl_motion_estimation_amd.feature_types import nonMaxSupScanline3x3

    rng = np.random.default_rng({"smooth": 1, "plateaus": 2, "ties": 3, "tiny": 4}[kind])
    if kind == "smooth":
        resp = rng.random((300, 400))
    elif kind == "plateaus":
        resp = np.floor(rng.random((200, 260)) * 4.0)
    elif kind == "ties":
        resp = np.kron(rng.integers(0, 3, (50, 70)), np.ones((2, 3))).astype(np.float64)
    else:
        resp = rng.random((3, 3))
    got, gmask = nonMaxSupScanline3x3(resp, ctx)
    ref, rmask = oracle.nms(resp)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)
    assert np.array_equal(gmask, rmask)


def test_nms_tall_image_multi_pass(ctx, oracle):
    from uasl_motion_estimation_amd.feature_types import nonMaxSupScanline3x3

    rng = np.random.default_rng(9)
    resp = np.floor(rng.random((2100, 40)) * 3.0)
    got, gm = nonMaxSupScanline3x3(resp, ctx)
    ref, rm = oracle.nms(resp)
    assert np.array_equal(got, ref) and np.array_equal(gm, rm)


# ------------------------------------------------------------------ KLT (A12)
def test_klt_bit_exact(ctx, oracle):
    from uasl_motion_estimation_amd.klt import calcOpticalFlowPyrLK

    scene, K, frames = S.stereo_stream(31, 640, 480, 2)
    rng = np.random.default_rng(0)
    pts = S.grid_features(rng, 500, 640, 480, 8).astype(np.float32)
    pts[:5] = [[1, 1], [639, 479], [-5, 10], [320.5, 240.25], [630, 10]]  # border cases
    got, gst = calcOpticalFlowPyrLK(frames[0].left, frames[1].left, pts, ctx=ctx)
    ref, rst = oracle.klt(frames[0].left, frames[1].left, pts)
    assert np.array_equal(gst, rst)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert gst.mean() > 0.8


@pytest.mark.parametrize("w,h,shift", [(640, 480, (13.3, -9.6)), (1280, 720, (2.5, 1.25)), (40, 30, (1.5, 0.5)),
                                       (200, 24, (3.0, 0.0))])
def test_klt_region_staging_bit_exact(ctx, oracle, w, h, shift):
    """Large displacements walk the window out of the LDS-staged region
    (restaging); levels under 32 px read global memory directly."""
    from uasl_motion_estimation_amd.klt import calcOpticalFlowPyrLK

    rng = np.random.default_rng(int(w + h))
    big = np.kron(rng.integers(0, 256, ((h + 3) // 4 + 16, (w + 3) // 4 + 16)), np.ones((4, 4)))
    big = (big + rng.integers(0, 16, big.shape)).clip(0, 255).astype(np.uint8)
    prev = np.ascontiguousarray(big[32:32 + h, 32:32 + w])
    ox, oy = int(32 + round(shift[0])), int(32 + round(shift[1]))
    nxt = np.ascontiguousarray(big[oy:oy + h, ox:ox + w])
    margin = min(12, w // 4, h // 4)
    pts = S.grid_features(rng, 300, w, h, margin).astype(np.float32)
    got, gst = calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx)
    ref, rst = oracle.klt(prev, nxt, pts)
    assert np.array_equal(gst, rst)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ------------------------------------------------------------------ device-resident BA windows
def test_ba_device_resident_matches_host_bit_exact(ctx):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions, ba_solve

    bp = S.ba_problem(31, 400, 10, 640, 480)
    hc, hp, hs = ba_solve(bp.copy(), SolverOptions.fixed_iterations(6), ctx=ctx)
    d = DeviceBAProblem(bp, ctx)
    ds = d.solve(SolverOptions.fixed_iterations(6))
    dc, dp = d.download()
    assert ds == hs
    assert np.array_equal(dc, hc) and np.array_equal(dp, hp)
    d.reset()
    ds2 = d.solve(SolverOptions.fixed_iterations(6))
    assert ds2 == hs and np.array_equal(d.download()[0], hc)
    d.close()


def test_ba_device_resident_bad_index_and_infeasible(ctx):
    from uasl_motion_estimation_amd._lib import MEError
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem

    bp = S.ba_problem(32, 50, 5, 640, 480)
    bad = bp.copy()
    bad.pt_idx = bp.pt_idx.copy()
    bad.pt_idx[3] = len(bp.pts) + 7
    d = DeviceBAProblem(bad, ctx)
    with pytest.raises(MEError):
        d.solve()
    d.close()
    inf = bp.copy()
    inf.pts[0, 2] = -5.0  # behind the camera: outside the Z box (BundleAdjuster.h:455-460)
    d = DeviceBAProblem(inf, ctx)
    s = d.solve()
    assert s["status"] == 3 and s["iterations"] == 0 and np.isnan(s["final_cost"])
    assert np.array_equal(d.download()[1], inf.pts)  # parameters untouched
    d.close()


def test_scale_device_resident_tracks_match_host(ctx, oracle):
    from uasl_motion_estimation_amd.optimisation import DeviceScaleTracks, scale_optimise

    sp = S.scale_problem(33, 320, 240, 300, window=5, w=5)
    ref = oracle.scale_optimise(sp)
    host = scale_optimise(sp, ctx=ctx)
    d = DeviceScaleTracks(sp, ctx)
    dev = scale_optimise(sp, ctx=ctx, dev_tracks=d.d)
    d.close()
    assert int(host["stop"]) == int(dev["stop"]) == int(ref["stop"])
    assert host["iterations"] == dev["iterations"] == ref["iterations"]
    assert host["scale"] == dev["scale"]
    np.testing.assert_allclose(dev["scale"], ref["scale"], rtol=1e-9)
    np.testing.assert_allclose(dev["trace"], ref["trace"], rtol=1e-9)


# ------------------------------------------------------------------ BA edge cases and large windows
@pytest.mark.parametrize("w,n,iters", [(30, 150, 4), (40, 120, 3), (21, 200, 5)])
def test_ba_large_windows_schur_variants(ctx, oracle, w, n, iters):
    """Windows past config 3 select the wider Schur instances (9 / 16 tiles per
    wave, with spills) -- same results as the restatement."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(60 + w, n, w, 640, 480)
    cams, pts, s = ba_solve(bp, SolverOptions.fixed_iterations(iters), ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp, max_num_iterations=iters, function_tolerance=0.0, gradient_tolerance=0.0,
                                 parameter_tolerance=0.0)
    assert s["iterations"] == rs["iterations"] and s["successful_steps"] == rs["successful_steps"]
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)


def test_ba_all_cameras_fixed(ctx, oracle):
    """fixedFrames >= window: every camera block constant, only the points move."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(71, 80, 4, 640, 480, fixed=4)
    cams, pts, s = ba_solve(bp, SolverOptions.fixed_iterations(5), ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp, max_num_iterations=5, function_tolerance=0.0, gradient_tolerance=0.0,
                                 parameter_tolerance=0.0)
    assert np.array_equal(cams, bp.cams)
    assert s["iterations"] == rs["iterations"]
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)


def test_ba_duplicate_observations(ctx, oracle):
    """Two residual blocks on the same (camera, point) pair are both summed (Ceres adds both)."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(72, 100, 6, 640, 480)
    k = np.arange(0, len(bp.obs), 7)
    bp.obs = np.vstack([bp.obs, bp.obs[k] + 0.3])
    bp.cam_idx = np.concatenate([bp.cam_idx, bp.cam_idx[k]]).astype(np.int32)
    bp.pt_idx = np.concatenate([bp.pt_idx, bp.pt_idx[k]]).astype(np.int32)
    cams, pts, s = ba_solve(bp, SolverOptions.fixed_iterations(6), ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp, max_num_iterations=6, function_tolerance=0.0, gradient_tolerance=0.0,
                                 parameter_tolerance=0.0)
    assert s["successful_steps"] == rs["successful_steps"]
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)


def test_ba_config5_window_50(ctx, oracle):
    """Config 5's 50-keyframe window: 48 variable cameras, a 289-column camera
    system (19 tiles, the widest Schur instance, S in global memory)."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(73, 150, 50, 1280, 720)
    assert len(bp.cams) - bp.fixed_frames == 48
    cams, pts, s = ba_solve(bp, SolverOptions.fixed_iterations(3), ctx=ctx)
    rc, rp, rs = oracle.ba_solve(bp, max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                                 parameter_tolerance=0.0)
    assert s["iterations"] == rs["iterations"] and s["successful_steps"] == rs["successful_steps"]
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------ asynchronous BA solve
def test_ba_solve_async_matches_sync_device_and_host(ctx, scale_prob):
    """me_ba_solve_async + me_ba_wait == me_ba_solve bit for bit, with other
    work (a scale LM) queued on the ctx between the two calls."""
    import ctypes

    from uasl_motion_estimation_amd._lib import BASummaryC
    from uasl_motion_estimation_amd.optimisation import (DeviceBAProblem, SolverOptions, ba_solve, ba_struct,
                                                         scale_optimise)

    bp = S.ba_problem(41, 300, 10, 640, 480)
    opts = SolverOptions.fixed_iterations(6)
    hc, hp, hs = ba_solve(bp.copy(), opts, ctx=ctx)
    d = DeviceBAProblem(bp, ctx)
    d.solve_async(opts)
    sc = scale_optimise(scale_prob, ctx=ctx)  # uses the ctx's own pinned staging meanwhile
    ds = d.wait()
    dc, dp = d.download()
    assert ds == hs and np.array_equal(dc, hc) and np.array_equal(dp, hp)
    assert sc["scale"] == scale_optimise(scale_prob, ctx=ctx)["scale"]
    # host-memory problem: results land in the caller's arrays at me_ba_wait
    keep = []
    p, cams, pts = ba_struct(bp.copy(), keep)
    o = opts.to_c()
    ctx.check(ctx.lib.me_ba_solve_async(ctx.h, ctypes.byref(p), ctypes.byref(o)), "async")
    s = BASummaryC()
    ctx.check(ctx.lib.me_ba_wait(ctx.h, ctypes.byref(s)), "wait")
    assert s.iterations == hs["iterations"] and np.array_equal(cams, hc) and np.array_equal(pts, hp)
    d.close()


def test_ba_async_drained_by_next_call_and_wait_errors(ctx):
    """A second BA call completes the pending solve; me_ba_wait without a
    pending solve is ME_ERR_STATE."""
    from uasl_motion_estimation_amd._lib import MEError
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions, ba_cost

    bp = S.ba_problem(42, 200, 8, 640, 480)
    opts = SolverOptions.fixed_iterations(4)
    d = DeviceBAProblem(bp, ctx)
    ref = d.solve(opts)
    ref_c = d.download()[0]
    d.reset()
    d.solve_async(opts)
    ba_cost(bp, ctx=ctx)  # another BA entry point: completes the pending solve first
    assert d.wait() == ref and np.array_equal(d.download()[0], ref_c)
    with pytest.raises(MEError):
        d.wait()
    d.close()


def test_ba_async_two_queued_windows(ctx):
    """Two windows queued back to back (the second in the other scratch /
    staging set while the first is in flight) give the synchronous results bit
    for bit, waited oldest first; a third queued solve before a wait is
    ME_ERR_STATE."""
    from uasl_motion_estimation_amd._lib import MEError
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions

    opts = SolverOptions.fixed_iterations(5)
    probs = [S.ba_problem(51, 400, 12, 640, 480), S.ba_problem(52, 300, 10, 640, 480)]
    ds = [DeviceBAProblem(bp, ctx) for bp in probs]
    ref = []
    for d in ds:
        ref.append((d.solve(opts), *d.download()))
        d.reset()
    for _ in range(2):  # twice: the sets alternate
        ds[0].solve_async(opts)
        ds[1].solve_async(opts)
        with pytest.raises(MEError):
            ds[0].solve_async(opts)
        for d, (rs, rc, rp) in zip(ds, ref):
            assert d.wait() == rs
            c, p = d.download()
            assert np.array_equal(c, rc) and np.array_equal(p, rp)
            d.reset()
    for d in ds:
        d.close()


def test_mi_lane_kernel_still_bit_exact(ctx, oracle):
    """The one-lane-per-pair batch kernel (test hook me_debug_solve_flags bit
    32768, the alternative of mi_quad_kernel) still matches the oracle bit for
    bit."""
    import ctypes

    from uasl_motion_estimation_amd.mutual_information import mi_scores

    hook = ctx.lib.me_debug_solve_flags
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hook(ctx.h, 32768) == 0
    try:
        for pw, ph in ((11, 11), (10, 10), (7, 9)):
            L, R, xyL, xyR = S.random_patches(300 + pw, 161, 97, 40000, pw, ph)
            got = mi_scores(L, R, xyL, xyR, (pw, ph), ctx=ctx)
            ref = oracle.mi_scores(L, R, xyL, xyR, pw, ph)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (pw, ph)
    finally:
        assert hook(ctx.h, 0) == 0
