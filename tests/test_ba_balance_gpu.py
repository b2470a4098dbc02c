"""BA camera assembly in balanced units and long tracks, against the CPU oracle.

The camera assembly deals every variable camera's observations out in units
of 256 slots (the plan's unit table, built on the device): camera c has
max(1, ceil(n_c / 256)) units, one workgroup each.  These windows put a
camera's count on the unit boundaries beside a camera of four units, skew the
cameras so that the heaviest needs more units than an even split would give,
and stretch tracks past the 16 and 32 lanes the point kernels give a landmark.
Every solve is held to the suite's BA bar: rtol 1e-6 / atol 1e-9 on cameras
and points with equal iteration, successful-step and termination counts.  The
windows were chosen on the CPU so that the oracle alone is finite and takes at
least one successful step (each test asserts that too)."""
import ctypes

import numpy as np
import pytest

from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

UNIT = 256
FIXED10 = dict(max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


def thin_camera(bp, cam, target):
    """`bp` with camera `cam` left `target` observations: its observations of
    the longest tracks go first (a track of three or more survives the loss),
    then landmarks left with fewer than 2 observations are dropped."""
    per_pt = np.bincount(bp.pt_idx, minlength=len(bp.pts))
    idx = np.flatnonzero(bp.cam_idx == cam)
    order = idx[np.argsort(-per_pt[bp.pt_idx[idx]], kind="stable")]
    keep = np.ones(len(bp.cam_idx), bool)
    keep[order[:len(idx) - target]] = False
    keep_pt = np.bincount(bp.pt_idx[keep], minlength=len(bp.pts)) >= 2
    keep &= keep_pt[bp.pt_idx]
    new_id = np.cumsum(keep_pt) - 1
    return S.BAProblem(bp.cams.copy(), bp.pts[keep_pt].copy(), np.ascontiguousarray(bp.obs[keep]),
                       bp.cam_idx[keep].copy(), new_id[bp.pt_idx[keep]].astype(np.int32), bp.K0, bp.K1, bp.baseline,
                       bp.feat_var, bp.fixed_frames, None, None, bp.obs_dim,
                       None if bp.cam_id is None else np.ascontiguousarray(bp.cam_id[keep]))


def camera_counts(bp):
    """Observations of every variable camera."""
    return np.bincount(bp.cam_idx, minlength=len(bp.cams))[bp.fixed_frames:]


def expected_units(bp):
    return int(sum(max(1, -(-int(n) // UNIT)) for n in camera_counts(bp)))


def unit_total(ctx):
    """The unit total the device plan of the ctx's last solve built (State::stamps[14])."""
    fn = ctx.lib.me_debug_read
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    buf = (ctypes.c_longlong * 16)()
    assert fn(ctx.h, buf, 16) == 0
    return int(buf[14])


def solve_and_compare(ctx, oracle, bp, fixed=True):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    rc, rp, rs = oracle.ba_solve(bp.copy(), **(FIXED10 if fixed else {}))
    assert np.isfinite(rc).all() and np.isfinite(rp).all() and rs["successful_steps"] >= 1, rs
    cams, pts, s = ba_solve(bp.copy(), SolverOptions.fixed_iterations(10) if fixed else None, ctx=ctx)
    assert unit_total(ctx) == expected_units(bp)
    assert (s["iterations"], s["successful_steps"], s["termination"]) == \
        (rs["iterations"], rs["successful_steps"], rs["termination"]), (s, rs)
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)
    return s, rs


# One variable camera thinned onto a unit boundary beside one of four units.
# 900 landmarks x 4 keyframes: cameras 374 / 676 / 869 / 807, cameras 2 and 3
# variable.  Thinning camera 2 to one observation takes the two-frame tracks
# of cameras 2 and 3 with it, so that case starts from 1200 landmarks
# (camera 3 keeps 772).
@pytest.mark.parametrize("n_pts,target", [(1200, 1), (900, 255), (900, 256), (900, 257), (900, 513)])
def test_ba_unit_boundaries(ctx, oracle, n_pts, target):
    bp = thin_camera(S.ba_problem(S.SEED0 + 21, n_pts, 4, 1280, 720), 2, target)
    n2, n3 = camera_counts(bp)
    assert n2 == target and n3 > 3 * UNIT, (n2, n3)
    solve_and_compare(ctx, oracle, bp)


def test_ba_unit_boundaries_mono(ctx, oracle):
    bp = thin_camera(S.ba_problem_mono(S.SEED0 + 21, 1300, 4, 1280, 720), 2, 257)
    n2, n3 = camera_counts(bp)
    assert n2 == 257 and n3 > 3 * UNIT, (n2, n3)
    solve_and_compare(ctx, oracle, bp)


# The heaviest camera needs more units than an even split of the observations
# over the variable cameras, ceil(no / (m 256)), would give it: 1000 x 14 has
# 4 against 3 (10 of 10 steps successful), 1500 x 10 has 6 against 5 (rejected
# steps among the 10).
@pytest.mark.parametrize("seed,n_pts,window", [(26, 1000, 14), (25, 1500, 10)])
def test_ba_skewed_cameras(ctx, oracle, seed, n_pts, window):
    bp = S.ba_problem(S.SEED0 + seed, n_pts, window, 1280, 720)
    counts = camera_counts(bp)
    even = -(-len(bp.cam_idx) // (len(counts) * UNIT))
    assert -(-int(counts.max()) // UNIT) > even, (counts, even)
    solve_and_compare(ctx, oracle, bp)


# 96 landmarks over W keyframes: the longest track has W observations (16: none
# over 16; 17, 20, 32: 5, 12, 36 tracks over 16; 40: 7 tracks over 32).  The
# oracle rejects steps at W = 16 and 32.
@pytest.mark.parametrize("window,over16,over32", [(16, 0, 0), (17, 5, 0), (20, 12, 0), (32, 36, 0), (40, 48, 7)])
def test_ba_long_tracks(ctx, oracle, window, over16, over32):
    bp = S.ba_problem(S.SEED0 + 22, 96, window, 1280, 720)
    per_pt = np.bincount(bp.pt_idx, minlength=len(bp.pts))
    assert per_pt.max() == window and (per_pt > 16).sum() == over16 and (per_pt > 32).sum() == over32
    solve_and_compare(ctx, oracle, bp)


# Default options (the function-tolerance stop): the oracle ends the
# 1025 x 6 window at 7 iterations with 6 successful steps, and the 20-keyframe
# long-track window by its tolerances as well.
@pytest.mark.parametrize("seed,n_pts,window", [(11, 1025, 6), (22, 96, 20)])
def test_ba_default_tolerances(ctx, oracle, seed, n_pts, window):
    bp = S.ba_problem(S.SEED0 + seed, n_pts, window, 1280, 720)
    s, rs = solve_and_compare(ctx, oracle, bp, fixed=False)
    assert rs["termination"] == 0 and rs["iterations"] < 50, rs
    if seed == 11:
        assert (rs["iterations"], rs["successful_steps"]) == (7, 6), rs
