"""BA with the linearisation inside the Schur pass, against the CPU oracle.

Small windows take the Schur instances that form each observation's residual,
Jacobian and normal-equation pieces in their own phase A (no linearize launch,
no V_o | g_o buffer).  Each window here is built for one way that phase can go
wrong: padding lanes and runs, second slots of a lane, fixed-camera slots that
contribute no W_o, duplicate residual blocks summed in CSR order, the stored
W_o read back by a pass that does not linearise (after a rejected step), the
mono model, and a rank's share of a sharded window.  Every solve is held to the
suite's BA bar: equal iteration, successful-step and termination counts, cameras
and points at rtol 1e-6 / atol 1e-9, initial and final cost at 1e-9 relative.
The windows were chosen on the CPU, with the oracle alone."""
import numpy as np
import pytest

from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

FIXED10 = dict(max_num_iterations=10, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


def keep_landmarks(bp, keep_pt):
    """`bp` restricted to the landmarks flagged in `keep_pt` (renumbered in order)."""
    keep = keep_pt[bp.pt_idx]
    new_id = np.cumsum(keep_pt) - 1
    return S.BAProblem(bp.cams.copy(), bp.pts[keep_pt].copy(), np.ascontiguousarray(bp.obs[keep]),
                       bp.cam_idx[keep].copy(), new_id[bp.pt_idx[keep]].astype(np.int32), bp.K0, bp.K1, bp.baseline,
                       bp.feat_var, bp.fixed_frames, None, None, bp.obs_dim,
                       None if bp.cam_id is None else np.ascontiguousarray(bp.cam_id[keep]))


def track_lengths(bp):
    return np.bincount(bp.pt_idx, minlength=len(bp.pts))


def first_of(mask, n):
    idx = np.flatnonzero(mask)
    assert len(idx) >= n, (len(idx), n)
    return idx[:n]


def solve_and_compare(ctx, oracle, bp):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    rc, rp, rs = oracle.ba_solve(bp.copy(), **FIXED10)
    assert np.isfinite(rc).all() and np.isfinite(rp).all() and rs["successful_steps"] >= 1, rs
    cams, pts, s = ba_solve(bp.copy(), SolverOptions.fixed_iterations(10), ctx=ctx)
    assert (s["iterations"], s["successful_steps"], s["termination"]) == \
        (rs["iterations"], rs["successful_steps"], rs["termination"]), (s, rs)
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(s["initial_cost"], rs["initial_cost"], rtol=1e-9)
    np.testing.assert_allclose(s["final_cost"], rs["final_cost"], rtol=1e-9)
    return s, rs


@pytest.fixture(scope="module")
def window20():
    """1800 landmarks x 20 keyframes: the pool the track-length windows are cut from."""
    return S.ba_problem(S.SEED0 + 32, 1800, 20, 1280, 720)


def test_ragged_runs(ctx, oracle):
    """70 landmarks x 6 keyframes: three runs of 32, the last with 6 landmarks and 26 padding lane groups."""
    bp = S.ba_problem(S.SEED0 + 31, 70, 6, 1280, 720)
    assert len(bp.pts) == 70 and len(bp.pts) % 32 != 0
    solve_and_compare(ctx, oracle, bp)


def test_long_tracks(ctx, oracle, window20):
    """40 landmarks seen in all 20 keyframes: every lane group has second slots (q0 + 16)."""
    per = track_lengths(window20)
    k = np.zeros(len(window20.pts), bool)
    k[first_of(per == 20, 40)] = True
    bp = keep_landmarks(window20, k)
    assert len(bp.pts) == 40 and (track_lengths(bp) == 20).all()
    solve_and_compare(ctx, oracle, bp)


def test_mixed_track_lengths(ctx, oracle, window20):
    """Tracks of 2, 16, 17 and 20 observations side by side: lane groups with one slot on two
    lanes only, exactly full, with one second slot and with four."""
    per = track_lengths(window20)
    k = np.zeros(len(window20.pts), bool)
    for length in (2, 16, 17, 20):
        k[first_of(per == length, 12)] = True
    bp = keep_landmarks(window20, k)
    assert sorted(np.unique(track_lengths(bp))) == [2, 16, 17, 20]
    solve_and_compare(ctx, oracle, bp)


def test_rejected_step(ctx, oracle):
    """96 landmarks x 16 keyframes: the oracle rejects two of the ten steps, so a pass without a
    linearisation reads the stored V, gps, psc and W_o."""
    bp = S.ba_problem(S.SEED0 + 22, 96, 16, 1280, 720)
    s, rs = solve_and_compare(ctx, oracle, bp)
    assert rs["successful_steps"] < rs["iterations"], rs


def test_fixed_camera_tracks(ctx, oracle):
    """Landmarks seen by the two fixed cameras only (no W_o at all) and landmarks with a single
    variable observation, beside ordinary ones.  The oracle rejects steps here as well."""
    pool = S.ba_problem(S.SEED0 + 36, 600, 6, 1280, 720, alive_frac=0.3)
    nvar = np.bincount(pool.pt_idx, weights=(pool.cam_idx >= pool.fixed_frames).astype(float), minlength=len(pool.pts))
    k = np.zeros(len(pool.pts), bool)
    k[first_of(nvar == 0, 18)] = True
    k[first_of(nvar == 1, 20)] = True
    k[first_of(nvar >= 2, 50)] = True
    bp = keep_landmarks(pool, k)
    nv = np.bincount(bp.pt_idx, weights=(bp.cam_idx >= bp.fixed_frames).astype(float), minlength=len(bp.pts))
    assert (nv == 0).sum() == 18 and (nv == 1).sum() == 20
    solve_and_compare(ctx, oracle, bp)


def test_duplicate_observations(ctx, oracle):
    """40 observations repeated with another measurement (same landmark, same camera, fixed
    cameras among them): the duplicate residual blocks of a camera add in CSR order."""
    bp = S.ba_problem(S.SEED0 + 37, 90, 6, 1280, 720)
    rng = np.random.default_rng(5)
    pick = rng.choice(len(bp.obs), 40, replace=False)
    assert (bp.cam_idx[pick] < bp.fixed_frames).any() and (bp.cam_idx[pick] >= bp.fixed_frames).any()
    obs = np.concatenate([bp.obs, bp.obs[pick] + rng.normal(0.0, 0.3, (40, 4))])
    dup = S.BAProblem(bp.cams, bp.pts, np.ascontiguousarray(obs),
                      np.concatenate([bp.cam_idx, bp.cam_idx[pick]]).astype(np.int32),
                      np.concatenate([bp.pt_idx, bp.pt_idx[pick]]).astype(np.int32), bp.K0, bp.K1, bp.baseline,
                      bp.feat_var, bp.fixed_frames)
    solve_and_compare(ctx, oracle, dup)


def test_mono(ctx, oracle):
    """The mono model (two residual rows, left or right image per track) on a small window."""
    bp = S.ba_problem_mono(S.SEED0 + 38, 150, 6, 1280, 720)
    assert bp.obs_dim == 2 and (bp.cam_id == 0).any() and (bp.cam_id != 0).any()
    s, rs = solve_and_compare(ctx, oracle, bp)
    assert rs["successful_steps"] < rs["iterations"], rs


def test_sharded_two_contexts(ctx):
    """A 100-landmark window sharded over two contexts through the callback communicator
    (each rank's Schur pass linearises its own landmarks and sums its own cost partials)
    against the single-device solve."""
    from test_distributed import _two_ctx_comm_solve
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(S.SEED0 + 39, 100, 6, 1280, 720)
    opts = SolverOptions.fixed_iterations(10)
    ref_c, ref_p, ref_s = ba_solve(bp.copy(), opts, ctx=ctx)
    cams, pts, summ = _two_ctx_comm_solve(bp, opts)
    for c, s in zip(cams, summ):
        assert (s["iterations"], s["successful_steps"], s["termination"]) == \
            (ref_s["iterations"], ref_s["successful_steps"], ref_s["termination"]), (s, ref_s)
        np.testing.assert_allclose(c, ref_c, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(s["initial_cost"], ref_s["initial_cost"], rtol=1e-9)
        np.testing.assert_allclose(s["final_cost"], ref_s["final_cost"], rtol=1e-9)
    np.testing.assert_allclose(pts, ref_p, rtol=1e-6, atol=1e-9)
