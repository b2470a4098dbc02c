"""BA with per-camera rotation tables, against the CPU oracle.

The linearisation (linearize_kernel, the fused phase A of pt_schur_kernel) and
the camera assembly take each camera's rotation matrix R and angle-axis
derivative matrix M from a table built once per camera (plan_count_kernel for
the starting cameras, the camera workgroup of pt_step_kernel for every
candidate) instead of rebuilding them per observation.  Each window here is
built for one way the table can go wrong: an entry on the other side of the
small-angle branch than its camera, a rejected candidate's table read as the
current one, the launches that read the table from another kernel
(linearize_kernel, the stand-alone camera assembly), two solves in flight with
one table between them, a rank's table in a sharded solve, and a failed camera
solve that builds no table.  Every solve runs SolverOptions.fixed_iterations(10)
and is held to the suite's BA bar: equal iteration and successful-step counts,
cameras and points at rtol 1e-6 / atol 1e-9, initial and final cost at 1e-9
relative.  The windows were chosen on the CPU, with the oracle alone."""
import ctypes

import numpy as np
import pytest

from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

FIXED = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
DBL_EPS = 2.220446049250313e-16  # rotate()'s branch: theta^2 > DBL_EPSILON takes the Rodrigues form


def oracle_solve(oracle, bp, iters=10):
    rc, rp, rs = oracle.ba_solve(bp.copy(), max_num_iterations=iters, **FIXED)
    assert np.isfinite(rc).all() and np.isfinite(rp).all() and np.isfinite(rs["final_cost"]), rs
    return rc, rp, rs


def compare(got, ref):
    (cams, pts, s), (rc, rp, rs) = got, ref
    assert (s["iterations"], s["successful_steps"]) == (rs["iterations"], rs["successful_steps"]), (s, rs)
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(s["initial_cost"], rs["initial_cost"], rtol=1e-9)
    np.testing.assert_allclose(s["final_cost"], rs["final_cost"], rtol=1e-9)


def solve_and_compare(ctx, oracle, bp):
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    ref = oracle_solve(oracle, bp)
    assert ref[2]["iterations"] == 10 and ref[2]["successful_steps"] >= 1, ref[2]
    compare(ba_solve(bp.copy(), SolverOptions.fixed_iterations(10), ctx=ctx), ref)
    return ref[2]


def geometry(ctx, nc, nf, n_pts):
    fn = ctx.lib.me_debug_ba_geometry
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    out = (ctypes.c_int * 10)()
    assert fn(nc, nf, n_pts, out) == 0
    return tuple(out)


@pytest.mark.parametrize("obs_dim", [4, 2])
def test_branch_boundary(ctx, oracle, obs_dim):
    """60 landmarks x 6 keyframes, two fixed cameras.  The variable cameras start at rotations
    (0, 0, 0), (1e-8, 0, 0) (theta^2 = 1e-16, the small-angle branch), (1.5e-8, 0, 0)
    (theta^2 = 2.25e-16, just above DBL_EPSILON: the Rodrigues branch with theta ~ 1e-8) and a
    generic one; fixed camera 1 is rotated, fixed camera 0 is not."""
    if obs_dim == 4:
        bp = S.ba_problem(S.SEED0 + 61, 60, 6, 1280, 720)
    else:
        bp = S.ba_problem_mono(S.SEED0 + 61, 60, 6, 1280, 720, min_len=2)
    assert len(bp.pts) == 60 and len(bp.cams) == 6 and bp.fixed_frames == 2 and bp.obs_dim == obs_dim
    bp.cams = bp.cams.copy()
    bp.cams[2, 3:] = (0.0, 0.0, 0.0)
    bp.cams[3, 3:] = (1e-8, 0.0, 0.0)
    bp.cams[4, 3:] = (1.5e-8, 0.0, 0.0)
    t2 = (bp.cams[:, 3:] ** 2).sum(1)
    assert t2[0] == 0.0 and t2[1] > 1e-6  # the fixed cameras: one per branch
    assert t2[2] == 0.0 and 0.0 < t2[3] <= DBL_EPS < t2[4] < 2.3e-16 and t2[5] > 1e-6
    assert np.bincount(bp.cam_idx, minlength=6).min() > 0  # every camera is observed
    solve_and_compare(ctx, oracle, bp)


def test_rejected_step(ctx, oracle):
    """80 landmarks x 8 keyframes: the oracle rejects its fourth step and accepts the fifth, so the
    table of a rejected candidate (rot[1 - cur]) lies beside the current one when the next
    iteration runs, and is overwritten by the next candidate."""
    bp = S.ba_problem(S.SEED0 + 71, 80, 8, 1280, 720)
    rs = solve_and_compare(ctx, oracle, bp)
    assert rs["successful_steps"] < rs["iterations"], rs
    succ = [oracle_solve(oracle, bp, k)[2]["successful_steps"] for k in range(1, 11)]
    first_rejected = next(k for k in range(10) if succ[k] < k + 1)
    assert succ[9] > succ[first_rejected], succ  # a step is accepted after a rejected one


def test_unfused_linearisation(ctx, oracle):
    """120 landmarks x 24 keyframes: 45 tile pairs, band-sorted runs, so the plan keeps the
    linearize_kernel launch, which reads the table that other launches wrote."""
    assert geometry(ctx, 24, 2, 120)[8] == 1  # sorted: not a fused plan
    bp = S.ba_problem(S.SEED0 + 62, 120, 24, 1280, 720)
    assert len(bp.pts) == 120 and len(bp.cams) == 24
    solve_and_compare(ctx, oracle, bp)


def test_single_variable_camera(ctx, oracle):
    """50 landmarks x 3 keyframes, two of them fixed: one variable camera, a table of three entries."""
    bp = S.ba_problem(S.SEED0 + 63, 50, 3, 1280, 720)
    assert len(bp.cams) - bp.fixed_frames == 1 and len(bp.pts) == 50
    solve_and_compare(ctx, oracle, bp)


def test_two_queued_solves(ctx, oracle):
    """Two asynchronous solves of different windows queued on one context: each scratch set has
    its own tables, and both results are the oracle's."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions

    opts = SolverOptions.fixed_iterations(10)
    probs = [S.ba_problem(S.SEED0 + 64, 150, 8, 1280, 720), S.ba_problem(S.SEED0 + 65, 90, 5, 1280, 720)]
    refs = [oracle_solve(oracle, bp) for bp in probs]
    ds = [DeviceBAProblem(bp, ctx) for bp in probs]
    try:
        for d in ds:
            d.solve_async(opts)
        for d, ref in zip(ds, refs):
            s = d.wait()
            compare((*d.download(), s), ref)
    finally:
        for d in ds:
            d.close()


def test_sharded_two_contexts(ctx):
    """A 100-landmark window sharded over two contexts through the callback communicator (each
    rank builds the whole window's tables from the exchanged camera step) against the
    single-context solve."""
    from test_distributed import _two_ctx_comm_solve
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(S.SEED0 + 66, 100, 6, 1280, 720)
    assert len(bp.pts) == 100
    opts = SolverOptions.fixed_iterations(10)
    ref_c, ref_p, ref_s = ba_solve(bp.copy(), opts, ctx=ctx)
    assert ref_s["successful_steps"] >= 1
    cams, pts, summ = _two_ctx_comm_solve(bp, opts)
    for c, s in zip(cams, summ):
        compare((c, pts, s), (ref_c, ref_p, ref_s))


def test_failed_camera_solve(ctx):
    """Test hook word 1024: every camera solve fails, so no candidate and no table is built and
    every step is rejected -- the parameters come back untouched, without an error; with the
    word cleared the same context solves as before."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(S.SEED0 + 67, 40, 4, 640, 480)
    opts = SolverOptions.fixed_iterations(10)
    c0, p0, s0 = ba_solve(bp.copy(), opts, ctx=ctx)
    assert s0["successful_steps"] > 0 and not np.array_equal(c0, bp.cams)
    hook = ctx.lib.me_debug_solve_flags
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hook(ctx.h, 1024) == 0
    try:
        c1, p1, s1 = ba_solve(bp.copy(), opts, ctx=ctx)
    finally:
        assert hook(ctx.h, 0) == 0
    assert s1["successful_steps"] == 0 and np.array_equal(c1, bp.cams) and np.array_equal(p1, bp.pts)
    c2, p2, s2 = ba_solve(bp.copy(), opts, ctx=ctx)
    assert np.array_equal(c0, c2) and np.array_equal(p0, p2) and s0 == s2
