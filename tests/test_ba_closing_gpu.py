"""BA without the closing linearisation, against the CPU oracle.

With gradient_tolerance <= 0 and max_num_iterations > 0 a solve queues exactly
max_num_iterations iterations: the linearisation that used to follow the last
step (for the closing gradient test and the final cost) is not queued, the last
step's decision ends the solve at the iteration limit, and the summary's
final_cost is the candidate cost of the last accepted step.  With
gradient_tolerance > 0, or without iterations, the pass runs as before.  Each
test here is built for one way that can go wrong: a solve that ends on a
rejected or on an accepted step, the limits 0 and 1, parameters that differ
from the kept path's, launches still queued, a solve's end reaching into the
one queued behind it, a rank of a sharded solve, a solve whose every step is
invalid, and the kept path itself.  The bar against the oracle is the suite's:
equal iterations, successful steps and termination, cameras and points at rtol
1e-6 / atol 1e-9, initial and final cost at 1e-9 relative.  The windows were
chosen on the CPU, with the oracle alone."""
import ctypes

import numpy as np
import pytest

from uasl_motion_estimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

TOL_OFF = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
TINY = 1e-300  # a gradient tolerance that keeps the closing pass and cannot fire


def oracle_solve(oracle, bp, iters):
    rc, rp, rs = oracle.ba_solve(bp.copy(), max_num_iterations=iters, **TOL_OFF)
    assert np.isfinite(rc).all() and np.isfinite(rp).all() and np.isfinite(rs["final_cost"]), rs
    return rc, rp, rs


def compare(got, ref):
    (cams, pts, s), (rc, rp, rs) = got, ref
    assert (s["iterations"], s["successful_steps"], s["termination"]) == \
        (rs["iterations"], rs["successful_steps"], rs["termination"]), (s, rs)
    np.testing.assert_allclose(cams, rc, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(pts, rp, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(s["initial_cost"], rs["initial_cost"], rtol=1e-9)
    np.testing.assert_allclose(s["final_cost"], rs["final_cost"], rtol=1e-9)


def options(iters, gradient_tolerance=0.0):
    from uasl_motion_estimation_amd.optimisation import SolverOptions

    o = SolverOptions.fixed_iterations(iters)
    o.gradient_tolerance = gradient_tolerance
    return o


def geometry(ctx, nc, nf, n_pts):
    fn = ctx.lib.me_debug_ba_geometry
    fn.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    out = (ctypes.c_int * 10)()
    assert fn(nc, nf, n_pts, out) == 0
    return tuple(out)


def rejecting_window():
    """80 landmarks x 8 keyframes: the oracle rejects its fourth step and accepts the fifth."""
    return S.ba_problem(S.SEED0 + 71, 80, 8, 1280, 720)


def fused_window():
    """200 landmarks x 20 keyframes: the headline window's plan in small -- 28 tile pairs in two tile
    groups of a 32-landmark run, linearised inside the Schur pass."""
    return S.ba_problem(S.SEED0 + 81, 200, 20, 1280, 720)


def sorted_window():
    """120 landmarks x 24 keyframes: band-sorted runs, so linearize_kernel and a stand-alone assembly."""
    return S.ba_problem(S.SEED0 + 62, 120, 24, 1280, 720)


def test_last_step_rejected_and_accepted(ctx, oracle):
    """fixed_iterations(4) ends on the rejected step (the summary keeps the third step's cost and
    parameters), fixed_iterations(5) on an accepted one (the candidate cost of that step)."""
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = rejecting_window()
    refs = {k: oracle_solve(oracle, bp, k) for k in (3, 4, 5)}
    succ = {k: r[2]["successful_steps"] for k, r in refs.items()}
    assert succ == {3: 3, 4: 3, 5: 4}, succ  # the fourth step rejected, the fifth accepted
    assert refs[4][2]["final_cost"] == refs[3][2]["final_cost"] > refs[5][2]["final_cost"]
    for k in (4, 5):
        compare(ba_solve(bp.copy(), options(k), ctx=ctx), refs[k])


def test_no_iterations(ctx, oracle):
    """max_num_iterations 0: the closing pass is the only linearisation and stays -- the initial
    cost, no step, the parameters bit for bit the input."""
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = rejecting_window()
    rs = oracle_solve(oracle, bp, 0)[2]
    cams, pts, s = ba_solve(bp.copy(), options(0), ctx=ctx)
    assert np.array_equal(cams, bp.cams) and np.array_equal(pts, bp.pts)
    assert (s["iterations"], s["successful_steps"], s["termination"]) == (0, 0, rs["termination"]), (s, rs)
    assert s["initial_cost"] == s["final_cost"]
    np.testing.assert_allclose(s["initial_cost"], rs["initial_cost"], rtol=1e-9)


def test_one_iteration(ctx, oracle):
    """max_num_iterations 1: the first decision is also the solve's end."""
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = rejecting_window()
    ref = oracle_solve(oracle, bp, 1)
    assert ref[2]["iterations"] == 1 and ref[2]["successful_steps"] == 1
    compare(ba_solve(bp.copy(), options(1), ctx=ctx), ref)


def _skip_windows():
    return {
        "fused": (fused_window, 6),
        "sorted": (sorted_window, 6),
        "mono": (lambda: S.ba_problem_mono(S.SEED0 + 61, 60, 6, 1280, 720, min_len=2), 6),
        "one_camera": (lambda: S.ba_problem(S.SEED0 + 63, 50, 3, 1280, 720), 6),
        "ends_rejected": (rejecting_window, 4),
    }


@pytest.mark.parametrize("name", list(_skip_windows()))
def test_skip_changes_no_parameter(ctx, name):
    """The same window with gradient_tolerance 0 (no closing pass) and 1e-300 (the pass runs, its test
    cannot fire): the same cameras and points bit for bit, the same counts and termination, and the
    two final costs -- the step evaluation's and the linearisation's -- equal to 1e-12 relative."""
    from uasl_motion_estimation_amd.optimisation import ba_solve

    make, iters = _skip_windows()[name]
    bp = make()
    g = geometry(ctx, len(bp.cams), bp.fixed_frames, len(bp.pts))
    if name == "fused":  # one sub-chunk per run, landmark order, two tile groups in at most 128 workgroups
        assert len(bp.cams) == 20 and g[2] == 1 and g[8] == 0 and g[6] == 2 and g[7] <= 128, g
    elif name == "sorted":
        assert g[8] == 1, g
    elif name == "mono":
        assert bp.obs_dim == 2
    elif name == "one_camera":
        assert len(bp.cams) - bp.fixed_frames == 1 and len(bp.pts) == 50
    c0, p0, s0 = ba_solve(bp.copy(), options(iters), ctx=ctx)
    c1, p1, s1 = ba_solve(bp.copy(), options(iters, TINY), ctx=ctx)
    assert s0["iterations"] == iters and s0["successful_steps"] >= 1, s0
    assert not np.array_equal(c0, bp.cams)
    assert np.array_equal(c0, c1) and np.array_equal(p0, p1)
    for k in ("iterations", "successful_steps", "termination", "status"):
        assert s0[k] == s1[k], (k, s0, s1)
    assert s0["initial_cost"] == s1["initial_cost"]
    print(name, "final_cost", s0["final_cost"], s1["final_cost"],
          "rel", abs(s0["final_cost"] - s1["final_cost"]) / s1["final_cost"])
    np.testing.assert_allclose(s0["final_cost"], s1["final_cost"], rtol=1e-12)


@pytest.mark.parametrize("name", ["fused", "sorted"])
def test_launches_are_gone(ctx, name):
    """Every launch of the linearisation's families counted by the per-family timers: a
    fixed_iterations(k) solve records k Schur launches (and, unfused, k linearize launches) at
    tolerance 0 and k + 1 at 1e-300; the camera solve and the step k either way.  The queued
    asynchronous solve counts the same."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, ba_solve

    bp = fused_window() if name == "fused" else sorted_window()
    fams = ["BA_LINEARIZE", "BA_SCHUR", "BA_SOLVE", "BA_STEP"]
    k = 5

    def counts(run):
        ctx.timing_reset()
        run()
        ctx.synchronize()
        return {f: ctx.timing_read(f)[0] for f in fams}

    def queued(o):
        d = DeviceBAProblem(bp, ctx)
        try:
            d.solve_async(o)
            d.wait()
        finally:
            d.close()

    lin = 0 if name == "fused" else 1  # linearize_kernel launches per linearisation
    ctx.timing_sample(1)
    ctx.timing(True, fams)
    try:
        for run in (lambda o: ba_solve(bp.copy(), o, ctx=ctx), queued):
            got = counts(lambda: run(options(k)))
            assert got == {"BA_LINEARIZE": lin * k, "BA_SCHUR": k, "BA_SOLVE": k, "BA_STEP": k}, got
            got = counts(lambda: run(options(k, TINY)))
            assert got == {"BA_LINEARIZE": lin * (k + 1), "BA_SCHUR": k + 1, "BA_SOLVE": k, "BA_STEP": k}, got
    finally:
        ctx.timing(False)
        ctx.timing_reset()


def test_two_queued_solves(ctx, oracle):
    """Two asynchronous solves of different windows and iteration limits queued on one context: the
    first solve's end in its last decision leaves the one queued behind it alone."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem

    jobs = [(S.ba_problem(S.SEED0 + 64, 150, 8, 1280, 720), 3), (S.ba_problem(S.SEED0 + 65, 90, 5, 1280, 720), 6)]
    refs = [oracle_solve(oracle, bp, k) for bp, k in jobs]
    assert [r[2]["iterations"] for r in refs] == [3, 6] and refs[1][2]["successful_steps"] == 5
    ds = [DeviceBAProblem(bp, ctx) for bp, _ in jobs]
    try:
        for d, (_, k) in zip(ds, jobs):
            d.solve_async(options(k))
        for d, ref in zip(ds, refs):
            s = d.wait()
            compare((*d.download(), s), ref)
    finally:
        for d in ds:
            d.close()


@pytest.mark.parametrize("name,iters", [("accepted", 6), ("rejected", 4)])
def test_sharded_two_contexts(ctx, name, iters):
    """A window sharded over two contexts through the callback communicator: every rank skips the
    closing exchange alike and ends in decide_kernel, as the single-context solve ends in its step
    launch.  Ending on an accepted step (100 landmarks x 6) and on a rejected one."""
    from test_distributed import _two_ctx_comm_solve
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = S.ba_problem(S.SEED0 + 66, 100, 6, 1280, 720) if name == "accepted" else rejecting_window()
    ref = ba_solve(bp.copy(), options(iters), ctx=ctx)
    assert ref[2]["iterations"] == iters
    assert (ref[2]["successful_steps"] == iters) == (name == "accepted"), ref[2]
    cams, pts, summ = _two_ctx_comm_solve(bp, options(iters))
    for c, s in zip(cams, summ):
        compare((c, pts, s), ref)


def test_every_step_invalid(ctx):
    """Test hook word 1024 (every camera solve fails) with fixed_iterations(3): the iteration limit
    is reached before max_num_consecutive_invalid_steps, the solve ends at the limit without an
    error and the parameters come back untouched -- as with the closing pass kept."""
    from uasl_motion_estimation_amd.optimisation import ba_solve

    bp = S.ba_problem(S.SEED0 + 67, 40, 4, 640, 480)
    assert options(3).max_num_consecutive_invalid_steps > 3
    hook = ctx.lib.me_debug_solve_flags
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hook(ctx.h, 1024) == 0
    try:
        c0, p0, s0 = ba_solve(bp.copy(), options(3), ctx=ctx)
        c1, p1, s1 = ba_solve(bp.copy(), options(3, TINY), ctx=ctx)
    finally:
        assert hook(ctx.h, 0) == 0
    for c, p, s in ((c0, p0, s0), (c1, p1, s1)):
        assert np.array_equal(c, bp.cams) and np.array_equal(p, bp.pts)
        assert (s["iterations"], s["successful_steps"], s["termination"]) == (3, 0, 1), s
        assert s["final_cost"] == s["initial_cost"]
    assert s0 == s1


def test_default_options(ctx, oracle):
    """Tolerances on (the kept path): the solve converges by function tolerance as the oracle does."""
    from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

    bp = S.ba_problem(S.SEED0 + 64, 150, 8, 1280, 720)
    rc, rp, rs = oracle.ba_solve(bp.copy())
    assert rs["termination"] == 0 and 1 <= rs["successful_steps"] < rs["iterations"] < 50, rs
    compare(ba_solve(bp.copy(), SolverOptions(), ctx=ctx), (rc, rp, rs))
