"""The per-landmark residual check on the device (me_ba_point_check,
csrc/ba_check.hip) and the VO loops' switch for it.

chi2 is compared bit for bit with the max-reduce, in numpy, of the device's own
me_ba_evaluate residuals; against the oracle's residuals at the bound that
follows from the project's residual bar (track_check_cases.chi2_bound); the
flags with the restatement on the oracle's residuals for every landmark
outside the band of 1e-6 chi2_max around chi2_max, and no landmark of the test
shapes may lie inside it.  Figures at the device's 5-iteration solutions
(MI355X): see each test's output before its assertions."""
import ctypes

import numpy as np
import pytest

import motion_gate_cases as MG
import track_check_cases as C
import window_cov_cases as WC
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd import synthetic as S
from uasl_motion_estimation_amd._lib import BASummaryC
from uasl_motion_estimation_amd.track_check import FLAG_BEHIND, FLAG_CHI2, TrackCheck, depths, point_check_ref

pytestmark = pytest.mark.gpu

D = TrackCheck()
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def solved(ctx, name):
    """The shape after 5 fixed LM iterations on the device (computed once, read only)."""
    if name not in _cache:
        from uasl_motion_estimation_amd.optimisation import SolverOptions, ba_solve

        bp = C.PROBLEMS[name]()
        bp.cams, bp.pts, summ = ba_solve(bp, SolverOptions.fixed_iterations(5), ctx=ctx)
        assert summ["termination"] != 2
        for a in (bp.cams, bp.pts):
            a.setflags(write=False)
        _cache[name] = bp
    return _cache[name]


def device_ref(ctx, bp, params=D):
    """The rule in numpy on the device's own residuals (me_ba_evaluate) of bp."""
    from uasl_motion_estimation_amd.optimisation import ba_evaluate

    with np.errstate(all="ignore"):
        r = ba_evaluate(bp, ctx=ctx)[0]
        return point_check_ref(r, depths(bp), bp.pt_idx, len(bp.pts), params)


def assert_is_device_ref(ctx, bp, params=D):
    from uasl_motion_estimation_amd.optimisation import ba_point_check

    chi2, flags, n = ba_point_check(bp, params, ctx=ctx)
    rchi2, rflags = device_ref(ctx, bp, params)
    assert np.array_equal(bits(chi2), bits(rchi2))
    assert np.array_equal(flags, rflags) and n == np.count_nonzero(rflags)
    return chi2, flags


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("name", list(C.PROBLEMS))
def test_shapes_three_comparisons(ctx, oracle, name):
    from uasl_motion_estimation_amd.optimisation import ba_point_check

    bp = solved(ctx, name)
    cnt = np.bincount(bp.pt_idx, minlength=len(bp.pts))
    if name == "mono_long_50":
        assert cnt.max() > 64 and getattr(bp, "obs_dim", 4) == 2 and len(bp.cams) == 50  # longer than a wavefront
    chi2, flags, n = ba_point_check(bp, ctx=ctx)
    # 1. bit for bit the max-reduce of the device's own residuals
    rchi2, rflags = device_ref(ctx, bp)
    assert np.array_equal(bits(chi2), bits(rchi2)) and np.array_equal(flags, rflags)
    assert n == np.count_nonzero(flags) and 0 < n < len(flags)
    # 2. against the oracle's residuals at the same parameters
    ochi2, oflags = C.oracle_check(oracle, bp)
    err = np.abs(chi2 - ochi2)
    bound = C.chi2_bound(ochi2)
    k = int(np.argmax(err - bound))
    closest = float(np.abs(ochi2 - D.chi2_max).min() / D.chi2_max)
    print(f"{name}: n_pts {len(flags)} longest track {cnt.max()} flagged {n} | worst |dchi2| {err[k]:.3e} at chi2 "
          f"{ochi2[k]:.3e} (bound {bound[k]:.3e}) | closest landmark to chi2_max: {closest:.3e} relative")
    assert np.all(err <= bound)
    # 3. no landmark inside the band, and the flags equal the restatement's on the oracle's residuals
    assert not C.in_band(ochi2, D).any()
    assert np.array_equal(flags, oflags)


@pytest.mark.parametrize("name", ["stereo_200x8", "mono_200x8", "mono_long_50"])
def test_host_and_device_forms_identical_repeatable_and_order_free(ctx, name):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, ba_point_check

    bp = solved(ctx, name)
    chi2, flags, n = ba_point_check(bp, ctx=ctx)
    again = ba_point_check(bp, ctx=ctx)
    assert np.array_equal(bits(again[0]), bits(chi2)) and np.array_equal(again[1], flags) and again[2] == n
    for seed in (1, 2):  # another order of the observation arrays: the same bits
        sh = ba_point_check(C.shuffled(bp, seed), ctx=ctx)
        assert np.array_equal(bits(sh[0]), bits(chi2)) and np.array_equal(sh[1], flags)
    for prob in (bp, C.shuffled(bp, 3)):
        dev = DeviceBAProblem(prob, ctx)
        try:
            for k in range(2):
                if k:  # (the outputs exist now: every entry is written again over a fill)
                    ctx.h2d(dev.d["check_chi2"], np.full(max(dev.n_pts, 1), -7.0))
                    ctx.h2d(dev.d["check_flags"], np.full(max(dev.n_pts, 16), 0x7f, np.uint8))
                dev.point_check_async()
                dchi2, dflags = dev.point_check_read()
                assert np.array_equal(bits(dchi2), bits(chi2)) and np.array_equal(dflags, flags)
        finally:
            dev.close()
    # other parameters: the same chi2, the flags by the rule
    other = TrackCheck(chi2_max=200.0, z_min=20.0)
    c2, f2, _ = ba_point_check(bp, other, ctx=ctx)
    assert np.array_equal(bits(c2), bits(chi2))
    assert np.array_equal(f2, device_ref(ctx, bp, other)[1]) and np.any(f2 & FLAG_BEHIND) and not np.all(f2 & FLAG_BEHIND)


def test_null_chi2_and_parameter_validation(ctx):
    from uasl_motion_estimation_amd.optimisation import ba_point_check, ba_struct

    bp = solved(ctx, "stereo_60x5")
    _, flags, _ = ba_point_check(bp, ctx=ctx)
    keep = []
    p, _, _ = ba_struct(bp, keep)
    got = np.full(len(bp.pts), 0x7f, np.uint8)
    assert ctx.lib.me_ba_point_check(ctx.h, ctypes.byref(p), None, None, got.ctypes.data, None) == 0  # NULL: defaults
    assert np.array_equal(got, flags)
    for chi2_max, z_min in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (18.47, -1.0), (18.47, float("inf")),
                            (18.47, float("nan"))):
        prm = D.to_c()
        prm.chi2_max, prm.z_min = chi2_max, z_min
        got[:] = 0x7f
        assert ctx.lib.me_ba_point_check(ctx.h, ctypes.byref(p), ctypes.byref(prm), None, got.ctypes.data, None) == -1
        assert np.all(got == 0x7f)
    assert b"me_ba_point_check" in ctx.lib.me_last_error(ctx.h)
    assert ctx.lib.me_ba_point_check(ctx.h, ctypes.byref(p), None, None, None, None) == -1  # flags is required
    dflt = D.to_c()
    dflt.chi2_max = dflt.z_min = -1.0
    ctx.lib.me_ba_point_check_default_params(ctypes.byref(dflt))
    assert (dflt.chi2_max, dflt.z_min) == (18.47, 0.0)


# ------------------------------------------------------------------ edges
def first_landmarks(bp, n):
    """bp cut to its first n landmarks and their observations."""
    out = WC.keep_obs(bp, bp.pt_idx < n)
    out.pts = bp.pts[:n].copy()
    return out


@pytest.mark.parametrize("n_obs", [255, 256, 257])
def test_observation_counts_around_the_workgroup_size(ctx, n_obs):
    bp = solved(ctx, "stereo_200x8")
    keep = np.zeros(len(bp.obs), bool)
    keep[np.random.default_rng(5).permutation(len(bp.obs))[:n_obs]] = True
    cut = WC.keep_obs(bp, keep)
    assert len(cut.obs) == n_obs
    chi2, _ = assert_is_device_ref(ctx, cut)
    assert np.count_nonzero(np.bincount(cut.pt_idx, minlength=len(cut.pts)) == 0) > 0  # some landmark lost every one
    assert np.all(chi2[np.bincount(cut.pt_idx, minlength=len(cut.pts)) == 0] == 0.0)


@pytest.mark.parametrize("n_pts", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_landmark_counts_around_a_wavefront_and_a_workgroup(ctx, n_pts):
    """8 lanes per landmark: a wavefront holds 8 landmarks, a workgroup 32; 64 and 256 are the thread counts."""
    bp = S.ba_problem(48, 300, 8, 640, 480)
    assert len(bp.pts) >= 257
    assert_is_device_ref(ctx, first_landmarks(bp, n_pts))


def test_landmark_without_observations_and_duplicated_pair(ctx):
    bp = solved(ctx, "stereo_60x5").copy()
    bp.pts = np.vstack([bp.pts, [[0.5, 0.2, 10.0]]])
    chi2, flags = assert_is_device_ref(ctx, bp)
    assert chi2[-1] == 0.0 and flags[-1] == 0
    # the same (point, camera) pair twice, the copy with another measurement: both count
    o = 7
    dup = bp.copy()
    dup.obs = np.vstack([bp.obs, bp.obs[o] + [9.0, 0.0, 0.0, 0.0]])
    dup.cam_idx = np.append(bp.cam_idx, bp.cam_idx[o]).astype(np.int32)
    dup.pt_idx = np.append(bp.pt_idx, bp.pt_idx[o]).astype(np.int32)
    c2, f2 = assert_is_device_ref(ctx, dup)
    i = int(bp.pt_idx[o])
    assert c2[i] > chi2[i] and c2[i] > (9.0 / 0.5) ** 2 * 0.5 and f2[i] & FLAG_CHI2
    assert np.array_equal(np.delete(bits(c2), i), np.delete(bits(chi2), i))


@pytest.mark.parametrize("name", ["stereo_60x5", "mono_200x8"])
def test_landmark_behind_a_camera_and_nan_landmark(ctx, name):
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem

    base = solved(ctx, name)
    _, f0 = assert_is_device_ref(ctx, base)
    assert not (f0 & FLAG_BEHIND).any()
    i = int(base.pt_idx[0])
    cam = base.cams[base.cam_idx[0]]
    behind = base.copy()
    behind.pts = base.pts.copy()
    behind.pts[i] = PL.aa_to_R(cam[3:]).T @ (np.array([0.1, 0.1, -2.0]) - cam[:3])
    _, f = assert_is_device_ref(ctx, behind)
    assert f[i] & FLAG_BEHIND and not (np.delete(f, i) & FLAG_BEHIND).any()
    nan = base.copy()
    nan.pts = base.pts.copy()
    nan.pts[i, 2] = np.nan
    c, f = assert_is_device_ref(ctx, nan)
    assert c[i] == np.inf and f[i] == (FLAG_CHI2 | FLAG_BEHIND)
    assert np.array_equal(np.delete(f, i), np.delete(f0, i))
    dev = DeviceBAProblem(nan, ctx)
    try:
        dev.point_check_async()
        dc, df = dev.point_check_read()
        assert np.array_equal(bits(dc), bits(c)) and np.array_equal(df, f)
    finally:
        dev.close()


def test_check_after_reserve(ctx):
    """me_ba_reserve sizes the check's buffers too; a window inside the reserved sizes gives the same bits."""
    from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, ba_point_check

    bp = solved(ctx, "stereo_60x5")
    chi2, flags, _ = ba_point_check(bp, ctx=ctx)
    ctx.check(ctx.lib.me_ba_reserve(ctx.h, 30, 400, 4000, 4, 2), "me_ba_reserve")
    dev = DeviceBAProblem(bp, ctx)
    try:
        dev.point_check_async()
        dc, df = dev.point_check_read()
    finally:
        dev.close()
    assert np.array_equal(bits(dc), bits(chi2)) and np.array_equal(df, flags)
    again = ba_point_check(bp, ctx=ctx)
    assert np.array_equal(bits(again[0]), bits(chi2)) and np.array_equal(again[1], flags)


# ------------------------------------------------------------------ queued behind a window solve
def submitted_pair(ctx, bufs, check, cov, iters=None):
    """test_vo_glue_gpu's pair of windows through me_vo_window_submit, each with `check` (a C struct or None) and
    `cov`; iters: LM iterations instead of that test's."""
    import test_vo_glue_gpu as G

    class Pair(G.SubmittedPair):
        def _prepare(self, w, chain, staged):
            super()._prepare(w, chain, staged)
            win = self.keep[-1][0]
            win.cov = cov
            if iters is not None:
                self.opt.max_num_iterations = iters
            win.check = ctypes.addressof(check) if check is not None else None

        def wait_check(self, k, with_cov):
            st = self.sets[k]
            c, p = np.zeros((st["nc"], 6)), np.zeros((st["npts"], 3))
            ccov, pcov = np.zeros((st["nc"], 6, 6)), np.zeros((st["npts"], 3, 3))
            cok = ctypes.c_int(-1 if with_cov else 0)  # (not passed without the covariance: stays 0)
            flags = np.full(st["npts"] + 8, 0x7f, np.uint8)
            fok = ctypes.c_int(-1)
            s = BASummaryC()
            self.ctx.check(self.ctx.lib.me_ba_wait_out_check(
                self.ctx.h, ctypes.byref(s), c.ctypes.data, p.ctypes.data, ccov.ctypes.data if with_cov else None,
                pcov.ctypes.data if with_cov else None, ctypes.addressof(cok) if with_cov else None, flags.ctypes.data,
                ctypes.addressof(fok)), "me_ba_wait_out_check")
            self.queued -= 1
            assert np.all(flags[st["npts"]:] == 0x7f)
            return c, p, s.termination, cok.value, flags[:st["npts"]], fok.value

    return Pair(ctx, bufs)


@pytest.fixture
def bufs(ctx):
    import test_vo_glue_gpu as G

    b = G.Bufs(ctx)
    yield b
    b.close()


@pytest.mark.parametrize("cov", [0, 2], ids=["check-alone", "behind-the-covariance"])
def test_flags_queued_behind_a_window_solve(ctx, bufs, cov):
    from uasl_motion_estimation_amd.optimisation import ba_point_check

    prm = D.to_c()
    sp = submitted_pair(ctx, bufs, prm, cov)
    try:
        res = [sp.wait_check(k, cov != 0) for k in (0, 1)]
    finally:
        sp.close()
    for w, (c, p, term, cok, flags, fok) in zip((sp.wp.w1, sp.wp.w2), res):
        assert term != 2 and fok == 1 and cok == cov
        want = ba_point_check(sp.wp.problem(w, c, p), ctx=ctx)[1]  # the stand-alone check at the cams / pts read back
        assert np.array_equal(flags, want) and 0 < np.count_nonzero(flags) < len(flags)


def test_check_ok_zero_when_none_was_queued_and_after_a_failed_solve(ctx, bufs):
    sp = submitted_pair(ctx, bufs, None, 0)
    try:
        res = [sp.wait_check(k, False) for k in (0, 1)]
    finally:
        sp.close()
    for c, p, term, _, flags, fok in res:
        assert term != 2 and fok == 0 and np.all(flags == 0x7f)
    prm = D.to_c()
    assert ctx.lib.me_debug_solve_flags(ctx.h, 1024) == 0  # every camera solve fails: termination 2
    try:
        sp = submitted_pair(ctx, bufs, prm, 0, iters=8)  # (5 consecutive invalid steps end a solve in FAILURE)
        try:
            res = [sp.wait_check(k, False) for k in (0, 1)]
        finally:
            sp.close()
    finally:
        ctx.lib.me_debug_solve_flags(ctx.h, 0)
    for c, p, term, _, flags, fok in res:
        assert term == 2 and fok == 0 and np.all(flags == 0x7f)
    # bad parameters are refused at the submit, nothing is queued
    import test_vo_glue_gpu as G

    bad = D.to_c()
    bad.chi2_max = float("nan")
    with pytest.raises(Exception, match="check"):
        submitted_pair(ctx, bufs, bad, 0)
    assert ctx.lib.me_ba_wait(ctx.h, None) == G.ME_ERR_STATE


# ------------------------------------------------------------------ the loops
def assert_band_in_every_window(be):
    for t, _, chi2, _ in be.check_log:
        assert not C.in_band(chi2, D).any(), t


def check_loop(g, o):
    from test_pipeline import _check_against_oracle  # the bar the loops are already held to (events exact, 1e-6)

    assert [r.n_tracked for r in g.results] == [r.n_tracked for r in o.results]
    assert [r.n_active for r in g.results] == [r.n_active for r in o.results]
    _check_against_oracle(g, o, 4, MG.N_KEYFRAMES)


def test_python_gpu_loop_matches_the_oracle_loop(ctx, oracle):
    o, obe = C.oracle_loop(D)
    assert_band_in_every_window(obe)
    _, K, p0, v = MG.stream()
    be = PL.GPUBackend(ctx)
    try:
        g = MG.run_loop(PL.WindowedStereoVO(MG.loop_config(track_check=D), be, K, p0, v, log_events=True, overlap=True))
    finally:
        be.close()
    assert g.flagged() == o.flagged() and len(g.flagged()) > 0
    assert be.check_log is None  # (the device ran the check: nothing was restated on the host)
    check_loop(g, o)


@pytest.mark.parametrize("overlap", [True, False], ids=["two-contexts", "one-context"])
def test_native_loop_matches_the_oracle_loop(ctx, oracle, overlap):
    o, obe = C.oracle_loop(D)
    assert_band_in_every_window(obe)
    _, K, p0, v = MG.stream()
    g = PL.NativeStereoVO(MG.loop_config(track_check=D), ctx, K, p0, v, log_events=True, overlap=overlap)
    try:
        MG.run_loop(g)
        assert g.flagged() == o.flagged()
        check_loop(g, o)
    finally:
        g.close()


def test_launch_counts_and_the_switch_left_off(ctx, oracle):
    """Off: no ME_KT_BA_CHECK launch and the events recorded before the switch
    existed (tests/golden); on: one launch per window solved."""
    import os

    from uasl_motion_estimation_amd._lib import Context

    want = open(os.path.join(os.path.dirname(__file__), "golden", "motion_gate_off_events.sha256")).read().split()[0]
    _, K, p0, v = MG.stream()
    n_windows = MG.N_KEYFRAMES - MG.loop_config().fixed_frames
    counts, digests = {}, {}
    for name, chk in (("off", None), ("on", D)):
        c = Context(ctx.device)
        try:
            c.timing(True, ["BA_CHECK"])
            c.timing_sample(1)
            c.timing_reset()
            g = PL.NativeStereoVO(MG.loop_config(track_check=chk), c, K, p0, v, log_events=True, overlap=False)
            try:
                MG.run_loop(g)
                digests[name] = MG.events_digest(g.events)
                n_flagged = len(g.flagged())
            finally:
                g.close()
            c.synchronize()
            counts[name] = c.timing_read("BA_CHECK")[0]
        finally:
            c.timing(False)
            c.close()
        assert (n_flagged > 0) == (name == "on")
    assert counts == {"off": 0, "on": n_windows}, counts
    assert digests["off"] == want and digests["on"] != want


def test_native_setter_rules(ctx):
    fr, K, p0, v = MG.stream()
    g = PL.NativeStereoVO(MG.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        pc = D.to_c()
        assert g.lib.me_vo_loop_set_track_check(g.h, ctypes.byref(pc)) == 0  # before the first keyframe: any number
        assert g.lib.me_vo_loop_set_track_check(g.h, None) == 0              # of times, NULL switches it off
        bad = D.to_c()
        bad.z_min = float("nan")
        assert g.lib.me_vo_loop_set_track_check(g.h, ctypes.byref(bad)) == -1
        assert b"z_min" in g.lib.me_vo_loop_last_error(g.h)
        g.process(0, fr[0].left, fr[0].right)
        assert g.lib.me_vo_loop_set_track_check(g.h, ctypes.byref(pc)) == -5  # ME_ERR_STATE
        assert b"residual check" in g.lib.me_vo_loop_last_error(g.h)
        g.finish()
        assert g.flagged() == []
    finally:
        g.close()
