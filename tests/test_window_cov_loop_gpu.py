"""The VO loops' covariance switch (PipelineConfig(covariance=WindowCovariance()),
me_vo_loop_set_covariance): NativeStereoVO, the GPU-backed WindowedStereoVO and
the loop on the oracle backend (window_cov_ref on numpy Jacobians) agree at the
covariance bar (window_cov_cases.py) for pose_cov(t) at every t and for
track_cov(); the switch is read only (events, poses and FrameResults bit for
bit with it on and off); off, the loops queue no covariance; a failed solve
leaves ok = 0 and the loop goes on.  Config 1 (640 x 480, 200 features), W = 5,
10 keyframes: the window fills and slides, tracks are deleted."""
import dataclasses

import numpy as np
import pytest

import window_cov_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.ba_cov import WindowCovariance

pytestmark = pytest.mark.gpu

N, W, ITERS = 10, 5, 5


def config(cov):
    cfg = PL.PipelineConfig.from_config(1, ba_iters=ITERS)
    cfg.window = W
    cfg.covariance = cov
    return cfg


@pytest.fixture(scope="module")
def seq():
    return PL.synthetic_sequence(1, N)


def snapshot(vo):
    """What the tests compare, taken before the loop is closed."""
    return dict(events=list(vo.events), poses={t: np.array(p) for t, p in vo.poses.items()},
                results=[dataclasses.astuple(r) for r in vo.results], ids=np.array(vo.ids),
                pose_cov={t: vo.pose_cov(t) for t in range(N)}, pose_ok=vo.pose_cov_ok(), track_cov=vo.track_cov())


def drive(vo, seq):
    fr = seq[0]
    for t in range(N):
        vo.process(t, fr[t].left, fr[t].right)
    vo.finish()
    return snapshot(vo)


def run_native(ctx, seq, cov, **kw):
    _, K, p0, v, _ = seq
    vo = PL.NativeStereoVO(config(cov), ctx, K, p0, v, log_events=True, **kw)
    try:
        return drive(vo, seq)
    finally:
        vo.close()


def run_python(ctx, seq, cov):
    _, K, p0, v, _ = seq
    be = PL.GPUBackend(ctx)
    try:
        return drive(PL.WindowedStereoVO(config(cov), be, K, p0, v, log_events=True, overlap=True), seq)
    finally:
        be.close()


@pytest.fixture(scope="module")
def runs(ctx, oracle, seq):
    from pipeline_oracle import OracleBackend

    _, K, p0, v, _ = seq
    on = WindowCovariance()
    return dict(native_on=run_native(ctx, seq, on), native_off=run_native(ctx, seq, None),
                python_on=run_python(ctx, seq, on), python_off=run_python(ctx, seq, None),
                ref_on=drive(PL.WindowedStereoVO(config(on), OracleBackend(), K, p0, v, log_events=True), seq))


def same_tuple(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) if isinstance(x, (np.ndarray, float))
                                    else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("loop", ["native", "python"])
def test_switch_is_read_only(runs, loop):
    on, off = runs[loop + "_on"], runs[loop + "_off"]
    assert on["events"] == off["events"] and np.array_equal(on["ids"], off["ids"])
    assert on["poses"].keys() == off["poses"].keys()
    assert all(np.array_equal(on["poses"][t], off["poses"][t]) for t in on["poses"])
    assert len(on["results"]) == len(off["results"]) == N
    assert all(same_tuple(a, b) for a, b in zip(on["results"], off["results"]))
    # off: nothing to read
    assert off["pose_ok"] == {} and off["track_cov"] == {} and all(v is None for v in off["pose_cov"].values())


def test_three_loops_agree_at_the_bar(runs):
    nat, py, ref = runs["native_on"], runs["python_on"], runs["ref_on"]
    fixed = config(None).fixed_frames
    have = list(range(fixed, N))  # a keyframe has a window of its own once the window holds a variable camera
    for r in (nat, py, ref):
        assert sorted(r["pose_ok"]) == have and all(r["pose_ok"].values())
        assert all(r["pose_cov"][t] is None for t in range(fixed))
    for t in have:
        want = ref["pose_cov"][t]
        assert np.all(np.linalg.eigvalsh(want) > 0)
        for got in (nat["pose_cov"][t], py["pose_cov"][t]):
            C.assert_cam_blocks(got, want)
    assert np.array_equal(nat["ids"], ref["ids"])
    live = set(int(i) for i in ref["ids"])
    assert set(ref["track_cov"]) == set(nat["track_cov"]) == set(py["track_cov"]) and set(ref["track_cov"]) <= live
    assert len(ref["track_cov"]) > 50
    ids = sorted(ref["track_cov"])
    want = np.stack([ref["track_cov"][i] for i in ids])
    for r in (nat, py):
        C.assert_pt_blocks(np.stack([r["track_cov"][i] for i in ids]), want)
    # (the two device loops are not compared bit for bit: their poses agree to the loops' 1e-6 bar, not to the bit)


def test_cameras_only(ctx, seq, runs):
    r = run_native(ctx, seq, WindowCovariance(landmarks=False))
    assert r["track_cov"] == {} and r["events"] == runs["native_off"]["events"]
    assert all(np.array_equal(r["pose_cov"][t], runs["native_on"]["pose_cov"][t]) for t in range(2, N))


def test_switch_off_queues_no_covariance(ctx, seq, runs):
    """Off, the loops launch what they launched: the window covariance adds one
    linearisation (one BA_SCHUR launch) per window, and only with the switch
    on; the Python loop never calls the covariance wait."""
    from uasl_motion_estimation_amd._lib import Context

    n_windows = N - config(None).fixed_frames
    counts = {}
    for name, cov in (("off", None), ("on", WindowCovariance())):
        c = Context(ctx.device)
        try:
            c.timing(True, ["BA_SCHUR"])
            c.timing_sample(1)
            c.timing_reset()
            run_native(c, seq, cov, overlap=False)
            c.synchronize()
            counts[name] = c.timing_read("BA_SCHUR")[0]
        finally:
            c.timing(False)
            c.close()
    assert counts["off"] > 0 and counts["off"] % n_windows == 0 and counts["on"] == counts["off"] + n_windows, counts
    be = PL.GPUBackend(ctx)
    called = []
    plain = be.ctx.lib.me_ba_wait_out_cov
    try:
        be.ctx.lib.me_ba_wait_out_cov = lambda *a: called.append(1) or plain(*a)
        _, K, p0, v, _ = seq
        r = drive(PL.WindowedStereoVO(config(None), be, K, p0, v, log_events=True, overlap=True), seq)
    finally:
        be.ctx.lib.me_ba_wait_out_cov = plain
        be.close()
    assert not called and r["events"] == runs["python_off"]["events"]


def test_failed_solves_leave_ok_zero_and_the_loop_goes_on(ctx, seq):
    """Every second window's solve fails (the test hook of tests/test_pipeline.py):
    its keyframe and landmarks read ok = 0, the other windows are served, and the
    loop's events are those of the same run without the switch."""
    res = {}
    for name, cov in (("off", None), ("on", WindowCovariance())):
        assert ctx.lib.me_debug_solve_flags(ctx.h, 2048) == 0
        try:
            res[name] = run_native(ctx, seq, cov)
        finally:
            ctx.lib.me_debug_solve_flags(ctx.h, 0)
    on, off = res["on"], res["off"]
    assert on["events"] == off["events"] and len(on["results"]) == N
    assert all(np.array_equal(on["poses"][t], off["poses"][t]) for t in on["poses"])
    ok = on["pose_ok"]
    assert sorted(ok) == list(range(2, N)) and any(ok.values()) and not all(ok.values())
    for t, good in ok.items():
        assert (on["pose_cov"][t] is not None) == good
    assert set(on["track_cov"]) <= set(int(i) for i in on["ids"])
