"""Window covariance, CPU side: window_cov_ref (the numpy Schur form the device
computation is checked against, uasl_motion_estimation_amd/ba_cov.py) against
the dense inverse of J^T J and against the oracle's camera blocks
(extract_covariance, BundleAdjuster.h:478-528).  The landmark blocks are the
ones the reference declares and leaves empty (BundleAdjuster.h:277,498-523).
Bar: window_cov_cases.py."""
import numpy as np
import pytest

import window_cov_cases as C
from uasl_motion_estimation_amd import synthetic as S
from uasl_motion_estimation_amd.ba_cov import huber_row_scale, window_cov_ref


@pytest.fixture(scope="module", params=list(C.PROBLEMS))
def case(request, oracle):
    bp = C.PROBLEMS[request.param]()
    return bp, C.ref_covariance(oracle, bp)


def test_ref_matches_dense_inverse(oracle, case):
    """Every camera and every landmark block, none left out."""
    bp, ref = case
    assert ref is not None
    cam, pt = ref
    dcam, dpt = C.dense_covariance(oracle, bp)
    assert cam.shape == (len(bp.cams), 6, 6) and pt.shape == (len(bp.pts), 3, 3)
    assert not cam[:bp.fixed_frames].any()
    C.assert_cam_blocks(cam, dcam)
    C.assert_pt_blocks(pt, dpt)


def test_ref_camera_blocks_match_oracle(oracle, case):
    bp, ref = case
    ocov = oracle.ba_covariance(bp)
    assert ocov is not None and ref is not None
    C.assert_cam_blocks(ref[0], ocov)


def test_outliers_exercise_the_loss_correction(oracle):
    r, _, _ = oracle.ba_evaluate(C.PROBLEMS["stereo_200x8"]())
    sc = huber_row_scale(r)
    assert 0.5 < np.mean(sc < 1.0) < 0.95 and np.all(sc > 0.0) and np.all(sc <= 1.0)


def test_fixed_camera_only_landmark_is_inverse_of_V(oracle):
    bp = C.fixed_only_landmark(S.ba_problem(48, 200, 8, 640, 480))
    mine = np.nonzero(bp.pt_idx == 0)[0]
    assert len(mine) == 1 and bp.cam_idx[mine[0]] < bp.fixed_frames
    r, Jc, Jp = oracle.ba_evaluate(bp)
    cam, pt = window_cov_ref(r, Jc, Jp, bp.cam_idx, bp.pt_idx, len(bp.cams), len(bp.pts), bp.fixed_frames)
    J = huber_row_scale(r)[mine[0]] * Jp[mine[0]]
    Vinv = np.linalg.inv(J.T @ J)
    np.testing.assert_allclose(pt[0], Vinv, rtol=1e-12, atol=1e-12 * np.abs(Vinv).max())
    # and the other blocks still are the dense inverse's
    dcam, dpt = C.dense_covariance(oracle, bp)
    C.assert_cam_blocks(cam, dcam)
    C.assert_pt_blocks(pt, dpt)


def test_landmark_without_observations_gives_none(oracle):
    bp = S.ba_problem(50, 40, 4, 640, 480)
    bp.pts = np.vstack([bp.pts, [[0.5, 0.2, 10.0]]])
    assert oracle.ba_covariance(bp) is None
    assert C.ref_covariance(oracle, bp) is None


def test_variable_camera_without_observations_gives_none(oracle):
    bp = S.ba_problem(44, 30, 4, 640, 480)
    bp = C.keep_obs(bp, bp.cam_idx != 3)
    assert oracle.ba_covariance(bp) is None
    assert C.ref_covariance(oracle, bp) is None


def test_all_cameras_fixed_gives_inverse_of_V(oracle):
    bp = S.ba_problem(42, 60, 5, 640, 480, fixed=5)
    cam, pt = C.ref_covariance(oracle, bp)
    assert not cam.any()
    _, dpt = C.dense_covariance(oracle, bp)
    C.assert_pt_blocks(pt, dpt)



def test_loop_on_a_host_backend_reports_covariances_and_changes_nothing(oracle):
    """WindowedStereoVO on the oracle backend with PipelineConfig(covariance=...): window_cov_ref on the numpy
    Jacobians of every window at its solved cams / pts; the loop's events, poses and landmarks are those without
    the switch."""
    from pipeline_oracle import OracleBackend

    from uasl_motion_estimation_amd import pipeline as PL
    from uasl_motion_estimation_amd.ba_cov import WindowCovariance, stereo_jacobians

    bp = S.ba_problem(42, 60, 5, 640, 480)
    for a, b in zip(stereo_jacobians(bp), oracle.ba_evaluate(bp)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * np.abs(b).max())
    n, frames = 7, PL.synthetic_sequence(1, 7)
    fr, K, p0, v, _ = frames
    vos = []
    for cov in (None, WindowCovariance()):
        cfg = PL.PipelineConfig.from_config(1, ba_iters=2)
        cfg.window, cfg.covariance = 4, cov
        vo = PL.WindowedStereoVO(cfg, OracleBackend(), K, p0, v, log_events=True)
        for t in range(n):
            vo.process(t, fr[t].left, fr[t].right)
        vo.finish()
        vos.append(vo)
    off, on = vos
    assert on.events == off.events and np.array_equal(on.X, off.X)
    assert all(np.array_equal(on.poses[t], off.poses[t]) for t in off.poses)
    assert off.pose_cov(n - 1) is None and off.track_cov() == {}
    assert sorted(on.pose_cov_ok()) == list(range(2, n)) and all(on.pose_cov_ok().values())
    assert on.pose_cov(0) is None and on.pose_cov(1) is None
    # the last window, rebuilt on the host at the loop's final state, gives the last keyframe's block
    f0 = n - 4
    upts = np.flatnonzero(on.last >= f0)
    last = on.ba_problem(n - 1, f0, upts)
    cam, pt = C.dense_covariance(oracle, last)
    C.assert_cam_blocks(on.pose_cov(n - 1), cam[-1])
    tc = on.track_cov()
    assert set(tc) <= set(int(i) for i in on.ids) and set(int(i) for i in on.ids[upts]) <= set(tc)
    C.assert_pt_blocks(np.stack([tc[int(i)] for i in on.ids[upts]]), pt)
    with pytest.raises(ValueError, match="covariance"):
        PL.PipelineConfig.from_config(1, covariance=True)
