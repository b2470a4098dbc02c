"""Shared by test_window_cov.py (CPU) and test_window_cov_gpu.py: the window
problems, the dense (J^T J)^-1 the Schur form is checked against, and the
project's covariance bar (tests/test_ba_mono_cov.py): rtol 1e-6, atol 1e-9 x
max|ref| -- over the whole array for the camera blocks, per block for the
landmark blocks, whose magnitudes span orders."""
import numpy as np

from uasl_motion_estimation_amd import synthetic as S

RTOL, ATOL = 1e-6, 1e-9

# name -> builder: the four windows whose Schur form was compared with the
# dense inverse when the bar was set (condition numbers up to 1.9e14; 75-85 %
# of the observations Huber outliers before a solve)
PROBLEMS = {
    "stereo_200x8": lambda: S.ba_problem(48, 200, 8, 640, 480),
    "stereo_60x5": lambda: S.ba_problem(42, 60, 5, 640, 480),
    "mono_200x8": lambda: S.ba_problem_mono(49, 200, 8, 640, 480),
    "stereo_33x3": lambda: S.ba_problem(51, 33, 3, 640, 480),
}


def n_fixed(bp):
    return min(max(bp.fixed_frames, 0), len(bp.cams))


def dense_covariance(oracle, bp):
    """(cam_cov, pt_cov) as the blocks of inv(J^T J), J the Huber-corrected
    Jacobian of the variable cameras and all landmarks, built densely from the
    oracle's residuals and Jacobians."""
    r, Jc, Jp = oracle.ba_evaluate(bp)
    nf = n_fixed(bp)
    m, npt, D = len(bp.cams) - nf, len(bp.pts), r.shape[1]
    J = np.zeros((r.size, 6 * m + 3 * npt))
    for o in range(len(r)):
        s = float(r[o] @ r[o])
        sc = np.sqrt(1.0 / np.sqrt(s)) if s > 1.0 else 1.0
        rows = slice(D * o, D * o + D)
        ci, pj = bp.cam_idx[o] - nf, 6 * m + 3 * bp.pt_idx[o]
        if ci >= 0:
            J[rows, 6 * ci:6 * ci + 6] = sc * Jc[o]
        J[rows, pj:pj + 3] = sc * Jp[o]
    C = np.linalg.inv(J.T @ J)
    cam = np.zeros((len(bp.cams), 6, 6))
    for i in range(m):
        cam[nf + i] = C[6 * i:6 * i + 6, 6 * i:6 * i + 6]
    pt = np.stack([C[6 * m + 3 * j:6 * m + 3 * j + 3, 6 * m + 3 * j:6 * m + 3 * j + 3] for j in range(npt)])
    return cam, pt


def ref_covariance(oracle, bp):
    """window_cov_ref on the oracle's residuals and Jacobians of bp."""
    from uasl_motion_estimation_amd.ba_cov import window_cov_ref

    r, Jc, Jp = oracle.ba_evaluate(bp)
    return window_cov_ref(r, Jc, Jp, bp.cam_idx, bp.pt_idx, len(bp.cams), len(bp.pts), bp.fixed_frames)


def assert_cam_blocks(got, ref):
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL * np.abs(ref).max())


def assert_pt_blocks(got, ref):
    assert got.shape == ref.shape
    scale = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    err = np.abs(got - ref) - RTOL * np.abs(ref)
    worst = (err.reshape(len(ref), -1).max(axis=1) / scale) if len(ref) else np.zeros(0)
    bad = np.nonzero(~(worst <= ATOL))[0]
    assert bad.size == 0, f"{bad.size} landmark blocks off the bar, worst {worst[bad].max():.3e} (landmark {bad[0]})"


def keep_obs(bp, keep):
    """bp with only the observations keep[o] (a copy; parameters shared)."""
    out = bp.copy()
    out.obs, out.cam_idx, out.pt_idx = bp.obs[keep], bp.cam_idx[keep], bp.pt_idx[keep]
    if bp.cam_id is not None:
        out.cam_id = bp.cam_id[keep]
    return out


def fixed_only_landmark(bp):
    """bp with landmark 0 seen by one constant camera only: its observations in
    the variable cameras deleted and one kept in a constant camera (its first
    observation is moved to camera 0 when it has none there)."""
    nf = n_fixed(bp)
    mine = np.nonzero(bp.pt_idx == 0)[0]
    in_fixed = mine[bp.cam_idx[mine] < nf]
    out = bp.copy()
    if in_fixed.size == 0:
        out.cam_idx = bp.cam_idx.copy()
        out.cam_idx[mine[0]] = 0
        in_fixed = mine[:1]
    keep = np.ones(len(bp.obs), bool)
    keep[mine] = False
    keep[in_fixed[0]] = True
    return keep_obs(out, keep)
