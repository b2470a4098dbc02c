"""Window covariance: the camera and landmark blocks of (J^T J)^-1 of a BA
window (me_ba_covariance_full, include/me_hip.h).

The reference treats the uncertainty as part of the result:
CalibrationParameters::compute_cov switches extract_covariance on inside
optimise (BundleAdjuster.h:424-425,471-472), CamPose carries a covariance, and
BundleAdjuster declares getPointsCovariance() / m_point_covs
(BundleAdjuster.h:239,277) whose computation is commented out (:498-523).

``window_cov_ref`` restates the device computation in numpy, by the Schur form
and never by a dense inverse: with the loss-corrected J = [Jc | Jp],
U = Jc^T Jc, V = Jp^T Jp (3 x 3 blocks V_j), W = Jc^T Jp,

    S          = U - W V^-1 W^T            (variable cameras only)
    Sigma_cc   = S^-1 = L^-T L^-1,  S = L L^T
    Sigma_pp,j = V_j^-1 + T_j^T Sigma_cc T_j,  T_j = W_j V_j^-1

The gauge is the BA's own: the window's first ``fixed`` cameras are constant,
so their blocks are zero (ceres::Covariance), and a landmark seen only by them
gets exactly V_j^-1."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class WindowCovariance:
    """Settings of the VO loops' covariance switch
    (PipelineConfig(covariance=WindowCovariance()), me_vo_loop_set_covariance):
    every window's covariance is taken at the cams / pts its solve leaves;
    ``landmarks`` also computes the landmark blocks (track_cov)."""
    landmarks: bool = True


def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def stereo_jacobians(bp):
    """(r (n_obs, 4), Jc (n_obs, 4, 6), Jp (n_obs, 4, 3)) of a stereo window
    (StereoReprojectionError, BundleAdjuster.h:142-180) in numpy: the raw
    residuals sinv (projection - observation) of the left (K0) and right (K1,
    x shifted by the baseline) image and their analytic Jacobians by the
    camera {t, angle-axis w} and the landmark, with d(R(w) X)/dw =
    -R [X]x Jr(w), Jr the right Jacobian of SO(3).  What a backend without a
    device hands to window_cov_ref."""
    cams = np.asarray(bp.cams, np.float64)[np.asarray(bp.cam_idx)]
    X = np.asarray(bp.pts, np.float64)[np.asarray(bp.pt_idx)]
    obs = np.asarray(bp.obs, np.float64)
    n = len(obs)
    w = cams[:, 3:]
    th2 = np.einsum("ij,ij->i", w, w)
    th = np.sqrt(th2)
    Wx = _skew(w)
    Wx2 = Wx @ Wx
    small = th2 < 1e-12
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)                      # sin t / t
    b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / ths ** 2)        # (1 - cos t) / t^2
    c = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / ths ** 3)  # (t - sin t) / t^3
    I = np.broadcast_to(np.eye(3), (n, 3, 3))
    R = I + a[:, None, None] * Wx + b[:, None, None] * Wx2
    Jr = I - b[:, None, None] * Wx + c[:, None, None] * Wx2
    P = np.einsum("nij,nj->ni", R, X) + cams[:, :3]
    dPdw = -R @ _skew(X) @ Jr
    sinv = 1.0 / np.sqrt(float(bp.feat_var))
    r = np.zeros((n, 4))
    Jc = np.zeros((n, 4, 6))
    Jp = np.zeros((n, 4, 3))
    for side, K, shift in ((0, np.asarray(bp.K0, np.float64).reshape(3, 3), 0.0),
                           (1, np.asarray(bp.K1, np.float64).reshape(3, 3), float(bp.baseline))):
        x, y, z = P[:, 0] - shift, P[:, 1], P[:, 2]
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        r[:, 2 * side] = sinv * (fx * x / z + cx - obs[:, 2 * side])
        r[:, 2 * side + 1] = sinv * (fy * y / z + cy - obs[:, 2 * side + 1])
        D = np.zeros((n, 2, 3))  # d(u, v) / dP
        D[:, 0, 0], D[:, 0, 2] = fx / z, -fx * x / z ** 2
        D[:, 1, 1], D[:, 1, 2] = fy / z, -fy * y / z ** 2
        D *= sinv
        Jc[:, 2 * side:2 * side + 2, :3] = D
        Jc[:, 2 * side:2 * side + 2, 3:] = D @ dPdw
        Jp[:, 2 * side:2 * side + 2] = D @ R
    return r, Jc, Jp


def huber_row_scale(r):
    """sqrt(rho') of HuberLoss(1.0) per observation: the factor the BA scales
    an observation's residual and Jacobian rows by (s = |r|^2 > 1: s^-1/4)."""
    r = np.asarray(r, np.float64)
    s = np.einsum("od,od->o", r, r)
    return np.where(s > 1.0, np.sqrt(1.0 / np.sqrt(np.maximum(s, 1.0))), 1.0)


def window_cov_ref(r, Jc, Jp, cam_idx, pt_idx, n_cams, n_pts, fixed):
    """(cam_cov (n_cams, 6, 6), pt_cov (n_pts, 3, 3)) from the raw residuals r
    (n_obs, D) and Jacobians Jc (n_obs, D, 6), Jp (n_obs, D, 3) of a window, or
    None when S or a V_j is not positive definite (a variable camera or a
    landmark without observations among them)."""
    r = np.asarray(r, np.float64)
    cam_idx = np.asarray(cam_idx, np.int64)
    pt_idx = np.asarray(pt_idx, np.int64)
    sc = huber_row_scale(r) if len(r) else np.zeros(0)
    Jc = np.asarray(Jc, np.float64) * sc[:, None, None]
    Jp = np.asarray(Jp, np.float64) * sc[:, None, None]
    nf = min(max(int(fixed), 0), n_cams)
    m = n_cams - nf
    n6 = 6 * m
    V = np.zeros((n_pts, 3, 3))
    np.add.at(V, pt_idx, np.einsum("oda,odb->oab", Jp, Jp))
    try:
        if n_pts:
            np.linalg.cholesky(V)
    except np.linalg.LinAlgError:
        return None
    Vi = np.linalg.inv(V) if n_pts else V
    Vi = 0.5 * (Vi + Vi.transpose(0, 2, 1))
    free = cam_idx >= nf
    ca = cam_idx[free] - nf
    S4 = np.zeros((m, 6, m, 6))
    Ublk = np.zeros((m, 6, 6))
    np.add.at(Ublk, ca, np.einsum("oda,odb->oab", Jc[free], Jc[free]))
    for i in range(m):
        S4[i, :, i, :] = Ublk[i]
    S = S4.reshape(n6, n6)
    # W_j dense (n6 x 3) per landmark: the observations' 6 x 3 blocks in their cameras' rows
    Wo = np.einsum("oda,odb->oab", Jc[free], Jp[free])
    Wd = np.zeros((n_pts, m, 6, 3))
    np.add.at(Wd, (pt_idx[free], ca), Wo)
    Wd = Wd.reshape(n_pts, n6, 3)
    T = Wd @ Vi  # (n_pts, n6, 3)
    S = S - np.einsum("jac,jbc->ab", T, Wd)
    S = 0.5 * (S + S.T)
    cam_cov = np.zeros((n_cams, 6, 6))
    if n6:
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None
        Li = np.linalg.inv(L)
        Scc = Li.T @ Li
        for i in range(m):
            cam_cov[nf + i] = Scc[6 * i:6 * i + 6, 6 * i:6 * i + 6]
        Y = np.einsum("ab,jbc->jac", Li, T)  # L^-1 T_j: T_j^T Sigma_cc T_j = Y_j^T Y_j
        pt_cov = Vi + np.einsum("jac,jad->jcd", Y, Y)
    else:
        pt_cov = Vi.copy()
    return cam_cov, pt_cov
