"""Per-landmark residual check behind a BA solve (me_ba_point_check,
include/me_hip.h).

The bundle adjustment is the one stage that sees a track against every camera
of the window.  After a solve, a landmark whose reprojection residual is still
tens of sigma in some camera does not belong to the rigid scene the window
describes; HuberLoss(1.0) only down-weights it.  The check names such
landmarks, and the VO loops' switch (PipelineConfig(track_check=TrackCheck()),
me_vo_loop_set_track_check) stops tracking them.

The rule, per observation o with the sigma-scaled residual r (4 rows; rows 2, 3
zero in the mono model) and the camera-frame depth Z_o:

    s_o = ((r0 r0 + r1 r1) + r2 r2) + r3 r3

and per landmark i over all of its observations (constant cameras included):

    chi2_i  = max s_o      (a non-finite s_o counts as +inf; none: 0)
    flags_i = 1 if not chi2_i <= chi2_max
            | 2 if some observation has not Z_o > z_min

A maximum and an "any": the result does not depend on the observations' order.
``point_check_ref`` restates it in numpy."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

FLAG_CHI2 = 1
FLAG_BEHIND = 2


@dataclass
class TrackCheck:
    """Parameters of the check (me_ba_point_check_params).  The defaults come
    from the statistics, not from real data: 18.47 is the 99.9 % point of
    chi-square with 4 degrees of freedom (a stereo observation's four rows at
    the stated sigma), z_min = 0 asks only that the landmark lies in front of
    every camera that sees it."""
    chi2_max: float = 18.47
    z_min: float = 0.0

    def __post_init__(self):
        self.chi2_max, self.z_min = float(self.chi2_max), float(self.z_min)
        if not self.chi2_max > 0.0:  # (false for NaN)
            raise ValueError("chi2_max must be > 0 (+inf allowed)")
        if not (math.isfinite(self.z_min) and self.z_min >= 0.0):
            raise ValueError("z_min must be finite and >= 0")

    def to_c(self):
        from ._lib import PointCheckParamsC

        return PointCheckParamsC(self.chi2_max, self.z_min)


def point_check_ref(r, Z, pt_idx, n_pts: int, params: TrackCheck | None = None):
    """(chi2 (n_pts,) float64, flags (n_pts,) uint8) from the residuals r
    (n_obs, 4) or (n_obs, 2), the depths Z (n_obs,) and the observations'
    landmarks pt_idx."""
    params = params or TrackCheck()
    r = np.asarray(r, np.float64).reshape(len(pt_idx), -1)
    Z = np.asarray(Z, np.float64).reshape(-1)
    pt_idx = np.asarray(pt_idx, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        for k in range(2, 4):
            s = s + (r[:, k] * r[:, k] if k < r.shape[1] else 0.0)
    s = np.where(np.isfinite(s), s, np.inf)
    chi2 = np.zeros(n_pts)
    np.maximum.at(chi2, pt_idx, s)
    behind = np.zeros(n_pts, bool)
    np.logical_or.at(behind, pt_idx, ~(Z > params.z_min))
    flags = (~(chi2 <= params.chi2_max)).astype(np.uint8) * FLAG_CHI2 | behind.astype(np.uint8) * FLAG_BEHIND
    return chi2, flags.astype(np.uint8)


def _rotate(aa, X):
    """R(aa) X per row, the angle-axis rotation of the BA residual (Rodrigues; first order below theta^2 = eps)."""
    t2 = np.einsum("ij,ij->i", aa, aa)
    small = ~(t2 > np.finfo(np.float64).eps)
    th = np.sqrt(np.where(small, 1.0, t2))
    w = aa / th[:, None]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    P = X * c + np.cross(w, X) * s + w * (np.einsum("ij,ij->i", w, X)[:, None] * (1.0 - c))
    return np.where(small[:, None], X + np.cross(aa, X), P)


def depths(bp):
    """The observations' camera-frame depths Z_o = (R X + t)[2] of a BAProblem."""
    cams = np.asarray(bp.cams, np.float64).reshape(-1, 6)[np.asarray(bp.cam_idx, np.int64)]
    X = np.asarray(bp.pts, np.float64).reshape(-1, 3)[np.asarray(bp.pt_idx, np.int64)]
    if len(cams) == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return _rotate(cams[:, 3:], X)[:, 2] + cams[:, 2]


def point_check_problem(bp, residuals, params: TrackCheck | None = None):
    """point_check_ref of a BAProblem at its current parameters:
    ``residuals(bp)`` gives the sigma-scaled residuals (n_obs, D), alone or as
    the first of a tuple (a ba_evaluate); the depths are ``depths(bp)``."""
    r = residuals(bp)
    if isinstance(r, tuple):
        r = r[0]
    return point_check_ref(np.asarray(r, np.float64).reshape(len(bp.pt_idx), -1), depths(bp), bp.pt_idx, len(bp.pts),
                           params)
