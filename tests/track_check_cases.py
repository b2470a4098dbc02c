"""Shared by test_track_check.py (CPU) and test_track_check_gpu.py (TEST
INFRASTRUCTURE): the plain double-loop statement of the residual check, the
problems it is run on, the band around chi2_max inside which a flag may differ
between two residual evaluations, and the loop on the oracle backend over the
overlay stream of motion_gate_cases.py."""
import numpy as np

import motion_gate_cases as MG
from uasl_motion_estimation_amd import synthetic as S
from uasl_motion_estimation_amd.track_check import TrackCheck, depths, point_check_ref

BAND = 1e-6  # flags are compared for landmarks whose reference chi2 is further than BAND * chi2_max from chi2_max


def plain_check(r, Z, pt_idx, n_pts, params):
    """The rule of include/me_hip.h as a double loop over landmarks and
    observations, Python floats (IEEE doubles, one rounding per operation)."""
    chi2 = np.zeros(n_pts)
    flags = np.zeros(n_pts, np.uint8)
    r = np.asarray(r, np.float64)
    for i in range(n_pts):
        m, behind = 0.0, False
        for o in np.nonzero(np.asarray(pt_idx) == i)[0]:
            row = [float(x) for x in r[o]] + [0.0] * (4 - r.shape[1])
            s = ((row[0] * row[0] + row[1] * row[1]) + row[2] * row[2]) + row[3] * row[3]
            if not np.isfinite(s):
                s = float("inf")
            m = max(m, s)
            behind = behind or not (float(Z[o]) > params.z_min)
        chi2[i] = m
        flags[i] = (0 if m <= params.chi2_max else 1) | (2 if behind else 0)
    return chi2, flags


def mono_long(seed=57, n_pts=120, window=50):
    """A mono 50-camera window in which every track is seen in both images
    (each stereo observation of S.ba_problem as a left and a right
    Observation<2>): a landmark seen by more than 32 cameras holds more than 64
    observations, a wavefront's worth."""
    bp = S.ba_problem(seed, n_pts, window, 640, 480)
    n = len(bp.obs)
    obs = np.ascontiguousarray(np.concatenate([bp.obs[:, 0:2], bp.obs[:, 2:4]]))
    cam_id = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])
    return S.BAProblem(bp.cams, bp.pts, obs, np.tile(bp.cam_idx, 2), np.tile(bp.pt_idx, 2), bp.K0, bp.K1, bp.baseline,
                       bp.feat_var, bp.fixed_frames, bp.cams_true, bp.pts_true, 2, cam_id)


# name -> builder: the windows the device check is compared on, after 5 LM iterations
PROBLEMS = {
    "stereo_200x8": lambda: S.ba_problem(48, 200, 8, 640, 480),
    "mono_200x8": lambda: S.ba_problem_mono(49, 200, 8, 640, 480),
    "stereo_60x5": lambda: S.ba_problem(42, 60, 5, 640, 480),
    "stereo_100x26": lambda: S.ba_problem(56, 100, 26, 640, 480),
    "mono_long_50": mono_long,
}


def oracle_check(oracle, bp, params=None):
    """point_check_ref on the oracle's residuals of bp: (chi2, flags)."""
    r = oracle.ba_evaluate(bp)[0]
    return point_check_ref(r, depths(bp), bp.pt_idx, len(bp.pts), params or TrackCheck())


def in_band(chi2, params, band=BAND):
    """Landmarks whose chi2 lies within band * chi2_max of chi2_max."""
    return np.abs(np.asarray(chi2) - params.chi2_max) <= band * params.chi2_max


def chi2_bound(ref):
    """|chi2 - ref| allowed between two residual evaluations that agree at the
    project's residual bar (rtol 1e-12, atol 1e-9, tests/test_golden.py): for
    rows r_k off by e_k <= 1e-12 |r_k| + 1e-9, the sum of four squares moves by
    at most sum 2 |r_k| e_k (+ e_k^2) <= 2e-12 chi2 + 2e-9 sum |r_k|, and
    sum |r_k| <= 2 sqrt(chi2) over four rows."""
    ref = np.asarray(ref, np.float64)
    return 2e-12 * ref + 4e-9 * np.sqrt(ref)


def shuffled(bp, seed=0):
    """bp with its observation arrays in another order (a copy; parameters shared)."""
    perm = np.random.default_rng(seed).permutation(len(bp.obs))
    out = bp.copy()
    out.obs, out.cam_idx, out.pt_idx = bp.obs[perm], bp.cam_idx[perm], bp.pt_idx[perm]
    if bp.cam_id is not None:
        out.cam_id = bp.cam_id[perm]
    return out


# ------------------------------------------------------------------ the loop switch
def oracle_backend():
    """The oracle backend with residuals of its own for the check (oracle/ba.cpp's, not the numpy restatement's)."""
    import oracle as O
    from pipeline_oracle import OracleBackend

    class Checked(OracleBackend):
        def ba_residuals(self, bp):
            return O.ba_evaluate(bp)[0]

    return Checked()


_RUNS = {}


def oracle_loop(check):
    """(loop, backend) of the sequential loop on the oracle backend over
    motion_gate_cases.stream() with PipelineConfig(track_check=check), cached."""
    from uasl_motion_estimation_amd import pipeline as PL

    key = None if check is None else (check.chi2_max, check.z_min)
    if key not in _RUNS:
        _, K, p0, v = MG.stream()
        be = oracle_backend()
        vo = PL.WindowedStereoVO(MG.loop_config(track_check=check), be, K, p0, v, log_events=True)
        _RUNS[key] = (MG.run_loop(vo), be)
    return _RUNS[key]


def expected_flagged(be, params):
    """What flagged() must be, from the backend's log of every window's chi2
    and the rule: per window (keyframe t, in order) the window's track IDs with
    flags != 0 -- every window track is still in the table when its result is
    applied (the loop pops one keyframe per step; a window's tracks were seen
    after the popped one)."""
    out = []
    for t, wids, chi2, flags in be.check_log:
        want = (~(chi2 <= params.chi2_max)).astype(np.uint8) | (flags & 2)
        assert np.array_equal(want, flags)
        out += [(t, int(i), int(f)) for i, f in zip(wids, flags) if f]
    return out
