"""The per-landmark residual check behind the BA on the CPU
(uasl_motion_estimation_amd/track_check.py; include/me_hip.h
me_ba_point_check): parameter validation, the numpy restatement against the
plain double loop on the oracle's residuals and on known answers, the loop
switch on the oracle backend over the overlay stream of motion_gate_cases.py,
the table's step on the host (tests/cpp/track_check_host.cpp over
csrc/vo_tracks.hpp alone) and the C++ adapter's setter and reader."""
import os
import subprocess

import numpy as np
import pytest

import motion_gate_cases as MG
import track_check_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd import synthetic as S
from uasl_motion_estimation_amd.track_check import (FLAG_BEHIND, FLAG_CHI2, TrackCheck, depths, point_check_problem,
                                                    point_check_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ parameters
def test_defaults_and_validation():
    p = TrackCheck()
    assert p.chi2_max == 18.47 and p.z_min == 0.0
    assert TrackCheck(chi2_max=float("inf")).chi2_max == float("inf")
    assert TrackCheck(5, 1).chi2_max == 5.0 and isinstance(TrackCheck(5, 1).z_min, float)
    for kw in (dict(chi2_max=0.0), dict(chi2_max=-1.0), dict(chi2_max=float("nan")), dict(z_min=-0.5),
               dict(z_min=float("inf")), dict(z_min=float("nan"))):
        with pytest.raises(ValueError):
            TrackCheck(**kw)


def test_pipeline_config_type_check():
    assert PL.PipelineConfig(160, 120, 48, 4).track_check is None
    assert PL.PipelineConfig(160, 120, 48, 4, track_check=TrackCheck()).track_check.chi2_max == 18.47
    for bad in (True, 18.47, {"chi2_max": 18.47}):
        with pytest.raises(ValueError):
            PL.PipelineConfig(160, 120, 48, 4, track_check=bad)


def test_ctypes_mirror_of_the_parameters_and_the_window(tmp_path):
    """me_ba_point_check_params and me_vo_window (with its trailing `check`) against the header, sizes and offsets."""
    import ctypes

    from uasl_motion_estimation_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "me_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d\\n", sizeof(me_ba_point_check_params), '
                   'offsetof(me_ba_point_check_params, z_min), sizeof(me_vo_window), offsetof(me_vo_window, check), '
                   '(int)ME_KT_BA_CHECK, (int)ME_KT_COUNT); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got[:2] == [ctypes.sizeof(_lib.PointCheckParamsC), _lib.PointCheckParamsC.z_min.offset]
    assert got[2:4] == [ctypes.sizeof(_lib.VOWindowC), _lib.VOWindowC.check.offset]
    assert got[4:] == [_lib.KT_MORE["BA_CHECK"], 19]
    c = TrackCheck(7.5, 0.25).to_c()
    assert (c.chi2_max, c.z_min) == (7.5, 0.25)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["stereo_60x5", "mono_60x5"])
@pytest.mark.parametrize("params", [TrackCheck(), TrackCheck(400.0, 9.0)], ids=["default", "other"])
def test_restatement_is_the_plain_double_loop(oracle, name, params):
    bp = S.ba_problem(42, 60, 5, 640, 480) if name == "stereo_60x5" else S.ba_problem_mono(51, 60, 5, 640, 480)
    r = oracle.ba_evaluate(bp)[0]
    assert r.shape[1] == (4 if name == "stereo_60x5" else 2)
    Z = depths(bp)
    chi2, flags = point_check_ref(r, Z, bp.pt_idx, len(bp.pts), params)
    pchi2, pflags = C.plain_check(r, Z, bp.pt_idx, len(bp.pts), params)
    assert np.array_equal(bits(chi2), bits(pchi2)) and np.array_equal(flags, pflags)
    assert flags.dtype == np.uint8 and 0 < np.count_nonzero(flags & FLAG_CHI2) < len(flags)
    if params.z_min > 0:
        assert np.any(flags & FLAG_BEHIND) and not np.all(flags & FLAG_BEHIND)
    # the helper that takes a problem and an evaluator (a tuple's first entry, or the residuals alone)
    for ev in (oracle.ba_evaluate, lambda b: oracle.ba_evaluate(b)[0]):
        c2, f2 = point_check_problem(bp, ev, params)
        assert np.array_equal(bits(c2), bits(chi2)) and np.array_equal(f2, flags)
    # another order of the observations: the same bits
    sh = C.shuffled(bp, 3)
    c3, f3 = point_check_problem(sh, oracle.ba_evaluate, params)
    assert np.array_equal(bits(c3), bits(chi2)) and np.array_equal(f3, flags)


def exact_problem(n_pts=40, window=5):
    """A window whose observations are the exact projections of its landmarks (no noise, no outliers)."""
    bp = S.ba_problem(43, n_pts, window, 640, 480, noise=0.0, outlier_frac=0.0)
    bp.cams, bp.pts, bp.feat_var = bp.cams_true.copy(), bp.pts_true.copy(), 0.25  # (sigma 0.5 px, as the loops')
    return bp


def test_known_answers(oracle):
    bp = exact_problem()
    ev = oracle.ba_evaluate
    chi2, flags = point_check_problem(bp, ev)
    # exact projections: zero to the rounding of the projection (pixels of a few hundred, sigma 0.5)
    assert chi2.max() < 1e-20 and not flags.any()
    # one observation shifted by k pixels in one row: chi2 = (k / sigma)^2 to rounding
    sigma = np.sqrt(bp.feat_var)
    for k, row in ((1.0, 0), (3.0, 2), (7.5, 1)):
        q = bp.copy()
        q.obs = bp.obs.copy()
        o = 11
        q.obs[o, row] += k
        c, f = point_check_problem(q, ev)
        i = int(bp.pt_idx[o])
        want = (k / sigma) ** 2
        assert abs(c[i] - want) <= 1e-9 * want
        assert f[i] == (FLAG_CHI2 if want > 18.47 else 0)
        assert np.delete(c, i).max() < 1e-20 and not np.delete(f, i).any()
    # a landmark without observations: 0 and no flag
    q = bp.copy()
    q.pts = np.vstack([bp.pts, [[0.5, 0.2, 10.0]]])
    c, f = point_check_problem(q, ev)
    assert c[-1] == 0.0 and f[-1] == 0 and len(c) == len(bp.pts) + 1
    # a landmark behind one of its cameras: bit 1 (and a large chi2 with it)
    q = bp.copy()
    q.pts = bp.pts.copy()
    i = int(bp.pt_idx[0])
    cam = bp.cams[bp.cam_idx[0]]
    R = PL.aa_to_R(cam[3:])
    q.pts[i] = R.T @ (np.array([0.1, 0.1, -2.0]) - cam[:3])  # depth -2 in that camera
    c, f = point_check_problem(q, ev)
    assert f[i] & FLAG_BEHIND and not (np.delete(f, i) & FLAG_BEHIND).any()
    # a NaN landmark: +inf and both bits
    q = bp.copy()
    q.pts = bp.pts.copy()
    q.pts[i, 1] = np.nan
    c, f = point_check_problem(q, ev)
    assert c[i] == np.inf and f[i] == (FLAG_CHI2 | FLAG_BEHIND) and not np.delete(f, i).any()
    # chi2_max = +inf: no chi2 is above it, +inf included; the depth bit stands
    c, f = point_check_problem(q, ev, TrackCheck(chi2_max=float("inf")))
    assert f[i] == FLAG_BEHIND and c[i] == np.inf


# ------------------------------------------------------------------ the loop switch (oracle backend)
def test_loop_drops_flagged_tracks_and_no_others():
    params = TrackCheck()
    vo, be = C.oracle_loop(params)
    off, _ = C.oracle_loop(None)
    fl = vo.flagged()
    ids = {i for _, i, _ in fl}
    all_ids = {int(ev[1]) for ev in vo.events if ev[0] == "new"}
    assert 0 < len(ids) < len(all_ids)
    assert all(f in (1, 2, 3) for _, _, f in fl)
    # no flagged (t, id) is added to after keyframe t + 1 (keyframe t + 1's add was booked before the result came)
    first = {}
    for t, i, _ in fl:
        first.setdefault(i, t)
    adds = [(int(ev[1]), int(ev[2])) for ev in vo.events if ev[0] == "add"]
    assert not [(i, t) for i, t in adds if i in first and t > first[i] + 1]
    # and some flagged track does stop there, where the loop without the switch goes on adding to it
    off_adds = {(int(ev[1]), int(ev[2])) for ev in off.events if ev[0] == "add"}
    assert any((i, t + 2) in off_adds for i, t in first.items())
    # flagged() is what the backend's log and the rule give, window by window
    assert fl == C.expected_flagged(be, params)
    assert [t for t, _, _, _ in be.check_log] == list(range(2, MG.N_KEYFRAMES))  # every window solved
    # the flagged tracks are inactive at the end; no event kind was added
    row = {int(i): k for k, i in enumerate(vo.ids)}
    assert all(not vo.active[row[i]] for i in ids if i in row)
    assert {ev[0] for ev in vo.events} <= {"new", "add", "pop", "del"}
    # n_active is counted after the step: never above the loop's without the switch until the tracks diverge
    assert vo.results[2].n_active <= off.results[2].n_active


def test_every_window_keeps_clear_of_the_bound():
    """The condition the GPU loops' comparison rests on, here on the CPU: in
    every window of the oracle loop no landmark's chi2 lies within 1e-6
    chi2_max of chi2_max (measured: the closest is 0.125 relative away, in the
    last window; 0.26, 0.48 and 0.48 in the others)."""
    params = TrackCheck()
    _, be = C.oracle_loop(params)
    for t, _, chi2, _ in be.check_log:
        assert not C.in_band(chi2, params).any(), t
        assert np.abs(chi2 - params.chi2_max).min() > 0.1 * params.chi2_max


def test_switch_off_is_the_loop_as_it_was():
    off, be = C.oracle_loop(None)
    with open(os.path.join(ROOT, "tests", "golden", "motion_gate_off_events.sha256")) as f:
        assert MG.events_digest(off.events) == f.read().split()[0]
    assert off.flagged() == [] and be.check_log is None


def test_failed_solve_applies_no_flags():
    """A solve that ends in FAILURE (status != 2) changes neither the state nor the active flags."""
    _, K, p0, v = MG.stream()
    be = C.oracle_backend()
    plain = be.ba_solve

    def failing(bp, iters):
        c, p, s = plain(bp, iters)
        return c, p, dict(s, status=3, termination=2)

    be.ba_solve = failing
    vo = MG.run_loop(PL.WindowedStereoVO(MG.loop_config(track_check=TrackCheck()), be, K, p0, v, log_events=True))
    assert vo.flagged() == [] and be.check_log is None


# ------------------------------------------------------------------ the table's step on the host
def test_table_step_on_the_host(tmp_path):
    """tests/cpp/track_check_host.cpp over csrc/vo_tracks.hpp alone: flags on a
    live row, on a row a pop moved, and for a row the pop deleted."""
    exe = str(tmp_path / "track_check_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpp", "track_check_host.cpp"), "-o", exe], check=True, timeout=120)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.split("\n")
    assert lines[:4] == ["case1 live_row applied=2 active=3", "case2 moved_row applied=1 row=2",
                         "case3 deleted_row ignored=1", "ok"]


def test_cpp_adapter_compiles_with_the_setter_and_the_reader(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "MotionEstimationAMD/motion_estimation_amd.hpp"\n'
                   'size_t use(me::WindowedStereoVO& vo) {\n'
                   '  vo.setTrackCheck(true);\n  vo.setTrackCheck(true, 25.0, 0.1);\n  vo.setTrackCheck(false);\n'
                   '  size_t n = 0;\n  for (const auto& f : vo.flagged()) n += (f.t >= 0) + (f.id >= 0) + f.flags;\n'
                   '  return n;\n}\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    str(src)], check=True, timeout=120)
