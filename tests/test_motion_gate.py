"""Rigid-motion gate of the tracked features (include/me_hip.h A12h), the
parts that need no GPU: the numpy restatement motion_gate.motion_gate_ref on
synthetic observation sets, its abstention classes, the configuration checks,
the loop switch PipelineConfig.motion_gate on the oracle backend and the C++
caller's build.  The device side is tests/test_motion_gate_gpu.py.
"""
import dataclasses
import math

import numpy as np
import pytest

import motion_gate_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.motion_gate import MotionGate, motion_gate_ref, sample_ref

T = 3  # the keyframe number of the single-call tests


def gate(o, p=None, t=T):
    return motion_gate_ref(*o.args, *C.CAM, t, p or MotionGate())


def in_margin(o):
    u, v = o.cur[:, 0], o.cur[:, 1]
    return (u >= C.MARGIN) & (u < C.W - C.MARGIN) & (v >= C.MARGIN) & (v < C.H - C.MARGIN)


# ------------------------------------------------------------------ the restatement
def test_a_static_scene_without_noise_loses_nothing():
    o = C.scene(200, 0.0, 0.0)
    ok, err, info = gate(o)
    assert info["abstained"] == 0 and info["n_valid"] > 0
    assert np.array_equal(ok, o.ok)
    usable = in_margin(o)
    assert info["n_usable"] == info["n_inliers"] == int(usable.sum()) > 150
    assert np.all(err[usable] < 1e-3) and np.all(np.isinf(err[~usable]))  # (float32 observations: ~1e-5 px)
    np.testing.assert_allclose(info["R"], C.CAM_MOTION[0], atol=1e-6)
    np.testing.assert_allclose(info["t"], C.CAM_MOTION[1], atol=1e-5)


def test_the_prototype_case_keeps_no_mover():
    """200 tracks, a quarter on a second body, 0.25 px noise, the defaults."""
    o = C.scene(200)
    ok, err, info = gate(o)
    usable = in_margin(o)
    assert info["abstained"] == 0 and int(o.mover.sum()) == 50
    assert int((usable & o.mover).sum()) >= 40  # (movers the gate had to decide on)
    assert not np.any(ok[usable & o.mover])  # no mover kept
    # the static tracks this seed drops: read off the restatement, not chosen
    dropped = int((usable & ~o.mover & (ok == 0)).sum())
    print("static tracks dropped: %d of %d" % (dropped, int((usable & ~o.mover).sum())))
    assert dropped == STATIC_DROPPED
    np.testing.assert_allclose(info["t"], C.CAM_MOTION[1], atol=0.02)
    # without the refinement the same winner drops many more of them (the reason it is in the definition)
    ok0, _, info0 = gate(o, MotionGate(refine=0))
    assert info0["winner"] == info["winner"] and info0["n_inliers"] < info["n_inliers"]


STATIC_DROPPED = 0


def test_the_result_depends_on_seed_and_keyframe_only_through_the_sampler():
    o = C.scene(200)
    p = MotionGate(n_hyp=32)
    usable = in_margin(o)
    idx, found = sample_ref(usable, T, p)
    assert found.all() and np.all(usable[idx])
    assert np.all(idx[:, 0] != idx[:, 1]) and np.all(idx[:, 0] != idx[:, 2]) and np.all(idx[:, 1] != idx[:, 2])
    other_t, _ = sample_ref(usable, T + 1, p)
    other_s, _ = sample_ref(usable, T, dataclasses.replace(p, seed=1))
    assert not np.array_equal(idx, other_t) and not np.array_equal(idx, other_s)
    a, b = gate(o, p), gate(o, p)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ------------------------------------------------------------------ abstention
def assert_abstained(o, ok, info):
    assert info["abstained"] == 1 and np.array_equal(ok, o.ok)


def test_fewer_than_three_usable_features_abstain():
    o = C.scene(64)
    for keep in (0, 1, 2):
        st = np.zeros(64, np.uint8)
        st[np.flatnonzero(in_margin(o))[:keep]] = 1
        oo = C.Obs(o.prev, o.cur, st, o.ok, o.mover)
        ok, err, info = gate(oo)
        assert_abstained(oo, ok, info)
        assert info["n_usable"] == keep and info["n_valid"] == 0 and info["winner"] == -1
        assert np.all(np.isinf(err))


def test_collinear_points_void_every_hypothesis():
    o = C.collinear()
    ok, err, info = gate(o)
    assert_abstained(o, ok, info)
    assert info["n_usable"] == 40 and info["n_valid"] == 0 and info["winner"] == -1 and np.all(np.isinf(err))


def test_a_best_count_below_min_inliers_abstains():
    o = C.scene(200)
    ok, err, info = gate(o, MotionGate(min_inliers=190))
    assert_abstained(o, ok, info)
    assert info["winner"] >= 0 and 100 < info["n_inliers"] < 190
    assert np.isfinite(err[in_margin(o)]).all()  # the pose exists: its errors are reported


def test_features_that_are_not_usable_pass_through():
    o = C.mixed_flags(C.scene(200))
    ok, err, info = gate(o)
    assert info["abstained"] == 0
    good = (o.status == 1) & (o.ok != 0) & in_margin(o)
    d0 = o.prev[:, 0].astype(np.float64) - o.prev[:, 2]
    d1 = o.cur[:, 0].astype(np.float64) - o.cur[:, 2]
    usable = good & (d0 >= 0.5) & (d1 >= 0.5)
    assert int((good & ~usable).sum()) >= 5 and info["n_usable"] == int(usable.sum())
    assert np.array_equal(ok[~usable], o.ok[~usable])  # byte for byte, the far but good ones among them
    assert np.all(np.isinf(err[~usable]))
    assert np.any(ok[usable] == 0) and set(np.unique(ok[usable])) <= {0, 1, 2}
    kept = usable & (ok != 0)
    assert np.array_equal(ok[kept], o.ok[kept]) and not np.any(kept & o.mover)


def test_points_behind_the_camera_under_the_winner_are_no_inliers():
    o = C.behind()
    ok, err, info = gate(o)
    usable = in_margin(o)
    assert info["abstained"] == 0 and int((usable & o.mover).sum()) >= 5
    assert int(np.isinf(err[usable & o.mover]).sum()) >= 5 and not np.any(ok[usable & o.mover])  # Y_z <= 0: no error
    assert np.all(ok[usable & ~o.mover] == 1)


# ------------------------------------------------------------------ configuration
@pytest.mark.parametrize("kw", [dict(gate_max=0.0), dict(gate_max=math.nan), dict(gate_max=-1.0), dict(min_disp=0.0),
                                dict(min_disp=math.inf), dict(n_hyp=0), dict(n_hyp=1025), dict(n_hyp=2.5),
                                dict(refine=-1), dict(refine=9), dict(min_inliers=2), dict(seed=-1),
                                dict(seed=2 ** 32), dict(n_hyp=True)])
def test_parameter_checks(kw):
    with pytest.raises(ValueError) as e:
        MotionGate(**kw)
    assert list(kw)[0] in str(e.value)


def test_pipeline_config_takes_a_motion_gate_or_none():
    assert PL.PipelineConfig(160, 120, 48, 4).motion_gate is None
    g = MotionGate(n_hyp=64)
    assert PL.PipelineConfig(160, 120, 48, 4, motion_gate=g).motion_gate is g
    for bad in (True, 2.0, dict(gate_max=2.0)):
        with pytest.raises(ValueError) as e:
            PL.PipelineConfig(160, 120, 48, 4, motion_gate=bad)
        assert "motion_gate" in str(e.value)
    with pytest.raises(ValueError):
        PL.PipelineConfig(160, 120, 48, 4, motion_gate=g, baseline=0.0)
    c = g.to_c()
    assert (c.gate_max, c.min_disp, c.n_hyp, c.refine, c.min_inliers, c.seed) == (2.0, 0.5, 64, 3, 10, 0)


# ------------------------------------------------------------------ the loop switch
def test_the_loop_drops_the_overlay_tracks(oracle):
    off, _ = C.oracle_loop(None)
    adds_off = C.rect_adds(off)
    assert sum(adds_off.values()) >= 10 and len(adds_off) >= 4  # without the gate the overlay's tracks are believed
    on, be = C.oracle_loop(C.loop_gate())
    log = dict(be.gate_log)
    assert sorted(log) == list(range(1, C.N_KEYFRAMES))  # every keyframe with tracked features ran the gate
    ran = [t for t, info in log.items() if not info["abstained"]]
    assert len(ran) >= 4
    adds_on = C.rect_adds(on)
    assert all(adds_on.get(t, 0) == 0 for t in ran), (adds_on, ran)
    # the background is still tracked, and the cells the overlay's tracks left were refilled in the same keyframe
    assert all(r.n_tracked >= 6 for r in on.results[1:])
    assert sum(r.n_new for r in on.results[1:]) > sum(r.n_new for r in off.results[1:])
    assert off.be.gate_log is None  # gate off: the restatement never ran


def test_the_gate_left_off_changes_nothing(oracle):
    """A loop whose configuration never mentions the gate, and one that says None."""
    from pipeline_oracle import OracleBackend

    off, _ = C.oracle_loop(None)
    _, K, p0, v = C.stream()
    plain = C.run_loop(PL.WindowedStereoVO(PL.PipelineConfig(C.SW, C.SH, 48, 4, ba_iters=2), OracleBackend(), K, p0, v,
                                           log_events=True))
    assert plain.events == off.events


def test_cpp_caller_builds(tmp_path):
    import os

    exe = C.build_cli(tmp_path)
    assert os.access(exe, os.X_OK)
