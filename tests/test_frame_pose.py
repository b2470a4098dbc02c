"""Frame pose (include/me_hip.h A12j), the parts that need no GPU: the numpy
restatement frame_pose.frame_pose_ref bit for bit against an independent
scalar statement of the header over the case table, what the cases are there
to reach, the parameter checks, WindowedStereoVO.push on the oracle backend
with the switch on and the C++ caller's build.  The device side is
tests/test_frame_pose_gpu.py.
"""
import math
import struct

import numpy as np
import pytest

import frame_pose_cases as C
import keyframe_cases as KC
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.frame_pose import FramePose, frame_pose_ref, info_words, parse_info
from uasl_motion_estimation_amd.keyframe import KeyframeSelect


def bits(x):
    return struct.pack("<d", float(x))


@pytest.mark.parametrize("name", list(C.cases()))
def test_restatement_is_the_scalar_statement_bit_for_bit(name):
    c = C.cases()[name]
    err, info = C.reference(name)
    serr, sinfo = C.scalar_statement(c)
    print(name, {k: v for k, v in info.items() if k not in ("R", "t")})
    for k in ("n_usable", "n_act", "n_inliers", "steps", "valid"):
        assert info[k] == sinfo[k], k
    assert [bits(x) for x in info["R"].ravel()] == [bits(x) for row in sinfo["R"] for x in row]
    assert [bits(x) for x in info["t"]] == [bits(x) for x in sinfo["t"]]
    assert np.array_equal(err.view(np.uint32), np.array(serr, np.float32).view(np.uint32))
    back = parse_info(info_words(info))
    assert np.array_equal(info_words(back), info_words(info))
    w = info_words(info)
    assert w.dtype == np.uint32 and len(w) == 32 and not w[5:8].any()


def test_the_cases_reach_what_they_are_for():
    got = {k: C.reference(k) for k in C.cases()}
    for name, (err, info) in got.items():
        # IEEE leaves a NaN's sign and payload open: no expected output may hold one
        assert not np.isnan(info["R"]).any() and not np.isnan(info["t"]).any() and not np.isnan(err).any(), name
        assert info["valid"] == int(info["steps"] == C.cases()[name].params.iters
                                    and info["n_inliers"] >= C.cases()[name].params.min_inliers)
    ident = dict(n_usable=0, n_act=0, n_inliers=0, steps=0, valid=0)
    for name in ("general-n0", "all-dead-n65", "all-dead-n257"):
        info = got[name][1]
        assert {k: info[k] for k in ident} == ident and np.array_equal(info["R"], np.eye(3)) and not info["t"].any()
        assert np.all(np.isposinf(got[name][0]))
    for n in (3, 5, 6, 63, 64, 65, 255, 256, 257, 1025, 2049):
        info = got[f"general-n{n}"][1]
        assert 0 < info["n_usable"] < n or n < 10, n
    big = got["general-n2049"][1]
    assert big["valid"] == 1 and big["steps"] == 6 and big["n_inliers"] > 1000
    np.testing.assert_allclose(big["R"], C.G.CAM_MOTION[0], atol=2e-3)
    np.testing.assert_allclose(big["t"], C.G.CAM_MOTION[1], atol=2e-2)
    # fewer than 3 usable: no step at all, the start pose stays
    two = got["usable-2"][1]
    assert (two["n_usable"], two["steps"], two["valid"]) == (2, 0, 0) and np.array_equal(two["R"], np.eye(3))
    assert np.isfinite(got["usable-2"][0]).sum() == 2
    three = got["usable-3"][1]
    assert three["n_usable"] == 3 and three["steps"] >= 1 and three["valid"] == 0
    five = got["usable-5-below-min-inliers"][1]
    assert (five["n_usable"], five["steps"], five["valid"]) == (5, 6, 0) and five["n_inliers"] == 5
    assert got["on-min-disp"][1]["n_usable"] == 33
    nf = got["not-finite"]
    assert nf[1]["n_usable"] == 130 - len(range(0, 130, 3)) and np.all(np.isposinf(nf[0][::3]))
    beh = got["behind"][1]
    c = C.cases()["behind"]
    first = frame_pose_ref(*c.args[:7], FramePose(iters=0), start=c.start)[1]
    assert 0 < first["n_act"] < first["n_usable"] == 200  # under the start pose some points lie behind the camera
    assert beh["n_usable"] == 200
    idn = got["identical"][1]
    assert idn["steps"] < 6 and idn["valid"] == 0 and idn["n_usable"] == 70
    out = got["outliers-30"][1]
    assert out["valid"] == 1 and 150 < out["n_inliers"] < 0.75 * 300
    np.testing.assert_allclose(out["t"], C.G.CAM_MOTION[1], atol=3e-2)
    ov = got["overflow"]
    assert ov[1]["steps"] == 0 and ov[1]["t"][0] == 1e150 and ov[1]["n_act"] == 130 and np.all(np.isposinf(ov[0]))
    assert got["iters-0"][1]["steps"] == 0 and np.array_equal(got["iters-0"][1]["R"], np.eye(3))
    assert got["iters-0-warm"][1]["valid"] == 1 and np.array_equal(got["iters-0-warm"][1]["t"],
                                                                   C.cases()["iters-0-warm"].start["t"])
    assert got["iters-16"][1]["steps"] == 16 and got["iters-16"][1]["valid"] == 1
    # a block whose valid word is not 1 starts at identity: the same bits as no block at all
    none = frame_pose_ref(*C.cases()["start-valid"].args)[1]
    for name in ("start-invalid", "start-valid-word-2"):
        assert np.array_equal(info_words(got[name][1]), info_words(none))
    assert not np.array_equal(info_words(got["start-valid"][1]), info_words(none))
    assert np.array_equal(info_words(got["start-is-info"][1]), info_words(got["start-valid"][1]))
    assert got["loose"][1]["valid"] == 1 and got["loose"][1]["steps"] == 3


@pytest.mark.parametrize("kw", [dict(huber=0.0), dict(huber=-1.0), dict(huber=math.nan), dict(huber=math.inf),
                                dict(huber="x"), dict(huber=True), dict(gate_max=0.0), dict(gate_max=math.nan),
                                dict(min_disp=0.0), dict(min_disp=math.inf), dict(iters=-1), dict(iters=17),
                                dict(iters=2.0), dict(iters=True), dict(min_inliers=2), dict(min_inliers=6.0)])
def test_parameter_checks(kw):
    with pytest.raises(ValueError) as e:
        FramePose(**kw)
    assert list(kw)[0] in str(e.value)


def test_defaults_and_the_pipeline_switch():
    d = FramePose()
    assert (d.huber, d.gate_max, d.min_disp, d.iters, d.min_inliers) == (1.0, 2.0, 0.5, 6, 6)
    c = d.to_c()
    assert (c.huber, c.gate_max, c.min_disp, c.iters, c.min_inliers) == (1.0, 2.0, 0.5, 6, 6)
    FramePose(iters=0), FramePose(iters=16), FramePose(min_inliers=3)
    assert PL.PipelineConfig(160, 120, 48, 4).frame_pose is None
    with pytest.raises(ValueError, match="keyframe_select"):
        PL.PipelineConfig(160, 120, 48, 4, frame_pose=d)
    for bad in (True, 3, dict(iters=3)):
        with pytest.raises(ValueError, match="frame_pose"):
            PL.PipelineConfig(160, 120, 48, 4, keyframe_select=KeyframeSelect(), frame_pose=bad)
    with pytest.raises(ValueError, match="baseline"):
        PL.PipelineConfig(160, 120, 48, 4, keyframe_select=KeyframeSelect(), frame_pose=d, baseline=0.0)
    assert PL.PipelineConfig(160, 120, 48, 4, keyframe_select=KeyframeSelect(), frame_pose=d).frame_pose is d
    with pytest.raises(ValueError, match="length"):
        frame_pose_ref(np.zeros((3, 3)), np.zeros((2, 2)), np.ones(3), *C.CAM)
    import uasl_motion_estimation_amd as me

    assert me.FramePose is FramePose and me.frame_pose_ref is frame_pose_ref


# ------------------------------------------------------------------ the loop on the oracle backend
def test_the_switch_changes_nothing_else(oracle):
    vo, kts = C.oracle_push()
    want_kts, want_digest = KC.golden()
    assert kts == want_kts and KC.events_digest(vo.events) == want_digest
    off, _ = KC.oracle_push(KeyframeSelect())
    keys = ("frame", "t", "gap", "guided", "n", "m", "rank", "flags", "med2")
    assert [[r[k] for k in keys] for r in vo.kf_log] == [[r[k] for k in keys] for r in off.kf_log]
    assert all("t_ref" not in r for r in off.kf_log)
    assert all(np.array_equal(a.pose, b.pose) for a, b in zip(vo.results, off.results))
    with pytest.raises(ValueError, match="frame_pose"):
        off.frame_pose(1)


def test_every_pushed_frame_gets_a_valid_pose_that_beats_no_motion(oracle):
    vo, kts = C.oracle_push()
    log = vo.kf_log
    assert len(log) == KC.N_FRAMES and "t_ref" not in log[0]
    kf_frame = {t: i for i, t in enumerate(kts) if t >= 0}  # keyframe -> stream frame
    last = 0
    for i, r in enumerate(log[1:], 1):
        assert r["t_ref"] == last and r["pose_valid"] == 1 and r["steps"] == 6, r
        assert 6 <= r["n_inliers"] <= r["n_usable"] <= r["n"]
        _, t_true = C.true_motion(kf_frame[r["t_ref"]], i)
        e, m = np.linalg.norm(r["t_rel"] - t_true), np.linalg.norm(t_true)
        print(i, r["t_ref"], r["n_usable"], r["n_inliers"], "error %.3f m of %.3f m" % (e, m))
        if r["t"] < 0:
            assert e < m, (i, e, m)  # the estimate beats "no motion since the keyframe"
        else:
            last = r["t"]
    assert C.record_lines(log) == C.golden_lines()


def test_frame_pose_accessor(oracle):
    vo, kts = C.oracle_push()
    R0, t0, v0 = vo.frame_pose(0)
    assert v0 == 1 and np.array_equal(t0, vo.poses[0][:3]) and np.array_equal(R0, PL.aa_to_R(vo.poses[0][3:]))
    r = vo.kf_log[4]
    R, t, valid = vo.frame_pose(4)
    assert valid == 1
    assert np.array_equal(R, r["R_rel"] @ PL.aa_to_R(vo.poses[0][3:]))
    assert np.array_equal(t, r["R_rel"] @ vo.poses[0][:3] + r["t_rel"])
    # world -> camera: the frame's camera centre lies nearer the stream's own than the keyframe's does
    # (the loop test's condition again, in the world: the estimate beats holding the keyframe's pose)
    fr = KC.stream()[0]
    centre = -fr[4].R.T @ fr[4].t
    assert np.linalg.norm(-R.T @ t - centre) < np.linalg.norm(-R0.T @ t0 - centre)
    R12, _, _ = vo.frame_pose(12)  # relative to keyframe 1, which frame 10 became
    assert vo.kf_log[12]["t_ref"] == 1 and np.array_equal(R12, vo.kf_log[12]["R_rel"] @ PL.aa_to_R(vo.poses[1][3:]))


def test_cpp_caller_builds(tmp_path):
    import os

    assert os.access(C.build_cli(tmp_path), os.X_OK)
