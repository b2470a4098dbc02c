"""Keyframe selection (include/me_hip.h A12i), the parts that need no GPU: the
numpy restatement keyframe.kf_update_ref against a brute-force statement of
the definition over the case table, the parameter checks, WindowedStereoVO.push
on the oracle backend and the C++ caller's build.  The device side is
tests/test_keyframe_gpu.py.
"""
import math
import struct

import numpy as np
import pytest

import keyframe_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.keyframe import KeyframeSelect, info_bytes, kf_update_ref, parse_info


def brute(c):
    """The definition feature by feature: a Python loop, sorted, the rank picked by index."""
    f32 = np.float32
    n = len(c.ref)
    cur, alive, d2 = c.cur.copy(), np.zeros(n, np.uint8), []
    for k in range(n):
        u, v = c.new[k]
        a = bool(c.alive[k] != 0 and c.status[k] == 1 and math.isfinite(u) and math.isfinite(v)
                 and u >= f32(C.MARGIN) and u < f32(C.W) - f32(C.MARGIN) and v >= f32(C.MARGIN)
                 and v < f32(C.H) - f32(C.MARGIN))
        if a:
            cur[k] = c.new[k]
            dx, dy = float(cur[k, 0]) - float(c.ref[k, 0]), float(cur[k, 1]) - float(c.ref[k, 1])
            d2.append((dx * dx) + (dy * dy))
            alive[k] = 1
    m = len(d2)
    med2 = sorted(d2)[(m - 1) >> 1] if m else 0.0
    p = c.params
    flags = ((1 if (n == 0 or 100 * m < p.min_tracked_pct * n) else 0) | (2 if 0.0 < p.min_parallax * p.min_parallax <= med2 else 0)
             | (4 if c.gap >= p.max_gap else 0))
    return cur, alive, dict(n=n, m=m, rank=(m - 1) >> 1, flags=flags, med2=med2, keyframe=flags != 0)


@pytest.mark.parametrize("name", list(C.cases()))
def test_restatement_is_the_brute_force_statement(name):
    c = C.cases()[name]
    cur, alive, info = kf_update_ref(*c.args)
    bcur, balive, binfo = brute(c)
    assert np.array_equal(cur.view(np.uint32), bcur.view(np.uint32)) and np.array_equal(alive, balive)
    assert struct.pack("<d", info.pop("med2")) == struct.pack("<d", binfo.pop("med2"))
    assert info == binfo
    info["med2"] = 0.0
    assert parse_info(info_bytes(info)) == info


def test_the_cases_reach_what_they_are_for():
    got = {k: kf_update_ref(*c.args) for k, c in C.cases().items()}
    for name, (_, want) in C.boundaries().items():
        assert got[f"bound-{name}"][2]["flags"] == want, name
    for n in C.N_FEW:
        assert got[f"all_alive-n{n}"][2]["m"] == n and got[f"all_dead-n{n}"][2]["m"] == 0
        assert got[f"all_dead-n{n}"][2]["med2"] == 0.0 and got[f"all_dead-n{n}"][2]["rank"] == -1
        assert got[f"one_alive-n{n}"][2]["m"] == 1
        assert got[f"equal-n{n}"][2]["med2"] == 25.0 and got[f"zeros-n{n}"][2]["med2"] == 0.0
        if n >= 2:
            assert got[f"even-n{n}"][2]["m"] % 2 == 0 and got[f"odd-n{n}"][2]["m"] % 2 == 1
        c = C.cases()[f"stay_dead-n{n}"]
        cur, alive, _ = got[f"stay_dead-n{n}"]
        dead = c.alive == 0
        assert not alive[dead].any() and np.array_equal(cur[dead].view(np.uint32), c.cur[dead].view(np.uint32))
        assert np.array_equal(cur[~dead], c.new[~dead])
        c = C.cases()[f"statuses-n{n}"]
        assert np.array_equal(got[f"statuses-n{n}"][1], (c.status == 1).astype(np.uint8))
        assert got[f"not_finite-n{n}"][2]["m"] == int((np.arange(n) % 4 == 3).sum())
    assert got["huge-n257"][2]["med2"] > 1e70 or got["huge-n257"][2]["m"] > 0
    m = got["margins-n257"]
    k = np.arange(257)
    on = (k // 2) % 4 % 2 == 0  # on the margin / on the far bound alternate with one float below
    far = (k // 2) % 4 == 2
    assert np.array_equal(m[1].astype(bool), np.where(far, False, on) | ((k // 2) % 4 == 3))
    t = got["tie-n257"][2]
    assert t["med2"] == 25.0
    lo = C.cases()["low_byte-n257"]
    d2 = 128.0 ** 2 + (lo.new[:, 1].astype(np.float64) - lo.ref[:, 1].astype(np.float64)) ** 2
    assert len(set(d2.view(np.uint64) >> np.uint64(8))) == 1 and len(set(d2.view(np.uint64) & np.uint64(255))) == 16
    hi = C.cases()["high_byte-n257"]
    d2 = (hi.new[:, 0].astype(np.float64) - hi.ref[:, 0].astype(np.float64)) ** 2
    assert len(set(d2.view(np.uint64) & np.uint64((1 << 56) - 1))) == 1 and len(set(d2.view(np.uint64) >> np.uint64(56))) == 4
    assert got["general-n0"][2] == dict(n=0, m=0, rank=-1, flags=1, med2=0.0, keyframe=True)


@pytest.mark.parametrize("kw", [dict(min_parallax=-1.0), dict(min_parallax=math.nan), dict(min_parallax=math.inf),
                                dict(min_parallax="x"), dict(min_tracked_pct=-1), dict(min_tracked_pct=101),
                                dict(min_tracked_pct=50.0), dict(max_gap=0), dict(max_gap=True), dict(max_gap=2.5)])
def test_parameter_checks(kw):
    with pytest.raises(ValueError) as e:
        KeyframeSelect(**kw)
    assert list(kw)[0] in str(e.value)


def test_defaults_and_the_pipeline_switch():
    d = KeyframeSelect()
    assert (d.min_parallax, d.min_tracked_pct, d.max_gap) == (12.0, 60, 10)
    c = d.to_c()
    assert (c.min_parallax, c.min_tracked_pct, c.max_gap) == (12.0, 60, 10)
    assert PL.PipelineConfig(160, 120, 48, 4).keyframe_select is None
    for bad in (True, 3, dict(max_gap=3)):
        with pytest.raises(ValueError, match="keyframe_select"):
            PL.PipelineConfig(160, 120, 48, 4, keyframe_select=bad)
    from uasl_motion_estimation_amd.tonemap import ToneMap

    with pytest.raises(ValueError, match="tonemap"):
        PL.PipelineConfig(160, 120, 48, 4, keyframe_select=d, tonemap=ToneMap())
    with pytest.raises(ValueError, match="gap"):
        kf_update_ref(*C.cases()["general-n2"].args[:8], 0, d)


def test_sub_frames_leave_the_keyframes_alone():
    from uasl_motion_estimation_amd import synthetic as S

    a, b = S.trajectory_arc(4), S.trajectory_arc(4, sub=1)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    dense = S.trajectory_arc(10, sub=3)
    for k in range(4):
        np.testing.assert_allclose(dense[3 * k][0], a[k][0], atol=1e-15)
        np.testing.assert_allclose(dense[3 * k][1], a[k][1], atol=1e-12)
    with pytest.raises(ValueError):
        S.trajectory_arc(3, sub=0)


# ------------------------------------------------------------------ the loop on the oracle backend
def plain_loop(frames_idx):
    from pipeline_oracle import OracleBackend

    _, K, p0, v = C.stream()
    return C.run_process(PL.WindowedStereoVO(C.loop_config(), OracleBackend(), K, p0, v, log_events=True), frames_idx)


def test_push_needs_the_switch(oracle):
    from pipeline_oracle import OracleBackend

    fr, K, p0, v = C.stream()
    vo = PL.WindowedStereoVO(C.loop_config(), OracleBackend(), K, p0, v)
    with pytest.raises(ValueError, match="keyframe_select"):
        vo.push(fr[0].left, fr[0].right)


def test_max_gap_one_is_the_process_loop(oracle):
    vo, kts = C.oracle_push(KeyframeSelect(max_gap=1))
    assert kts == list(range(C.N_FRAMES))
    assert not any(r["guided"] for r in vo.kf_log)
    plain = plain_loop(range(C.N_FRAMES))
    assert vo.events == plain.events
    assert all(np.array_equal(a.pose, b.pose) for a, b in zip(vo.results, plain.results))


def test_gap_rule_alone_gives_every_third_frame(oracle):
    vo, kts = C.oracle_push(KeyframeSelect(min_parallax=0.0, min_tracked_pct=0, max_gap=3))
    assert [i for i, t in enumerate(kts) if t >= 0] == list(range(0, C.N_FRAMES, 3))
    assert [t for t in kts if t >= 0] == list(range(5))
    log = [r for r in vo.kf_log if r["t"] >= 1]
    assert all(r["guided"] and r["gap"] == 3 and r["flags"] == 4 for r in log)


def test_defaults_on_the_stream(oracle):
    d = KeyframeSelect()
    vo, kts = C.oracle_push(d)
    print("keyframes:", kts, [(r["gap"], r["flags"], r["m"], r["n"], round(r["med2"], 2)) for r in vo.kf_log])
    assert kts[0] == 0 and [t for t in kts if t >= 0] == list(range(max(kts) + 1))
    assert all(r["gap"] <= d.max_gap for r in vo.kf_log)
    for r in vo.kf_log[1:]:
        assert (r["flags"] != 0) == (r["t"] >= 0)
    assert any(t < 0 for t in kts) and max(kts) >= 1  # the stream has both kinds of frame
    # the events are those of the frames that became keyframes: a process() loop over them, guided like push()
    want_kts, want_digest = C.golden()
    assert kts == want_kts and C.events_digest(vo.events) == want_digest


def test_frames_that_are_no_keyframes_leave_no_trace(oracle):
    """The frames between keyframes touch nothing but the carried state: a
    process() loop over the keyframes alone, handed the same guesses, gives the same events."""
    from pipeline_oracle import OracleBackend

    sel = KeyframeSelect(min_parallax=0.0, min_tracked_pct=0, max_gap=3)
    vo, kts = C.oracle_push(sel)
    fr, K, p0, v = C.stream()
    # the guesses push() used, recorded by following the same frames with a second backend
    be = OracleBackend()
    ref = PL.WindowedStereoVO(C.loop_config(sel), be, K, p0, v, log_events=True)
    seen = []
    orig = ref.process

    def spy(t, left, right, guess=None):
        seen.append(None if guess is None else np.array(guess))
        return orig(t, left, right, guess=guess)

    ref.process = spy
    C.run_push(ref)
    plain = PL.WindowedStereoVO(C.loop_config(), OracleBackend(), K, p0, v, log_events=True)
    for t, i in enumerate(range(0, C.N_FRAMES, 3)):
        plain.process(t, fr[i].left, fr[i].right, guess=seen[t])
    plain.finish()
    assert plain.events == vo.events


def test_cpp_caller_builds(tmp_path):
    import os

    assert os.access(C.build_cli(tmp_path), os.X_OK)
