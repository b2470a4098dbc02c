"""Frame pose on the device (include/me_hip.h A12j, csrc/frame_pose.hip):
every info word and every err_out float of me_frame_pose bit for bit against
the numpy restatement frame_pose.frame_pose_ref over the case table, the
guard bytes around the outputs, the argument checks, the
push() loops against the oracle-backend run recorded in tests/golden, the loop
with the switch off, and the C++ caller.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import frame_pose_cases as C
import keyframe_cases as KC
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import MEError
from uasl_motion_estimation_amd.frame_pose import FramePose, frame_pose, frame_pose_ref, info_words
from uasl_motion_estimation_amd.keyframe import KeyframeSelect

pytestmark = pytest.mark.gpu

def check(c, got, want):
    """A device result against the restatement's: the words, the floats, and every byte that is no output."""
    err, info = got
    werr, winfo = want
    assert np.array_equal(info["words"], info_words(winfo)), (info, winfo)
    n = len(c.ref)
    blk, sent, o_err, o_info = info["block"], info["sent"], info["o_err"], info["o_info"]
    out = np.zeros(len(blk), bool)
    out[o_info:o_info + 128] = True
    if c.want_err:
        assert np.array_equal(err.view(np.uint32), werr.view(np.uint32))
        out[o_err:o_err + 4 * n] = True
    assert np.array_equal(blk[~out], sent[~out])  # inputs, the 0xEE guards, err's bytes when err_out is NULL
    assert np.all(blk[o_info - 16:o_info] == 0xEE) and np.all(blk[o_info + 128:] == 0xEE)
    assert np.all(blk[o_err - 16:o_err] == 0xEE) and np.all(blk[o_err + 4 * n:o_err + 4 * n + 16] == 0xEE)


@pytest.mark.parametrize("name", list(C.cases()))
def test_device_call_is_the_restatement_bit_for_bit(ctx, name):
    c = C.cases()[name]
    want = C.reference(name)
    got = frame_pose(*c.args, start=c.start, ctx=ctx, alias=c.alias, want_err=c.want_err)
    print(name, {k: v for k, v in want[1].items() if k not in ("R", "t")})
    check(c, got, want)


def test_each_frame_starts_where_the_last_one_ended(ctx):
    """Three calls in a row with start == info, the positions drifting on, against three of the restatement."""
    c = C.cases()["general-n1025"]
    start_d = start_r = C.block(np.eye(3), [0.0, 0.0, 0.0], valid=0)
    for step in range(3):
        cur = (c.cur + np.float32(0.4 * step)).astype(np.float32)
        werr, winfo = frame_pose_ref(c.ref, cur, c.alive, *C.CAM, c.params, start=start_r)
        gerr, ginfo = frame_pose(c.ref, cur, c.alive, *C.CAM, c.params, start=start_d, ctx=ctx, alias=True)
        assert np.array_equal(ginfo["words"], info_words(winfo)), step
        assert np.array_equal(gerr.view(np.uint32), werr.view(np.uint32))
        start_r, start_d = winfo, {k: ginfo[k] for k in winfo}
    assert winfo["valid"] == 1 and winfo["steps"] == 6


@pytest.mark.parametrize("field,bad", [("huber", 0.0), ("huber", float("nan")), ("gate_max", -1.0),
                                       ("gate_max", float("inf")), ("min_disp", 0.0), ("min_disp", float("nan")),
                                       ("iters", -1), ("iters", 17), ("min_inliers", 2)])
def test_bad_parameters_are_invalid(ctx, field, bad):
    c = C.cases()["general-n64"]
    p = FramePose()
    object.__setattr__(p, field, bad)  # (past FramePose's own check)
    with pytest.raises(MEError) as e:
        frame_pose(*c.args[:7], p, ctx=ctx)
    assert e.value.code == -1 and field in str(e.value) and "me_frame_pose" in str(e.value)


def test_bad_arguments_are_invalid_and_the_context_survives(ctx):
    V = ctypes.c_void_p
    pc = FramePose().to_c()
    one = ctx.malloc(4096)
    try:
        def call(n=64, null=None, f=C.F, b=C.B, cx=C.CX, info=one, params=ctypes.byref(pc)):
            a = [V(one)] * 4
            if null is not None:
                a[null] = None
            rc = ctx.lib.me_frame_pose(ctx.h, *a, n, f, cx, C.CY, b, params, None, None, V(info) if info else None)
            return rc, ctx.lib.me_last_error(ctx.h)

        for kw, word in ((dict(n=-1), b"n must"), (dict(n=(1 << 24) + 1), b"n must"), (dict(null=0), b"null ref_uv"),
                         (dict(null=1), b"null ref_xr"), (dict(null=2), b"null cur_uv"), (dict(null=3), b"null alive"),
                         (dict(f=0.0), b"f must"), (dict(f=float("nan")), b"f must"), (dict(b=-0.1), b"baseline"),
                         (dict(b=float("inf")), b"baseline"), (dict(cx=float("nan")), b"cx"),
                         (dict(info=0), b"null info"), (dict(info=one + 4), b"8-byte"),
                         (dict(params=None), b"null params")):
            rc, msg = call(**kw)
            assert rc == -1 and b"me_frame_pose" in msg and word in msg, (kw, msg)
        # n = 0 with null arrays is legal
        assert ctx.lib.me_frame_pose(ctx.h, None, None, None, None, 0, C.F, C.CX, C.CY, C.B, ctypes.byref(pc), None,
                                     None, V(one)) == 0
        ctx.synchronize()
    finally:
        ctx.free(one)
    c = C.cases()["general-n64"]
    check(c, frame_pose(*c.args, ctx=ctx), C.reference("general-n64"))


# ------------------------------------------------------------------ the loops
def native(ctx, frame_pose=C.D, **kw):
    _, K, p0, v = KC.stream()
    return PL.NativeStereoVO(C.loop_config(frame_pose), ctx, K, p0, v, log_events=True, **kw)


def test_python_gpu_loop_gives_the_recorded_run(ctx, oracle):
    want_kts, want_digest = KC.golden()
    _, K, p0, v = KC.stream()
    be = PL.GPUBackend(ctx)
    try:
        g = PL.WindowedStereoVO(C.loop_config(), be, K, p0, v, log_events=True, overlap=True)
        kts = KC.run_push(g)
    finally:
        be.close()
    assert kts == want_kts and KC.events_digest(g.events) == want_digest
    assert C.record_lines(g.kf_log) == C.golden_lines()
    o, _ = C.oracle_push()  # and the oracle backend still gives what was recorded
    assert C.record_lines(o.kf_log) == C.golden_lines()
    assert [(r["n_usable"], r["gap"]) for r in g.kf_log[1:]] == [(r["n_usable"], r["gap"]) for r in o.kf_log[1:]]
    for i in (0, 4, 12):
        for a, b in zip(g.frame_pose(i), o.frame_pose(i)):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)  # (the loops' bar on the keyframe pose underneath)


def test_native_loop_gives_the_recorded_run(ctx, oracle):
    want_kts, want_digest = KC.golden()
    g = native(ctx)
    try:
        kts = KC.run_push(g)
        assert kts == want_kts and KC.events_digest(g.events) == want_digest
        log = g.frame_pose_log
        assert C.record_lines(log) == C.golden_lines()
        assert [r["frame"] for r in log] == list(range(1, KC.N_FRAMES))
        assert [r["t"] for r in log] == want_kts[1:]
        o, _ = C.oracle_push()
        assert [(r["n_usable"], r["gap"]) for r in log] == [(r["n_usable"], r["gap"]) for r in o.kf_log[1:]]
        R0, t0, v0 = g.frame_pose(0)
        assert v0 == 1 and np.array_equal(t0, g.poses[0][:3])
        R, t, valid = g.frame_pose(12)
        assert valid == 1 and np.array_equal(R, log[11]["R_rel"] @ PL.aa_to_R(g.poses[1][3:]))
        assert np.array_equal(t, log[11]["R_rel"] @ g.poses[1][:3] + log[11]["t_rel"])
    finally:
        g.close()


def test_loops_with_the_switch_off_make_the_calls_they_made(ctx, oracle):
    """No me_frame_pose launch and a 32-byte read-back per frame, on both GPU loops."""
    want_kts, want_digest = KC.golden()
    _, K, p0, v = KC.stream()
    be = PL.GPUBackend(ctx)
    sizes = []
    try:
        be.tctx.timing(True, ["FRAMEPOSE", "KEYFRAME"])
        be.tctx.timing_reset()
        plain = be.tctx.copy_async

        def spy(dst, src, nbytes):
            sizes.append(int(nbytes))
            return plain(dst, src, nbytes)

        be.tctx.copy_async = spy
        g = PL.WindowedStereoVO(KC.loop_config(KeyframeSelect()), be, K, p0, v, log_events=True, overlap=True)
        kts = KC.run_push(g)
        be.tctx.synchronize()
        assert be.tctx.timing_read("FRAMEPOSE")[0] == 0
        assert be.tctx.timing_read("KEYFRAME")[0] == KC.N_FRAMES - 1
    finally:
        be.tctx.__dict__.pop("copy_async", None)
        be.tctx.timing(False)
        be.close()
    assert kts == want_kts and KC.events_digest(g.events) == want_digest
    assert sizes.count(32) >= KC.N_FRAMES - 1 and 160 not in sizes  # (one 32-byte read-back per frame, none of 160)
    assert all("t_ref" not in r for r in g.kf_log)
    from uasl_motion_estimation_amd._lib import Context

    t = Context(ctx.device)
    try:
        t.timing(True, ["FRAMEPOSE", "KEYFRAME"])
        n = PL.NativeStereoVO(KC.loop_config(KeyframeSelect()), ctx, K, p0, v, log_events=True, tctx=t)
        try:
            assert KC.run_push(n) == want_kts and KC.events_digest(n.events) == want_digest
            t.synchronize()
            assert t.timing_read("FRAMEPOSE")[0] == 0 and t.timing_read("KEYFRAME")[0] == KC.N_FRAMES - 1
            assert n.frame_pose_log == []
            with pytest.raises(ValueError, match="frame_pose"):
                n.frame_pose(1)
        finally:
            n.close()
        # and with it on, the family counts: six iteration launches and the final one per frame
        t.timing_reset()
        n = PL.NativeStereoVO(C.loop_config(), ctx, K, p0, v, log_events=True, tctx=t)
        try:
            KC.run_push(n)
            t.synchronize()
            assert t.timing_read("FRAMEPOSE")[0] == 7 * (KC.N_FRAMES - 1)
        finally:
            n.close()
    finally:
        t.timing(False)
        t.close()


def test_native_setter_rules(ctx):
    fr, K, p0, v = KC.stream()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        fc, kc = FramePose().to_c(), KeyframeSelect().to_c()
        assert g.lib.me_vo_loop_set_frame_pose(g.h, ctypes.byref(fc)) == -1  # before the keyframe switch
        assert b"me_vo_loop_set_keyframe_select" in g.lib.me_vo_loop_last_error(g.h)
        assert g.lib.me_vo_loop_set_frame_pose(g.h, None) == 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, ctypes.byref(kc)) == 0
        bad = FramePose().to_c()
        bad.iters = 17
        assert g.lib.me_vo_loop_set_frame_pose(g.h, ctypes.byref(bad)) == -1
        assert b"iters" in g.lib.me_vo_loop_last_error(g.h)
        assert g.lib.me_vo_loop_set_frame_pose(g.h, ctypes.byref(fc)) == 0
        assert g.lib.me_vo_loop_set_frame_pose(g.h, None) == 0
        assert g.lib.me_vo_loop_set_frame_pose(g.h, ctypes.byref(fc)) == 0
        kt = ctypes.c_int(7)
        L, R = np.ascontiguousarray(fr[0].left), np.ascontiguousarray(fr[0].right)
        assert g.lib.me_vo_loop_push(g.h, L.ctypes.data, R.ctypes.data, 0, ctypes.byref(kt)) == 0 and kt.value == 0
        assert g.lib.me_vo_loop_set_frame_pose(g.h, None) == -1  # after the first frame
        assert b"before the first frame" in g.lib.me_vo_loop_last_error(g.h)
        n = ctypes.c_int(-1)
        assert g.lib.me_vo_loop_frame_poses(g.h, None, 0, ctypes.byref(n)) == 0 and n.value == 0
        g.finish()
    finally:
        g.close()


def test_cpp_caller_prints_the_recorded_run(ctx, tmp_path):
    want_kts, _ = KC.golden()
    exe = C.build_cli(tmp_path)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(C.cli_input())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert [int(w) for w in lines[0].split()] == want_kts
    got = []
    for ln in lines[1:]:
        w = ln.split()
        got.append(" ".join(w[:5] + [float.fromhex(x).hex() for x in w[5:]]))
    assert got == C.golden_lines()
