"""Keyframe selection on the device (include/me_hip.h A12i, csrc/keyframe.hip):
cur_uv, alive and all 32 info bytes of me_kf_update bit for bit against the
numpy restatement keyframe.kf_update_ref over the case table, the argument
checks, the push() loops against the oracle-backend run recorded in
tests/golden, and the C++ caller.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import keyframe_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import MEError
from uasl_motion_estimation_amd.keyframe import KeyframeSelect, info_bytes, kf_update, kf_update_ref

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """The restatement's (cur_uv, alive, info) of a case, computed once."""
    if name not in _REF:
        _REF[name] = kf_update_ref(*C.cases()[name].args)
    return _REF[name]


@pytest.mark.parametrize("name", list(C.cases()))
def test_device_update_is_the_restatement_bit_for_bit(ctx, name):
    c = C.cases()[name]
    cur, alive, info = reference(name)
    gcur, galive, ginfo = kf_update(*c.args, ctx=ctx)
    print(name, info)
    assert np.array_equal(ginfo["bytes"], info_bytes(info)), (ginfo, info)
    assert np.array_equal(gcur.view(np.uint32), cur.view(np.uint32))
    assert np.array_equal(galive, alive)


def test_a_second_call_carries_the_state_on(ctx):
    """Two updates in a row on the device against two of the restatement: what the first left is what the second reads."""
    c = C.cases()["general-n1025"]
    cur1, alive1, _ = reference("general-n1025")
    new2 = (cur1 + np.float32(1.5)).astype(np.float32)
    st2 = np.ones(len(cur1), np.uint8)
    want = kf_update_ref(c.ref, cur1, alive1, new2, st2, C.W, C.H, C.MARGIN, 2, c.params)
    g1 = kf_update(*c.args, ctx=ctx)
    got = kf_update(c.ref, g1[0], g1[1], new2, st2, C.W, C.H, C.MARGIN, 2, c.params, ctx=ctx)
    assert np.array_equal(got[2]["bytes"], info_bytes(want[2]))
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("field,bad", [("min_parallax", -1.0), ("min_parallax", float("nan")),
                                       ("min_parallax", float("inf")), ("min_tracked_pct", -1),
                                       ("min_tracked_pct", 101), ("max_gap", 0)])
def test_bad_parameters_are_invalid(ctx, field, bad):
    c = C.cases()["general-n64"]
    p = KeyframeSelect()
    object.__setattr__(p, field, bad)  # (past KeyframeSelect's own check)
    with pytest.raises(MEError) as e:
        kf_update(*c.args[:9], p, ctx=ctx)
    assert e.value.code == -1 and field in str(e.value)


def test_bad_arguments_are_invalid_and_the_context_survives(ctx):
    V = ctypes.c_void_p
    pc = KeyframeSelect().to_c()
    one = ctx.malloc(4096)
    try:
        def call(n=64, gap=1, null=None, info=one, params=ctypes.byref(pc)):
            a = [V(one)] * 5
            if null is not None:
                a[null] = None
            rc = ctx.lib.me_kf_update(ctx.h, *a, n, C.W, C.H, C.MARGIN, gap, params, V(info) if info else None)
            return rc, ctx.lib.me_last_error(ctx.h)

        for kw, word in ((dict(n=-1), b"n must"), (dict(gap=0), b"gap"), (dict(null=0), b"null feature array"),
                         (dict(null=2), b"null feature array"), (dict(null=4), b"null feature array"),
                         (dict(info=0), b"null info"), (dict(params=None), b"null params")):
            rc, msg = call(**kw)
            assert rc == -1 and b"me_kf_update" in msg and word in msg, (kw, msg)
        # n = 0 with null arrays is legal
        assert ctx.lib.me_kf_update(ctx.h, None, None, None, None, None, 0, C.W, C.H, C.MARGIN, 1, ctypes.byref(pc),
                                    V(one)) == 0
        ctx.synchronize()
    finally:
        ctx.free(one)
    c = C.cases()["general-n64"]
    assert np.array_equal(kf_update(*c.args, ctx=ctx)[2]["bytes"], info_bytes(reference("general-n64")[2]))


# ------------------------------------------------------------------ the loops
def native(select, **kw):
    _, K, p0, v = C.stream()
    return PL.NativeStereoVO(C.loop_config(select), kw.pop("ctx"), K, p0, v, log_events=True, **kw)


def test_python_gpu_loop_gives_the_recorded_run(ctx, oracle):
    want_kts, want_digest = C.golden()
    _, K, p0, v = C.stream()
    be = PL.GPUBackend(ctx)
    try:
        g = PL.WindowedStereoVO(C.loop_config(KeyframeSelect()), be, K, p0, v, log_events=True, overlap=True)
        kts = C.run_push(g)
    finally:
        be.close()
    assert kts == want_kts and C.events_digest(g.events) == want_digest
    o, okts = C.oracle_push(KeyframeSelect())  # and the oracle backend still gives what was recorded
    assert okts == want_kts and C.events_digest(o.events) == want_digest
    assert [(r["flags"], r["m"], r["n"], r["med2"]) for r in g.kf_log] == \
        [(r["flags"], r["m"], r["n"], r["med2"]) for r in o.kf_log]


def test_native_loop_gives_the_recorded_run(ctx, oracle):
    want_kts, want_digest = C.golden()
    g = native(KeyframeSelect(), ctx=ctx)
    try:
        kts = C.run_push(g)
        assert kts == want_kts and C.events_digest(g.events) == want_digest
    finally:
        g.close()


def test_gap_rule_alone_on_both_gpu_loops(ctx, oracle):
    """Guided keyframes (every third frame): both GPU loops against the oracle-backend loop."""
    sel = KeyframeSelect(min_parallax=0.0, min_tracked_pct=0, max_gap=3)
    o, okts = C.oracle_push(sel)
    g = native(sel, ctx=ctx)
    try:
        assert C.run_push(g) == okts and g.events == o.events
    finally:
        g.close()
    _, K, p0, v = C.stream()
    be = PL.GPUBackend(ctx)
    try:
        w = PL.WindowedStereoVO(C.loop_config(sel), be, K, p0, v, log_events=True, overlap=True)
        assert C.run_push(w) == okts and w.events == o.events
    finally:
        be.close()


def test_native_push_with_max_gap_one_is_native_process(ctx):
    g = native(KeyframeSelect(max_gap=1), ctx=ctx)
    try:
        assert C.run_push(g) == list(range(C.N_FRAMES))
        ev, poses = g.events, [r.pose for r in g.results]
    finally:
        g.close()
    p = native(None, ctx=ctx)
    try:
        C.run_process(p, range(C.N_FRAMES))
        assert p.events == ev
        for a, b in zip(poses, [r.pose for r in p.results]):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)  # (the loops' bar: test_pipeline._check_against_oracle)
    finally:
        p.close()


def test_native_setter_and_entry_rules(ctx):
    fr, K, p0, v = C.stream()
    g = PL.NativeStereoVO(C.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        kt = ctypes.c_int(7)
        L, R = np.ascontiguousarray(fr[0].left), np.ascontiguousarray(fr[0].right)
        assert g.lib.me_vo_loop_push(g.h, L.ctypes.data, R.ctypes.data, 0, ctypes.byref(kt)) == -5  # switch off
        assert b"me_vo_loop_set_keyframe_select" in g.lib.me_vo_loop_last_error(g.h) and kt.value == -1
        pc = KeyframeSelect().to_c()
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, ctypes.byref(pc)) == 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, None) == 0
        bad = KeyframeSelect().to_c()
        bad.max_gap = 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, ctypes.byref(bad)) == -1
        assert b"max_gap" in g.lib.me_vo_loop_last_error(g.h)
        from uasl_motion_estimation_amd.tonemap import ToneMap

        tm = ToneMap().to_c()
        assert g.lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(tm)) == 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, ctypes.byref(pc)) == -1  # together with the tone map
        assert b"tone map" in g.lib.me_vo_loop_last_error(g.h)
        assert g.lib.me_vo_loop_set_tonemap(g.h, None) == 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, ctypes.byref(pc)) == 0
        assert g.lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(tm)) == -1
        assert g.lib.me_vo_loop_push(g.h, L.ctypes.data, R.ctypes.data, 0, ctypes.byref(kt)) == 0 and kt.value == 0
        assert g.lib.me_vo_loop_set_keyframe_select(g.h, None) == -5  # after the first frame
        assert g.lib.me_vo_loop_process(g.h, 1, L.ctypes.data, R.ctypes.data, 0) == -5  # push and process do not mix
        g.finish()
    finally:
        g.close()
    with pytest.raises(ValueError, match="keyframe_select"):
        PL.NativeStereoVO(C.loop_config(), ctx, K, p0, v, overlap=False).push(fr[0].left, fr[0].right)


# ------------------------------------------------------------------ push() behind the rectifier and CLAHE
PUSH_SELECT = KeyframeSelect(min_parallax=0.0, min_tracked_pct=0, max_gap=3)
_CHAIN = {}


def chain_config(rectify):
    """The stream's loop with CLAHE and the gap rule, and the cropping rectifier of padded frames when asked for."""
    import rectify_cases as RC
    from uasl_motion_estimation_amd.equalise import Clahe

    kw = dict(rectify=RC.padded_rectifier(C.SW, C.SH, C.stream()[1])) if rectify else {}
    return C.loop_config(PUSH_SELECT, equalise=Clahe(), **kw)


def chain_frames(rectify):
    """The stream as 16-level frames whose level drifts (equalise_cases.low_frame), padded for the rectifier."""
    import equalise_cases as EC
    import rectify_cases as RC

    out = [(EC.low_frame(f.left, i), EC.low_frame(f.right, i)) for i, f in enumerate(C.stream()[0])]
    return [(RC.pad_frame(L), RC.pad_frame(R)) for L, R in out] if rectify else out


def chain_oracle(rectify):
    """(loop, keyframe index per frame) of push() on the oracle backend with the same switches, computed once.
    Guarded: the run has guided keyframes that track, so a loop that equals it has run the whole chain."""
    from pipeline_oracle import OracleBackend

    if rectify not in _CHAIN:
        _, K, p0, v = C.stream()
        vo = PL.WindowedStereoVO(chain_config(rectify), OracleBackend(), K, p0, v, log_events=True)
        kts = [vo.push(L, R) for L, R in chain_frames(rectify)]
        vo.finish()
        assert sum(bool(r["guided"]) for r in vo.kf_log) >= 4
        assert len(vo.results) >= 5 and all(r.n_tracked >= 20 for r in vo.results[1:])
        _CHAIN[rectify] = (vo, kts)
    return _CHAIN[rectify]


def check_chain(g, kts, rectify):
    o, okts = chain_oracle(rectify)
    print(kts, [r.n_tracked for r in g.results], len(g.events))
    assert kts == okts and g.events == o.events
    assert len(g.results) == len(o.results)
    for a, b in zip(g.results, o.results):
        np.testing.assert_allclose(a.pose, b.pose, rtol=0, atol=1e-6)  # (the loops' bar, as above)


def test_oracle_push_chain_is_the_same_with_and_without_the_rectifier(oracle):
    (a, ka), (b, kb) = chain_oracle(False), chain_oracle(True)
    assert ka == kb and a.events == b.events


@pytest.mark.parametrize("rectify,tensors", [(True, False), (True, True), (False, True)],
                         ids=["rectify-equalise-host", "rectify-equalise-tensors", "equalise-tensors"])
def test_native_push_behind_the_front_end_chain(ctx, oracle, rectify, tensors):
    """me_vo_loop_push with the rectifier and CLAHE on, from host arrays and from the caller's device tensors
    (remap into the loop's pair, CLAHE in place; without the rectifier CLAHE out of place from the caller's
    images): the oracle-backend run's keyframes, events and poses, and the caller's tensors come back unchanged."""
    import torch

    _, K, p0, v = C.stream()
    frames = chain_frames(rectify)
    fed = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in frames] if tensors else frames
    g = PL.NativeStereoVO(chain_config(rectify), ctx, K, p0, v, log_events=True)
    try:
        kts = [g.push(L, R) for L, R in fed]
        g.finish()
        check_chain(g, kts, rectify)
    finally:
        g.close()
    if tensors:
        torch.cuda.synchronize()
        for (dL, dR), (L, R) in zip(fed, frames):
            assert np.array_equal(dL.cpu().numpy(), L) and np.array_equal(dR.cpu().numpy(), R)


def test_python_gpu_push_behind_the_front_end_chain(ctx, oracle):
    _, K, p0, v = C.stream()
    be = PL.GPUBackend(ctx)
    try:
        g = PL.WindowedStereoVO(chain_config(True), be, K, p0, v, log_events=True, overlap=True)
        kts = [g.push(L, R) for L, R in chain_frames(True)]
        g.finish()
        check_chain(g, kts, True)
    finally:
        be.close()


def test_cpp_caller_prints_the_recorded_keyframes(ctx, tmp_path):
    want_kts, _ = C.golden()
    exe = C.build_cli(tmp_path)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(C.cli_input(KeyframeSelect()))
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(w) for w in r.stdout.split()] == want_kts
