"""Rigid-motion gate on the device (include/me_hip.h A12h, csrc/motion_gate.hip):
ok_out, err_out and every word of the info block bit-exact against the numpy
restatement motion_gate.motion_gate_ref at the smallest shapes that can go
wrong, the argument checks, the loops with the gate on against the
oracle-backend loop, the gate left off, and the C++ caller.

A failing Cholesky pivot: the case "pivot" reaches it with a bound so small
(1e-30 px) that only the first point of the winner's own triple, which its
translation reproduces exactly, is an inlier: three Jacobian rows, a rank-3
normal matrix, and a pivot that is not > 0 in the restatement.  The pose the
refinement keeps is then the hypothesis' own.
"""
import ctypes
import dataclasses
import subprocess

import numpy as np
import pytest

import motion_gate_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import MEError
from uasl_motion_estimation_amd.motion_gate import (MotionGate, info_words, motion_gate, motion_gate_device,
                                                    motion_gate_ref)

pytestmark = pytest.mark.gpu

D = MotionGate()


def head(o, n):
    return C.Obs(o.prev[:n], o.cur[:n], o.status[:n], o.ok[:n], o.mover[:n])


def few_usable(n, keep):
    o = C.scene(n)
    st = np.zeros(n, np.uint8)
    st[:keep] = 1
    return C.Obs(o.prev, o.cur, st, o.ok, o.mover)


# name -> (observations, parameters, keyframe number, ok_out aliases ok)
CASES = {
    "n0": (lambda: head(C.scene(8), 0), D, 1, False),
    "n1": (lambda: head(C.scene(8), 1), D, 1, False),
    "n2": (lambda: head(C.scene(8), 2), D, 1, True),
    "n3": (lambda: head(C.scene(8, 0.0, 0.0), 3), MotionGate(min_inliers=3), 1, False),  # three features: one triangle
    "n63": (lambda: C.scene(63), D, 2, False),
    "n64": (lambda: C.scene(64), D, 2, True),
    "n65": (lambda: C.scene(65), D, 2, False),
    "n129": (lambda: C.mixed_flags(C.scene(129)), D, 2, True),
    "n257-hyp1": (lambda: C.scene(257, 0.0, 0.05), MotionGate(n_hyp=1), 4, False),
    "n257-hyp1024": (lambda: C.scene(257), MotionGate(n_hyp=1024), 4, True),
    "refine0": (lambda: C.scene(200), MotionGate(refine=0), 3, False),
    "refine8": (lambda: C.scene(200), MotionGate(refine=8), 3, True),
    "separate": (lambda: C.mixed_flags(C.scene(200)), D, 3, False),
    "aliased": (lambda: C.mixed_flags(C.scene(200)), D, 3, True),
    "behind": (C.behind, D, 3, False),
    "wrap-t": (lambda: C.scene(129), MotionGate(seed=0xFFFFFFFF), 2 ** 31 - 1, False),
    "wrap-seed": (lambda: C.scene(129), MotionGate(seed=0x9E3779B9), 0x7FFFFFF0, True),
    "abstain-usable": (lambda: few_usable(64, 2), D, 3, False),
    "abstain-void": (C.collinear, D, 3, True),
    "abstain-count": (lambda: C.scene(200), MotionGate(min_inliers=190), 3, False),
    "pivot": (lambda: C.scene(129), MotionGate(gate_max=1e-30, refine=3), 3, False),
    "gate-tight": (lambda: C.scene(129, 0.25, 0.0), MotionGate(gate_max=1e-3), 3, True),
}

_REF = {}


def reference(name):
    """(observations, ok, err, info) of the restatement, computed once per case."""
    if name not in _REF:
        make, p, t, _ = CASES[name]
        o = make()
        _REF[name] = (o,) + motion_gate_ref(*o.args, *C.CAM, t, p)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_device_gate_is_the_restatement_bit_for_bit(ctx, name):
    _, p, t, alias = CASES[name]
    o, ok, err, info = reference(name)
    gok, gerr, ginfo = motion_gate(*o.args, *C.CAM, t, p, ctx=ctx, alias=alias)
    print(name, {k: info[k] for k in ("n_usable", "n_valid", "winner", "n_inliers", "abstained")})
    assert np.array_equal(ginfo["words"], info_words(info)), (ginfo, info)
    assert np.array_equal(gok, ok)
    assert np.array_equal(gerr.view(np.uint32), err.view(np.uint32))


def test_the_cases_reach_what_they_are_for():
    """The restatement's own account of each case (no device): an input that
    stops exercising its branch fails here instead of hiding."""
    info = {k: reference(k)[3] for k in CASES}
    assert info["n0"]["n_usable"] == 0 and info["n0"]["abstained"] == 1
    assert info["n3"]["n_usable"] == 3 and info["n3"]["abstained"] == 0 and info["n3"]["n_inliers"] == 3
    for k in ("n63", "n64", "n65", "n129", "n257-hyp1024", "refine0", "refine8", "separate", "behind", "wrap-t",
              "wrap-seed", "gate-tight"):
        assert info[k]["abstained"] == 0, k
    assert info["n257-hyp1"]["n_valid"] == 1
    assert not np.array_equal(info["refine0"]["R"], info["refine8"]["R"])
    o, ok, err, _ = reference("separate")
    assert np.any(ok != o.ok) and np.any(ok == 2)
    o, ok, err, _ = reference("behind")
    usable = (o.cur[:, 0] >= C.MARGIN) & (o.cur[:, 0] < C.W - C.MARGIN) & (o.cur[:, 1] >= C.MARGIN) \
        & (o.cur[:, 1] < C.H - C.MARGIN)
    assert int((usable & np.isinf(err)).sum()) >= 5  # usable, Y_z <= 0 under the winner
    assert info["wrap-t"]["winner"] != info["n129"]["winner"] or info["wrap-t"]["n_valid"] != info["n129"]["n_valid"]
    assert (info["abstain-usable"]["n_usable"], info["abstain-usable"]["winner"]) == (2, -1)
    assert info["abstain-void"]["n_usable"] == 40 and info["abstain-void"]["n_valid"] == 0
    assert info["abstain-count"]["winner"] >= 0 and info["abstain-count"]["abstained"] == 1
    # the pivot case: a winner exists, one point is an inlier of it, so the normal matrix has rank 3, a pivot fails
    # and the pose is the hypothesis' own (refine = 0 gives the same words)
    assert info["pivot"]["winner"] >= 0 and info["pivot"]["n_inliers"] == 1
    o = reference("pivot")[0]
    same = motion_gate_ref(*o.args, *C.CAM, 3, MotionGate(gate_max=1e-30, refine=0))[2]
    assert np.array_equal(info_words(same), info_words(info["pivot"]))


def test_null_outputs_and_a_second_call_on_the_context(ctx):
    """err_out and info may be NULL; the scratch of one call does not leak into the next."""
    o, ok, _, _ = reference("separate")
    n = len(o.prev)
    parts = [np.ascontiguousarray(o.prev[:, :2]), np.ascontiguousarray(o.prev[:, 2]), np.ascontiguousarray(o.cur[:, :2]),
             np.ascontiguousarray(o.cur[:, 2]), o.status, o.ok]
    offs = np.cumsum([0] + [a.nbytes for a in parts])
    host = np.concatenate([a.view(np.uint8).ravel() for a in parts])
    d = ctx.malloc(host.nbytes)
    try:
        ctx.h2d(d, host)
        p = [int(d + x) for x in offs]
        motion_gate_device(ctx, D, p[0], p[1], p[2], p[3], p[4], p[5], n, *C.CAM, 3, p[5])
        ctx.synchronize()
        back = np.empty_like(host)
        ctx.d2h(back, d)
    finally:
        ctx.free(d)
    assert np.array_equal(back[offs[5]:], ok) and np.array_equal(back[:offs[5]], host[:offs[5]])
    for name in ("n64", "separate"):
        _, p_, t, alias = CASES[name]
        o2, ok2, err2, info2 = reference(name)
        g = motion_gate(*o2.args, *C.CAM, t, p_, ctx=ctx, alias=alias)
        assert np.array_equal(g[0], ok2) and np.array_equal(g[2]["words"], info_words(info2))


@pytest.mark.parametrize("field,bad", [("gate_max", 0.0), ("gate_max", float("nan")), ("min_disp", -1.0), ("n_hyp", 0),
                                       ("n_hyp", 1025), ("refine", 9), ("refine", -1), ("min_inliers", 2)])
def test_bad_parameters_are_invalid(ctx, field, bad):
    o = C.scene(64)
    p = MotionGate()
    object.__setattr__(p, field, bad)  # (past MotionGate's own check)
    with pytest.raises(MEError) as e:
        motion_gate(*o.args, *C.CAM, 1, p, ctx=ctx)
    assert e.value.code == -1 and field in str(e.value)


def test_bad_arguments_are_invalid_and_the_context_survives(ctx):
    o = C.scene(64)
    V = ctypes.c_void_p
    pc = D.to_c()
    one = ctx.malloc(4096)
    try:
        def call(n=64, f=C.F, b=C.B, t=1, null=None, info=one):
            a = [V(one)] * 6
            if null is not None:
                a[null] = None
            return ctx.lib.me_motion_gate(ctx.h, *a, n, f, C.CX, C.CY, b, C.W, C.H, C.MARGIN, t, ctypes.byref(pc),
                                          V(one), None, V(info))

        assert call(n=-1) == -1 and call(f=0.0) == -1 and call(b=float("nan")) == -1 and call(t=-1) == -1
        assert call(null=0) == -1 and call(null=5) == -1 and call(info=one + 4) == -1
        assert b"me_motion_gate" in ctx.lib.me_last_error(ctx.h)
        assert ctx.lib.me_motion_gate(ctx.h, *([V(one)] * 6), 8, C.F, C.CX, C.CY, C.B, C.W, C.H, C.MARGIN, 1, None,
                                      V(one), None, None) == -1
    finally:
        ctx.free(one)
    _, p, t, alias = CASES["n64"]
    o, ok, err, info = reference("n64")
    assert np.array_equal(motion_gate(*o.args, *C.CAM, t, p, ctx=ctx, alias=alias)[0], ok)


# ------------------------------------------------------------------ the loops
def check_loop(g, o):
    from test_pipeline import _check_against_oracle  # the bar the loops are already held to (events exact, 1e-6)

    assert [r.n_tracked for r in g.results] == [r.n_tracked for r in o.results]
    _check_against_oracle(g, o, 4, C.N_KEYFRAMES)


@pytest.mark.parametrize("on", [True, False], ids=["gate-on", "gate-off"])
def test_python_gpu_loop_matches_the_oracle_loop(ctx, oracle, on):
    gate = C.loop_gate() if on else None
    o, _ = C.oracle_loop(gate)
    if on:
        assert o.events != C.oracle_loop(None)[0].events and not C.rect_adds(o)  # the gate rejects something here
    _, K, p0, v = C.stream()
    be = PL.GPUBackend(ctx)
    try:
        g = C.run_loop(PL.WindowedStereoVO(C.loop_config(motion_gate=gate), be, K, p0, v, log_events=True, overlap=True))
    finally:
        be.close()
    check_loop(g, o)


@pytest.mark.parametrize("on", [True, False], ids=["gate-on", "gate-off"])
def test_native_loop_matches_the_oracle_loop(ctx, oracle, on):
    gate = C.loop_gate() if on else None
    o, _ = C.oracle_loop(gate)
    _, K, p0, v = C.stream()
    g = PL.NativeStereoVO(C.loop_config(motion_gate=gate), ctx, K, p0, v, log_events=True)
    try:
        C.run_loop(g)
        check_loop(g, o)
    finally:
        g.close()


def test_gate_left_off_events_are_the_parent_commit_s(ctx, oracle):
    """The events of the stream with the gate off, recorded on the oracle
    backend at the commit before the gate existed (tests/golden)."""
    import os

    want = open(os.path.join(os.path.dirname(__file__), "golden", "motion_gate_off_events.sha256")).read().split()[0]
    _, K, p0, v = C.stream()
    g = PL.NativeStereoVO(C.loop_config(), ctx, K, p0, v, log_events=True)
    try:
        C.run_loop(g)
        assert C.events_digest(g.events) == want
    finally:
        g.close()
    assert C.events_digest(C.oracle_loop(None)[0].events) == want


def test_native_setter_rules(ctx):
    fr, K, p0, v = C.stream()
    g = PL.NativeStereoVO(C.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        pc = D.to_c()
        assert g.lib.me_vo_loop_set_motion_gate(g.h, ctypes.byref(pc)) == 0  # before the first keyframe: any number
        assert g.lib.me_vo_loop_set_motion_gate(g.h, None) == 0              # of times, NULL switches it off
        bad = dataclasses.replace(D).to_c()
        bad.n_hyp = 0
        assert g.lib.me_vo_loop_set_motion_gate(g.h, ctypes.byref(bad)) == -1
        assert b"n_hyp" in g.lib.me_vo_loop_last_error(g.h)
        g.process(0, fr[0].left, fr[0].right)
        assert g.lib.me_vo_loop_set_motion_gate(g.h, ctypes.byref(pc)) == -5  # ME_ERR_STATE
        assert b"motion gate" in g.lib.me_vo_loop_last_error(g.h).replace(b"-", b" ")
        g.finish()
    finally:
        g.close()


def test_cpp_caller_prints_the_python_result(ctx, tmp_path):
    name = "n129"
    _, p, t, _ = CASES[name]
    o, ok, err, info = reference(name)
    exe = C.build_cli(tmp_path)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(C.cli_input(o, t, p))
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    gok, gerr, ginfo = motion_gate(*o.args, *C.CAM, t, p, ctx=ctx)
    assert [int(w, 16) for w in lines[0].split()] == [int(w) for w in ginfo["words"]]
    rows = [ln.split() for ln in lines[1:] if ln]
    assert [int(a) for a, _ in rows] == [int(x) for x in gok]
    assert [int(b, 16) for _, b in rows] == [int(x) for x in gerr.view(np.uint32)]
    assert np.array_equal(gok, ok)
