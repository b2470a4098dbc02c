"""Left-right consistency check of the epipolar MI matcher on the device
(me_mi_epipolar_match_lr / _lr_count, csrc/mi.hip) against its numpy
restatement (pipeline.match_lr_host around oracle/mi.cpp): xr bit for bit for
every feature match_host accepts (the bar of the plain matcher's test), ok and
lr_err for every feature; the loop switch match_lr_max on the Python GPU loop
and the native loop against the oracle-backend loop.
"""
import ctypes
import math

import numpy as np
import pytest

import klt_fb_cases as KC
import match_lr_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import MEError

pytestmark = pytest.mark.gpu
V = ctypes.c_void_p
SENTINEL = 0x7f  # output bytes the call must leave alone


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lr_device(ctx, w, h, patch, uv, lo, nd=C.ND, unique=False, d_max=C.D_MAX, lr_max=C.LR_MAX, valid=None, status=None,
              stride=None, want_err=True, count=None, plain=False):
    """me_mi_epipolar_match_lr on the pair (w, h) with rows of `stride` bytes
    (padding 255); count: the _count form over a device count (n = n_max);
    plain: me_mi_epipolar_match instead.  Returns (xr, ok, lr_err)."""
    L, R = C.image_pair(w, h)
    stride = stride or w
    n = len(uv)
    bufs = []

    def dev(a=None, nbytes=0):
        a = None if a is None else np.ascontiguousarray(a)
        bufs.append(ctx.malloc(max(a.nbytes if a is not None else nbytes, 16)))
        if a is not None and a.nbytes:
            ctx.h2d(bufs[-1], a)
        return bufs[-1]

    try:
        imgs = []
        for im in (L, R):
            padded = np.full((h, stride), 255, np.uint8)
            padded[:, :w] = im
            imgs.append(dev(padded))
        duv = dev(np.asarray(uv, np.float32))
        dlo = dev(np.asarray(lo, np.int32))
        dval = dev(np.asarray(valid, np.uint8)) if valid is not None else None
        dst = dev(np.asarray(status, np.uint8)) if status is not None else None
        dxr = dev(np.full(n, SENTINEL, np.uint8).repeat(4))
        dok = dev(np.full(n, SENTINEL, np.uint8))
        derr = dev(np.full(n, SENTINEL, np.uint8).repeat(4))
        lib = ctx.lib
        if plain:
            rc = lib.me_mi_epipolar_match(ctx.h, V(imgs[0]), V(imgs[1]), w, h, stride, V(duv), V(dlo), V(dval), V(dst),
                                          n, nd, patch, d_max, int(unique), 1.2, float(C.MARGIN), V(dxr), V(dok))
        elif count is not None:
            dcnt = dev(np.array([count, 0, 0, 0], np.int32))
            rc = lib.me_mi_epipolar_match_lr_count(ctx.h, V(imgs[0]), V(imgs[1]), w, h, stride, V(duv), V(dlo),
                                                   V(dcnt), n, nd, patch, d_max, int(unique), 1.2, float(C.MARGIN),
                                                   float(lr_max), V(dxr), V(dok), V(derr) if want_err else None)
        else:
            rc = lib.me_mi_epipolar_match_lr(ctx.h, V(imgs[0]), V(imgs[1]), w, h, stride, V(duv), V(dlo), V(dval),
                                             V(dst), n, nd, patch, d_max, int(unique), 1.2, float(C.MARGIN),
                                             float(lr_max), V(dxr), V(dok), V(derr) if want_err else None)
        ctx.check(rc, "me_mi_epipolar_match_lr")
        ctx.synchronize()
        xr, ok, err = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        if n:
            ctx.d2h(xr, dxr)
            ctx.d2h(ok, dok)
            ctx.d2h(err, derr)
        return xr, ok, err
    finally:
        for b in bufs:
            ctx.free(b)


def check_against(ref, got, want_err=True):
    xr, ok, err, ok_f, _ = ref
    gxr, gok, gerr = got
    assert np.array_equal(gok, ok.astype(np.uint8))
    assert np.array_equal(bits(gxr)[ok_f], bits(xr)[ok_f])
    if want_err:
        assert np.array_equal(bits(gerr), bits(err))
    else:
        assert np.all(gerr.view(np.uint8) == SENTINEL)


def prefix(ref, n):
    return tuple(a[:n] for a in ref)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d-p%d" % s)
def test_parity_on_the_occluded_striped_pair(ctx, oracle, shape):
    """80 features (five whole 16-pair waves of candidates per 13), 79 and one."""
    w, h, patch = shape
    ref = C.oracle_lr(*shape)
    C.assert_classes_populated(ref)
    uv = C.features(w, h)
    lo = np.full(len(uv), C.LO)
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo))
    check_against(prefix(ref, 79), lr_device(ctx, w, h, patch, uv[:79], lo[:79]))
    k = int(np.flatnonzero(ref[1])[0])  # an accepted feature
    check_against(tuple(a[k:k + 1] for a in ref), lr_device(ctx, w, h, patch, uv[k:k + 1], lo[k:k + 1]))
    j = int(np.flatnonzero(ref[3] & ~ref[1])[0])  # one the check rejects
    check_against(tuple(a[j:j + 1] for a in ref), lr_device(ctx, w, h, patch, uv[j:j + 1], lo[j:j + 1]))


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d-p%d" % s)
def test_parity_padded_rows_null_lr_err_and_infinite_bound(ctx, oracle, shape):
    w, h, patch = shape
    ref = C.oracle_lr(*shape)
    C.assert_classes_populated(ref)
    uv = C.features(w, h)
    lo = np.full(len(uv), C.LO)
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo, stride=w + 13))
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo, want_err=False), want_err=False)
    inf = C.oracle_lr(*shape, lr_max=math.inf)
    assert np.array_equal(inf[1], inf[3] & inf[4])
    check_against(inf, lr_device(ctx, w, h, patch, uv, lo, lr_max=math.inf))


@pytest.mark.parametrize("shape", [C.SHAPES[0], C.SHAPES[2]], ids=lambda s: "%dx%d-p%d" % s)
def test_parity_small_d_max(ctx, oracle, shape):
    """d_max = 14: the upper candidates are -inf in both passes."""
    w, h, patch = shape
    ref = C.oracle_lr(*shape, d_max=14)
    if shape == C.SHAPES[0]:
        assert C.classes(*ref)[1:3] == (59, 10)
    uv = C.features(w, h)
    check_against(ref, lr_device(ctx, w, h, patch, uv, np.full(len(uv), C.LO), d_max=14))


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d-p%d" % s)
def test_parity_per_feature_windows_validity_and_status(ctx, oracle, shape):
    w, h, patch = shape
    rng = np.random.default_rng(5)
    uv = C.features(w, h)
    n = len(uv)
    lo = rng.choice([2, 4, 8], n)
    valid = rng.random(n) > 0.1
    assert 0 < (~valid).sum() < n // 4
    ref = C.oracle_lr(*shape, lo=lo, dvalid=valid, key="lo248-valid")
    assert C.classes(*ref)[1] >= 8 and C.classes(*ref)[2] >= 4
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo, valid=valid))
    # the KLT gate: status 1 and inside the margin (the eight border features are outside it)
    status = (rng.random(n) > 0.15).astype(np.uint8)
    status[3] = 2  # (any value but 1 fails)
    gate = valid & (status == 1) & PL.in_margin(uv, w, h)
    assert not gate[72:].any() and 0 < (status[:72] != 1).sum()
    ref = C.oracle_lr(*shape, lo=lo, dvalid=gate, key="lo248-valid-status")
    assert C.classes(*ref)[1] >= 8
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo, valid=valid, status=status))


def test_no_features(ctx):
    xr, ok, err = lr_device(ctx, 96, 64, 11, np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    assert len(xr) == 0 and len(ok) == 0 and len(err) == 0


@pytest.mark.parametrize("shape", [C.SHAPES[1], C.SHAPES[2]], ids=lambda s: "%dx%d-p%d" % s)
def test_count_form_stops_at_the_device_count(ctx, oracle, shape):
    w, h, patch = shape
    ref = C.oracle_lr(*shape)
    uv = C.features(w, h)
    lo = np.full(len(uv), C.LO)
    k = 50
    xr, ok, err = lr_device(ctx, w, h, patch, uv, lo, count=k)
    check_against(prefix(ref, k), (xr[:k], ok[:k], err[:k]))
    assert C.classes(*prefix(ref, k))[2] >= 1
    for a in (xr[k:], ok[k:], err[k:]):
        assert np.all(a.view(np.uint8) == SENTINEL)
    # a count above n_max is clamped
    check_against(ref, lr_device(ctx, w, h, patch, uv, lo, count=len(uv) + 7))


@pytest.mark.parametrize("shape,accepted", [(C.SHAPES[0], 43), (C.SHAPES[1], 31)], ids=["160x120", "96x64"])
def test_parity_with_the_uniqueness_test(ctx, oracle, shape, accepted):
    """lo = 2, nd = 31, unique = 1: the ratio test leaves the check nothing to reject; bits only."""
    w, h, patch = shape
    ref = C.oracle_lr(*shape, lo=2, nd=31, unique=True)
    assert C.classes(*ref) == (accepted, accepted, 0, 0)
    uv = C.features(w, h)
    check_against(ref, lr_device(ctx, w, h, patch, uv, np.full(len(uv), 2), nd=31, unique=True))


def test_lane_kernel_path(ctx, oracle):
    """Test hook me_debug_solve_flags bit 32768: both scoring passes on mi_lane_kernel."""
    shape = C.SHAPES[1]
    w, h, patch = shape
    ref = C.oracle_lr(*shape)
    C.assert_classes_populated(ref)
    uv = C.features(w, h)
    hook = ctx.lib.me_debug_solve_flags
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hook(ctx.h, 32768) == 0
    try:
        check_against(ref, lr_device(ctx, w, h, patch, uv, np.full(len(uv), C.LO)))
        check_against(prefix(ref, 79), lr_device(ctx, w, h, patch, uv[:79], np.full(79, C.LO), stride=w + 13))
    finally:
        assert hook(ctx.h, 0) == 0


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan])
def test_rejects_a_bound_that_is_not_positive(ctx, oracle, bad):
    shape = C.SHAPES[1]
    w, h, patch = shape
    uv = C.features(w, h)
    lo = np.full(len(uv), C.LO)
    with pytest.raises(MEError) as e:
        lr_device(ctx, w, h, patch, uv, lo, lr_max=bad)
    assert "lr_max" in str(e.value)
    with pytest.raises(MEError) as e:
        lr_device(ctx, w, h, patch, uv, lo, lr_max=bad, count=10)
    assert "lr_max" in str(e.value)
    # the context is still usable
    check_against(C.oracle_lr(*shape), lr_device(ctx, w, h, patch, uv, lo))


@pytest.mark.parametrize("shape", C.SHAPES[:2], ids=lambda s: "%dx%d" % s[:2])
def test_plain_call_after_the_check_is_match_host(ctx, oracle, shape):
    """Both calls share the context's score scratch: the plain call's result does not move."""
    w, h, patch = shape
    uv = C.features(w, h)
    lo = np.full(len(uv), C.LO)
    check_against(C.oracle_lr(*shape), lr_device(ctx, w, h, patch, uv, lo))
    pxr, pok = C.oracle_plain(*shape)
    xr, ok, err = lr_device(ctx, w, h, patch, uv, lo, plain=True)
    assert np.array_equal(ok, pok.astype(np.uint8)) and np.array_equal(bits(xr)[pok], bits(pxr)[pok])
    assert pok.sum() == C.COUNTS[shape][0] and np.all(err.view(np.uint8) == SENTINEL)


# ------------------------------------------------------------------ the loops
def check_loop(g, o):
    from test_pipeline import _check_against_oracle  # the bar the loops are already held to (events exact, 1e-6)

    assert [r.n_tracked for r in g.results] == [r.n_tracked for r in o.results]
    _check_against_oracle(g, o, 4, KC.N_KEYFRAMES)


def test_python_gpu_loop_with_the_check_matches_the_oracle_loop(ctx, oracle):
    o = KC.oracle_loop(match_lr_max=1.0)
    off = KC.oracle_loop()
    assert 0 < o.results[1].n_tracked < off.results[1].n_tracked  # the check rejects something on this sequence
    _, K, p0, v, _ = KC.sequence()
    be = PL.GPUBackend(ctx)
    try:
        g = KC.run_loop(PL.WindowedStereoVO(KC.loop_config(match_lr_max=1.0), be, K, p0, v, log_events=True,
                                            overlap=True))
        assert be.match_lr_max == 1.0
    finally:
        be.close()
    check_loop(g, o)


def test_native_loop_with_the_check_matches_the_oracle_loop(ctx, oracle):
    o = KC.oracle_loop(match_lr_max=1.0)
    _, K, p0, v, _ = KC.sequence()
    g = PL.NativeStereoVO(KC.loop_config(match_lr_max=1.0), ctx, K, p0, v, log_events=True)
    try:
        KC.run_loop(g)
        check_loop(g, o)
    finally:
        g.close()


def test_native_setter_after_the_first_keyframe_is_a_state_error(ctx):
    fr, K, p0, v, _ = KC.sequence()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        assert g.lib.me_vo_loop_set_match_lr(g.h, 0.5) == 0  # before the first keyframe: any number of times
        assert g.lib.me_vo_loop_set_match_lr(g.h, 0.0) == 0
        g.process(0, fr[0].left, fr[0].right)
        assert g.lib.me_vo_loop_set_match_lr(g.h, 1.0) == -5  # ME_ERR_STATE
        assert b"match_lr_max" in g.lib.me_vo_loop_last_error(g.h)
        g.finish()
    finally:
        g.close()


@pytest.mark.parametrize("bad", [-1.0, math.nan])
def test_native_loop_rejects_a_bad_bound(ctx, bad):
    _, K, p0, v, _ = KC.sequence()
    cfg = KC.loop_config()
    cfg.match_lr_max = bad  # (past PipelineConfig's own check)
    with pytest.raises(MEError) as e:
        PL.NativeStereoVO(cfg, ctx, K, p0, v, overlap=False)
    assert "match_lr_max" in str(e.value)
