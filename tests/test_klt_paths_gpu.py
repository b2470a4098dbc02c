"""klt_kernel (csrc/klt.hip) on the KLT path cases (tests/klt_paths_cases.py)
against oracle/klt.cpp: window sums past 2^31, the fourth bilinear weight of
-1, eigenvalue rejects, every window size, the iteration parameters' edges,
pyramids down to one pixel, positions that are not finite or out of range, and
partly filled workgroups.  Positions by bit pattern (NaN by isnan), status and
round-trip distance exactly: the tracker is bit-exact by construction, there
is no tolerance anywhere.  tests/test_klt_paths.py proves on the CPU that each
case reaches the path it is named for.
"""
import ctypes

import numpy as np
import pytest

import klt_paths_cases as C
from test_klt_guided_gpu import device_call
from uasl_motion_estimation_amd._lib import ME_HOST
from uasl_motion_estimation_amd.klt import calcOpticalFlowPyrLK, klt_params

pytestmark = pytest.mark.gpu


def host_call(ctx, c, pts, fb_max=None):
    return calcOpticalFlowPyrLK(c.prev, c.next, pts, ctx=ctx, fb_max=fb_max, **c.kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_parity_with_the_oracle(ctx, oracle, name):
    c = C.CASES[name]
    got = host_call(ctx, c, c.pts)
    C.assert_same(got, C.oracle_ref(name))
    if c.bad is not None:
        # the valid rows, workgroup neighbours of the bad ones: those of a call without the bad rows
        alone = host_call(ctx, c, c.pts[~c.bad])
        C.assert_same(alone, C.oracle_valid_only(name))
        C.assert_same((got[0][~c.bad], got[1][~c.bad]), alone)
        assert not got[1][c.bad].any() and C.same_positions(got[0][c.bad], c.pts[c.bad])


@pytest.mark.parametrize("name", C.FB_NAMES)
def test_forward_backward_parity_with_the_two_call_restatement(ctx, oracle, name):
    c = C.CASES[name]
    ref = C.oracle_fb_ref(name)
    C.assert_same(host_call(ctx, c, c.pts, C.FB_MAX), ref)
    if c.bad is not None:
        assert not ref[1][c.bad].any() and np.all(np.isposinf(ref[2][c.bad]))


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.kind(n) == "S"])
def test_S_device_mode_with_padded_rows(ctx, oracle, name):
    c = C.CASES[name]
    C.assert_same(device_call(ctx, c, c.pts, c.pts, stride=c.w + 13, plain=True), C.oracle_ref(name))


def test_N_device_mode_forward_backward(ctx, oracle):
    """The gated backward pass reads the forward pass's NaN / infinite results in device memory."""
    name = "N-win9-L3"
    c = C.CASES[name]
    C.assert_same(device_call(ctx, c, c.pts, c.pts, C.FB_MAX, stride=c.w + 13, plain=True), C.oracle_fb_ref(name))


@pytest.mark.parametrize("n", C.SMALL_N)
def test_small_n_on_the_plain_entry_point(ctx, oracle, n):
    """Four features per workgroup: n = 1, 2, 3, 5 leave the last one partly empty; n = 0 launches nothing."""
    c = C.CASES[C.SMALL_N_CASE]
    full = C.oracle_ref(C.SMALL_N_CASE)
    want = (full[0][:n], full[1][:n])
    got = host_call(ctx, c, c.pts[:n])
    assert got[0].shape == (n, 2) and got[1].shape == (n,)
    C.assert_same(got, want)
    C.assert_same(device_call(ctx, c, c.pts[:n], c.pts[:n], stride=c.w + 13, plain=True), want)
    if n == 0:  # no feature arrays at all
        kp = klt_params(**c.kw)
        ctx.check(ctx.lib.me_klt_track(ctx.h, ME_HOST, c.prev.ctypes.data, c.next.ctypes.data, c.w, c.h, c.w, None,
                                       None, None, 0, ctypes.byref(kp)), "me_klt_track n = 0")
        # and the context still tracks
        C.assert_same(host_call(ctx, c, c.pts), full)
