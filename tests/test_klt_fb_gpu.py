"""Forward-backward KLT check on the device (me_klt_track_fb, csrc/klt.hip)
against its two-call oracle restatement (pipeline.klt_fb_host around
oracle/klt.cpp): positions, status and round-trip distance bit for bit, in
host and device memory mode; the loop switch klt_fb_max on the Python GPU loop
and the native loop against the oracle-backend loop.
"""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import klt_fb_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import ME_DEVICE, ME_HOST, MEError
from uasl_motion_estimation_amd.klt import calcOpticalFlowPyrLK, klt_params

pytestmark = pytest.mark.gpu
V = ctypes.c_void_p


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fb_device(ctx, prev, nxt, pts, fb_max, kp, stride=None, want_err=True):
    """me_klt_track_fb in ME_DEVICE mode on images of row stride `stride` (padding bytes 255)."""
    h, w = prev.shape
    stride = stride or w
    n = len(pts)
    bufs = []

    def dev(nbytes):
        bufs.append(ctx.malloc(max(nbytes, 16)))
        return bufs[-1]

    try:
        imgs = []
        for im in (prev, nxt):
            padded = np.full((h, stride), 255, np.uint8)
            padded[:, :w] = im
            d = dev(stride * h)
            ctx.h2d(d, padded)
            imgs.append(d)
        din, dout, dst, derr = dev(8 * n), dev(8 * n), dev(n), dev(4 * n)
        if n:
            ctx.h2d(din, np.ascontiguousarray(pts, np.float32))
        ctx.check(ctx.lib.me_klt_track_fb(ctx.h, ME_DEVICE, V(imgs[0]), V(imgs[1]), w, h, stride, V(din), V(dout),
                                          V(dst), V(derr) if want_err else None, n, ctypes.byref(kp), float(fb_max)),
                  "me_klt_track_fb")
        ctx.synchronize()
        out, st, err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        if n:
            ctx.d2h(out, dout)
            ctx.d2h(st, dst)
            if want_err:
                ctx.d2h(err, derr)
        return out, st, err
    finally:
        for b in bufs:
            ctx.free(b)


def check_against(ref, got):
    q, st, err = ref[:3]
    out, gst, gerr = got
    assert np.array_equal(bits(out), bits(q))
    assert np.array_equal(gst, st)
    assert np.array_equal(bits(gerr), bits(err))


@pytest.mark.parametrize("fb_max", [0.5, 1.0])
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_parity_host_and_device_mode(ctx, oracle, shape, fb_max):
    """The 8 x 8 grid of each pair: 64 features, and its first 63 (the last
    workgroup of four features is partly empty)."""
    w, h, win, lv = shape
    ref = C.oracle_fb(w, h, win, lv, fb_max)
    C.assert_classes_populated(*ref[1:])
    prev, nxt = C.image_pair(w, h)
    pts = C.grid_points(w, h, win)
    check_against(ref, calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, fb_max=fb_max, win=win, max_level=lv))
    kp = klt_params(win=win, max_level=lv)
    ref63 = tuple(a[:63] for a in ref[:3])
    check_against(ref63, fb_device(ctx, prev, nxt, pts[:63], fb_max, kp))
    check_against(ref63, calcOpticalFlowPyrLK(prev, nxt, pts[:63], ctx=ctx, fb_max=fb_max, win=win, max_level=lv))
    # the forward output is me_klt_track's own
    plain, pst = calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, win=win, max_level=lv)
    assert np.array_equal(bits(plain), bits(ref[0])) and np.array_equal(pst, ref[3])


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_parity_padded_rows_one_point_and_lost_points(ctx, oracle, shape):
    w, h, win, lv = shape
    prev, nxt = C.image_pair(w, h)
    grid = C.grid_points(w, h, win)
    kp = klt_params(win=win, max_level=lv)
    ref = C.oracle_fb(w, h, win, lv, 0.5)
    C.assert_classes_populated(*ref[1:])
    # device mode, rows padded by 13 bytes
    check_against(tuple(a[:63] for a in ref[:3]), fb_device(ctx, prev, nxt, grid[:63], 0.5, kp, stride=w + 13))
    # one point (an accepted one), both modes
    k = int(np.flatnonzero(ref[1] == 1)[0])
    one = tuple(a[k:k + 1] for a in ref[:3])
    check_against(one, fb_device(ctx, prev, nxt, grid[k:k + 1], 0.5, kp))
    check_against(one, calcOpticalFlowPyrLK(prev, nxt, grid[k:k + 1], ctx=ctx, fb_max=0.5, win=win, max_level=lv))
    # two points the forward pass loses (window outside the image), among the others
    pts = np.concatenate([grid[:30], np.array([[2, 2], [w - 1, h - 1]], np.float32), grid[30:]])
    ref2 = C.oracle_fb(w, h, win, lv, 0.5, pts=pts, key="lost")
    assert ref2[3][30] == 0 and ref2[3][31] == 0 and np.all(np.isinf(ref2[2][30:32])) and np.all(ref2[1][30:32] == 0)
    check_against(ref2, fb_device(ctx, prev, nxt, pts, 0.5, kp))
    check_against(ref2, calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, fb_max=0.5, win=win, max_level=lv))


def test_infinite_bound_accepts_every_feature_both_passes_tracked(ctx, oracle):
    w, h, win, lv = C.SHAPES[0]
    ref = C.oracle_fb(w, h, win, lv, math.inf)
    assert np.array_equal(ref[1], ((ref[3] == 1) & (ref[4] == 1)).astype(np.uint8))
    prev, nxt = C.image_pair(w, h)
    check_against(ref, calcOpticalFlowPyrLK(prev, nxt, C.grid_points(w, h, win), ctx=ctx, fb_max=math.inf, win=win,
                                            max_level=lv))


def test_null_fb_err_and_no_features(ctx, oracle):
    w, h, win, lv = C.SHAPES[0]
    prev, nxt = C.image_pair(w, h)
    pts = C.grid_points(w, h, win)
    kp = klt_params(win=win, max_level=lv)
    ref = C.oracle_fb(w, h, win, lv, 0.5)
    out, st, _ = fb_device(ctx, prev, nxt, pts, 0.5, kp, want_err=False)
    assert np.array_equal(st, ref[1]) and np.array_equal(bits(out), bits(ref[0]))
    # host mode, fb_err = NULL
    pts_c = np.ascontiguousarray(pts)
    out, st = np.zeros_like(pts_c), np.zeros(len(pts_c), np.uint8)
    ctx.check(ctx.lib.me_klt_track_fb(ctx.h, ME_HOST, prev.ctypes.data, nxt.ctypes.data, w, h, w, pts_c.ctypes.data,
                                      out.ctypes.data, st.ctypes.data, None, len(pts_c), ctypes.byref(kp), 0.5),
              "me_klt_track_fb")
    assert np.array_equal(st, ref[1]) and np.array_equal(bits(out), bits(ref[0]))
    # n = 0, both modes
    ctx.check(ctx.lib.me_klt_track_fb(ctx.h, ME_HOST, prev.ctypes.data, nxt.ctypes.data, w, h, w, None, None, None,
                                      None, 0, ctypes.byref(kp), 0.5), "me_klt_track_fb n = 0")
    out, st, err = fb_device(ctx, prev, nxt, pts[:0], 0.5, kp)
    assert out.shape == (0, 2) and len(st) == 0 and len(err) == 0


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan])
def test_rejects_a_bound_that_is_not_positive(ctx, oracle, bad):
    w, h, win, lv = C.SHAPES[2]
    prev, nxt = C.image_pair(w, h)
    pts = C.grid_points(w, h, win)
    with pytest.raises(MEError) as e:
        calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, fb_max=bad, win=win, max_level=lv)
    assert "fb_max" in str(e.value)
    # the context is untouched by the rejected call
    check_against(C.oracle_fb(w, h, win, lv, 0.5),
                  calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, fb_max=0.5, win=win, max_level=lv))


def test_identity_pair(ctx):
    img, pts = C.identity_case()
    out, st, err = calcOpticalFlowPyrLK(img, img, pts, ctx=ctx, fb_max=0.5)
    assert np.all(st == 1) and np.all(err == 0.0) and np.array_equal(bits(out), bits(pts))


def test_plain_call_after_the_check_reproduces_the_golden_result(ctx):
    """Both calls share the context's pyramid scratch: the plain call's result does not move."""
    import golden_io as G

    d = G.load("klt")
    out, st, err = calcOpticalFlowPyrLK(d["prev"], d["next"], d["pts"], ctx=ctx, fb_max=0.5)
    assert np.array_equal(out, d["out"]) and np.all(st <= d["status"])
    out, st = calcOpticalFlowPyrLK(d["prev"], d["next"], d["pts"], ctx=ctx)
    assert np.array_equal(out, d["out"]) and np.array_equal(st, d["status"])


# ------------------------------------------------------------------ the loops
def check_loop(g, o):
    from test_pipeline import _check_against_oracle  # the bar the loops are already held to (events exact, 1e-6)

    assert [r.n_tracked for r in g.results] == [r.n_tracked for r in o.results]
    _check_against_oracle(g, o, 4, C.N_KEYFRAMES)


def test_python_gpu_loop_with_the_check_matches_the_oracle_loop(ctx, oracle):
    o = C.oracle_loop(klt_fb_max=0.5)
    off = C.oracle_loop()
    assert o.results[1].n_tracked < off.results[1].n_tracked  # the check rejects something on this sequence
    _, K, p0, v, _ = C.sequence()
    be = PL.GPUBackend(ctx)
    try:
        g = C.run_loop(PL.WindowedStereoVO(C.loop_config(klt_fb_max=0.5), be, K, p0, v, log_events=True, overlap=True))
        assert be.klt_fb_max == 0.5
    finally:
        be.close()
    check_loop(g, o)


def test_native_loop_with_the_check_matches_the_oracle_loop(ctx, oracle):
    o = C.oracle_loop(klt_fb_max=0.5)
    _, K, p0, v, _ = C.sequence()
    g = PL.NativeStereoVO(C.loop_config(klt_fb_max=0.5), ctx, K, p0, v, log_events=True)
    try:
        C.run_loop(g)
        check_loop(g, o)
    finally:
        g.close()


def test_native_loop_rejects_a_bad_bound(ctx):
    _, K, p0, v, _ = C.sequence()
    cfg = C.loop_config()
    cfg.klt_fb_max = -1.0  # (past PipelineConfig's own check)
    with pytest.raises(MEError) as e:
        PL.NativeStereoVO(cfg, ctx, K, p0, v, overlap=False)  # (one context: nothing to undo after the refusal)
    assert "klt_fb_max" in str(e.value)


def test_cpp_overload_prints_the_python_result(ctx, tmp_path):
    w, h, win, lv = C.SHAPES[0]
    prev, nxt = C.image_pair(w, h)
    pts = C.grid_points(w, h, win)
    exe = C.build_cli(tmp_path)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([w, h, len(pts)], np.int32).tobytes())
        fh.write(np.array([0.5], np.float64).tobytes())
        fh.write(prev.tobytes())
        fh.write(nxt.tobytes())
        fh.write(pts.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out, st, err = calcOpticalFlowPyrLK(prev, nxt, pts, ctx=ctx, fb_max=0.5)  # (the overload's default parameters)
    want = ["%d %08x %08x %08x" % (st[i], bits(err)[i], bits(out)[i, 0], bits(out)[i, 1]) for i in range(len(pts))]
    assert r.stdout.split("\n")[:-1] == want
    assert 8 <= int(st.sum()) < len(pts)
