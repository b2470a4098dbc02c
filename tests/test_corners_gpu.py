"""GPU tests of the corner detector (csrc/corners.hip) against its numpy
restatement (uasl_motion_estimation_amd/corners.py): the response map and the
new features bit for bit, the chain into the reference's NMS primitive, the
agreement with the KLT's acceptance test, and the VO loops with
detector = "corners"."""
import ctypes
import functools

import numpy as np
import pytest

from uasl_motion_estimation_amd import corners as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import ME_DEVICE, ME_HOST, MEError, vptr

pytestmark = pytest.mark.gpu

SHAPES = [(21, 21, 21), (22, 22, 21), (23, 40, 21), (97, 61, 21), (200, 130, 7), (640, 480, 21)]
KINDS = ["noise", "stripes_x", "stripes_y", "diag", "antidiag", "zeros", "full"]


@functools.lru_cache(maxsize=None)
def image(kind, w, h):
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    if kind == "noise":
        img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w))
    elif kind == "stripes_x":      # 0, 0, 255, 255: |dx| = 4080 everywhere, A11 needs more than 32 bits
        img = (x // 2) % 2 * 255
    elif kind == "stripes_y":
        img = (y // 2) % 2 * 255
    elif kind == "diag":           # the two signs of A12
        img = ((x + y) // 2) % 2 * 255
    elif kind == "antidiag":
        img = ((x - y) // 2) % 2 * 255
    else:
        img = np.full((h, w), 0 if kind == "zeros" else 255)
    img = np.ascontiguousarray(img, np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def response_ref(kind, w, h, win):
    R = C.corner_response_ref(image(kind, w, h), win)
    R.setflags(write=False)
    return R


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("w,h,win", SHAPES)
def test_response_bit_equal_host_memory(ctx, w, h, win):
    for kind in KINDS:
        got = C.corner_response(image(kind, w, h), win, ctx)
        ref = response_ref(kind, w, h, win)
        assert np.array_equal(bits(got), bits(ref)), (kind, int((bits(got) != bits(ref)).sum()))
    if w >= 64:
        assert response_ref("stripes_x", w, h, win).max() == 0 and response_ref("noise", w, h, win).max() > 0


def _response_device(ctx, buf, w, h, stride, win, mem):
    p = C.corner_params(win)
    out = np.full((h, w), -1.0)
    if mem == ME_HOST:
        ctx.check(ctx.lib.me_corner_response(ctx.h, ME_HOST, vptr(buf), w, h, stride, ctypes.byref(p), vptr(out)),
                  "me_corner_response")
        return out
    d_img, d_out = ctx.malloc(buf.nbytes), ctx.malloc(out.nbytes)
    try:
        ctx.h2d(d_img, buf)
        ctx.check(ctx.lib.me_corner_response(ctx.h, ME_DEVICE, ctypes.c_void_p(d_img), w, h, stride, ctypes.byref(p),
                                             ctypes.c_void_p(d_out)), "me_corner_response")
        ctx.d2h(out, d_out)  # (synchronises the ctx stream)
    finally:
        ctx.free(d_img)
        ctx.free(d_out)
    return out


@pytest.mark.parametrize("mem", [ME_HOST, ME_DEVICE])
@pytest.mark.parametrize("w,h,win,pad", [(97, 61, 21, 3), (200, 130, 7, 0), (23, 40, 21, 3)])
def test_response_bit_equal_stride_and_device_memory(ctx, mem, w, h, win, pad):
    for kind in ("noise", "diag"):
        img = image(kind, w, h)
        buf = np.full((h, w + pad), 77, np.uint8)  # padding the kernel must not read as pixels
        buf[:, :w] = img
        got = _response_device(ctx, buf, w, h, w + pad, win, mem)
        assert np.array_equal(bits(got), bits(response_ref(kind, w, h, win))), kind


def test_response_feeds_the_reference_nms(ctx, oracle):
    from uasl_motion_estimation_amd.feature_types import nonMaxSupScanline3x3

    got, gmask = nonMaxSupScanline3x3(C.corner_response(image("noise", 97, 61), 21, ctx), ctx)
    ref, rmask = oracle.nms(response_ref("noise", 97, 61, 21))
    assert len(ref) > 0 and np.array_equal(got, ref) and np.array_equal(gmask, rmask)


# ---- me_vo_new_corners
def grid_of(w, h, n_feats):
    """WindowedStereoVO's grid: (margin, nx, ny, cw, ch)."""
    aw, ah = w - 2 * PL.MARGIN, h - 2 * PL.MARGIN
    nx = max(1, int(round(np.sqrt(n_feats * aw / ah))))
    ny = max(1, int(np.ceil(n_feats / nx)))
    return PL.MARGIN, nx, ny, aw / nx, ah / ny


GRIDS = {"640x480": (640, 480) + grid_of(640, 480, 200), "97x61": (97, 61, 12, 3, 2, 73 / 3, 37 / 2)}


@functools.lru_cache(maxsize=None)
def detector_image(name, kind):
    w, h = GRIDS[name][:2]
    if kind == "scene":
        if name == "640x480":
            return np.ascontiguousarray(PL.synthetic_sequence(1, 2)[0][0].left)
        return image("noise", w, h)
    if kind == "periodic":
        patch = np.random.default_rng(5).integers(0, 256, (16, 16), dtype=np.uint8)
        return np.ascontiguousarray(np.tile(patch, (h // 16 + 1, w // 16 + 1))[:h, :w])
    return image("full", w, h)


def tracked(name, case):
    w, h, margin, nx, ny, cw, ch = GRIDS[name]
    rng = np.random.default_rng(11)
    if case == "none":
        return None, None, None
    if case == "all_cells":  # one good feature in the middle of every cell
        cx, cy = np.meshgrid(np.arange(nx), np.arange(ny))
        uv = np.stack([margin + (cx.ravel() + 0.5) * cw, margin + (cy.ravel() + 0.5) * ch], -1).astype(np.float32)
        return uv, np.ones(len(uv), np.uint8), np.ones(len(uv), np.uint8)
    n = 3 * nx * ny // 4  # mixed: some lost, some unmatched, some outside the margin, one on the last pixel
    uv = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], -1).astype(np.float32)
    uv[0] = (margin, margin)
    uv[1] = (w - margin, h - margin)  # just outside
    uv[2] = (np.nextafter(np.float32(w - margin), np.float32(0)), margin)
    st, ok = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)
    st[:3], ok[:3] = 1, (1, 1, 2)  # the first and the third occupy the first row's end cells
    return uv, st, ok


CASES = [("scene", "none", 10 ** 6), ("scene", "all_cells", 10 ** 6), ("scene", "none", 7), ("scene", "mixed", 10 ** 6),
         ("scene", "mixed", 60), ("periodic", "none", 10 ** 6), ("periodic", "mixed", 10 ** 6),
         ("flat", "none", 10 ** 6)]


@pytest.mark.parametrize("name", list(GRIDS))
def test_new_corners_equal_the_restatement(ctx, name):
    w, h, margin, nx, ny, cw, ch = GRIDS[name]
    win = 21 if name == "640x480" else 7
    counts = {}
    for kind, case, n_feats in CASES:
        n_feats = min(n_feats, 4 * nx * ny)
        img = detector_image(name, kind)
        uv, st, ok = tracked(name, case)
        ref_uv, ref_lo = C.new_corners_ref(img, uv, st, ok, margin, nx, ny, cw, ch, n_feats, 2, win, 1e-4)
        got_uv, got_lo = C.new_corners(img, uv, st, ok, margin, nx, ny, cw, ch, n_feats, 2, win, 1e-4, ctx=ctx)
        assert got_uv.shape == ref_uv.shape, (kind, case, n_feats, got_uv.shape, ref_uv.shape)
        assert np.array_equal(bits(got_uv), bits(ref_uv)) and np.array_equal(got_lo, ref_lo), (kind, case, n_feats)
        counts[(kind, case, n_feats)] = len(ref_uv)
    # the cases are what they claim to be
    full = counts[("scene", "none", 4 * nx * ny)]
    assert full > nx * ny // 2 and counts[("scene", "all_cells", 4 * nx * ny)] == 0
    assert counts[("scene", "none", 7)] == min(7, full) and counts[("flat", "none", 4 * nx * ny)] == 0
    assert 0 < counts[("scene", "mixed", 4 * nx * ny)] < full
    assert counts[("periodic", "none", 4 * nx * ny)] > 0


def test_invalid_parameters_are_rejected(ctx):
    img = image("noise", 97, 61)
    out = np.zeros((61, 97))
    for win, me in [(20, 1e-4), (1, 1e-4), (33, 1e-4), (-3, 1e-4)]:
        p = C.corner_params(win, me)
        rc = ctx.lib.me_corner_response(ctx.h, ME_HOST, vptr(img), 97, 61, 97, ctypes.byref(p), vptr(out))
        assert rc == -1 and b"window" in ctx.lib.me_last_error(ctx.h)
    p = C.corner_params(21)
    assert ctx.lib.me_corner_response(ctx.h, ME_HOST, vptr(img), 97, 61, 90, ctypes.byref(p), vptr(out)) == -1
    assert (out == 0).all()  # nothing ran
    g = (12, 3, 2, 73 / 3, 37 / 2)
    for kw, word in [(dict(win=20), "window"), (dict(min_eig=0.0), "min_eig"), (dict(min_eig=-1.0), "min_eig")]:
        with pytest.raises(MEError) as e:
            C.new_corners(img, None, None, None, *g, 10, ctx=ctx, **kw)
        assert e.value.code == -1 and word in str(e.value)
    with pytest.raises(MEError) as e:  # 65 792 cells
        C.new_corners(img, None, None, None, 12, 256, 257, 0.1, 0.1, 10, ctx=ctx)
    assert e.value.code == -1 and "cells" in str(e.value)
    ctx.synchronize()


def test_emitted_corners_are_accepted_by_the_tracker(ctx):
    """R >= min_eig at an integer point is the KLT's own level-0 test (and implies its determinant
    test: D >= (441 * 1e-4)^2 > 1.19e-7), so tracking an image onto itself keeps every corner."""
    from uasl_motion_estimation_amd.klt import calcOpticalFlowPyrLK

    w, h, margin, nx, ny, cw, ch = GRIDS["640x480"]
    img = detector_image("640x480", "scene")
    uv, _ = C.new_corners(img, None, None, None, margin, nx, ny, cw, ch, 200, ctx=ctx)
    assert len(uv) > 100
    out, st = calcOpticalFlowPyrLK(img, img, uv, ctx=ctx)
    assert (st == 1).all() and np.array_equal(out, uv)


# ---- the loops, config 1 (640 x 480, 200 features, window 5), 6 keyframes
N_KF = 6


@pytest.fixture(scope="module")
def seq1():
    return PL.synthetic_sequence(1, N_KF)


def _cfg(**kw):
    return PL.PipelineConfig.from_config(1, ba_iters=5, **kw)


def _python_loop(seq, backend, overlap, **kw):
    fr, K, p0, v, truth = seq
    vo = PL.WindowedStereoVO(_cfg(**kw), backend, K, p0, v, log_events=True, overlap=overlap)
    for t in range(N_KF):
        vo.process(t, fr[t].left, fr[t].right)
    vo.finish()
    return vo


def _native_loop(ctx, seq, **kw):
    fr, K, p0, v, truth = seq
    vo = PL.NativeStereoVO(_cfg(**kw), ctx, K, p0, v, log_events=True)
    for t in range(N_KF):
        vo.process(t, fr[t].left, fr[t].right)
    vo.finish()
    return vo


@pytest.fixture(scope="module")
def gpu_corners_run(ctx, seq1):
    be = PL.GPUBackend(ctx)
    try:
        return _python_loop(seq1, be, True, detector="corners")
    finally:
        be.close()


def test_python_loop_with_corners_matches_the_oracle_backend(oracle, seq1, gpu_corners_run):
    from pipeline_oracle import OracleBackend

    g, o = gpu_corners_run, _python_loop(seq1, OracleBackend(), False, detector="corners")
    new = [e for e in o.events if e[0] == "new"]
    assert sum(1 for e in new if e[2] == 0) > o.cfg.n_feats / 2 and all(e[3][0] == int(e[3][0]) for e in new)
    assert g.events == o.events and np.array_equal(g.ids, o.ids)
    assert len(g.results) == len(o.results) == N_KF
    for rg, ro in zip(g.results, o.results):
        assert (rg.n_tracked, rg.n_new, rg.n_window_pts, rg.n_window_obs) == \
            (ro.n_tracked, ro.n_new, ro.n_window_pts, ro.n_window_obs)
    for t in g.poses:
        np.testing.assert_allclose(g.poses[t], o.poses[t], rtol=1e-6, atol=1e-9)


def test_native_loop_with_corners_matches_the_python_loop(ctx, seq1, gpu_corners_run):
    n = _native_loop(ctx, seq1, detector="corners")
    try:
        assert n.events == gpu_corners_run.events
    finally:
        n.close()


def test_native_loop_default_config_is_the_grid_detector(ctx, seq1):
    from uasl_motion_estimation_amd._lib import VOLoopConfigC

    c = VOLoopConfigC()
    ctx.lib.me_vo_loop_default_config(ctypes.byref(c))
    assert (c.detector, c.corner_win, c.corner_min_eig) == (0, 21, 1e-4)
    a, b = _native_loop(ctx, seq1), _native_loop(ctx, seq1, detector="grid")
    try:
        ea = a.event_records()
        assert len(ea) and np.array_equal(ea, b.event_records())
        assert any(float(r["feat"][0]) != int(r["feat"][0]) for r in ea[ea["kind"] == 0])  # jittered cell centres
    finally:
        a.close()
        b.close()
