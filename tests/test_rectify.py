"""Stereo rectification (include/me_hip.h, section A12d), the parts that need
no GPU: the numpy restatement (rectify.rectify_map_ref / remap_ref) against
closed forms and against exact rational arithmetic, the argument checks, the
configuration switch on the oracle backend.  The device side is
tests/test_rectify_gpu.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import klt_fb_cases as KC
import rectify_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.rectify import (SENTINEL, CameraModel, RectifiedModel, StereoRectifier,
                                                rectify_map_ref, remap_ref)

BORDERS = [0, 255, 77]


# ------------------------------------------------------------------ 1. remap_ref
def test_identity_map_returns_the_source():
    for img in (C.noise(17, 9), C.checker(17, 9), C.noise(1, 1)):
        h, w = img.shape
        assert np.array_equal(remap_ref(img, C.identity_map(w, h), 5), img)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("dx,dy", [(3, 0), (-3, 0), (0, 2), (0, -2), (2, -1)])
def test_integer_shift_exposes_the_border(dx, dy, border):
    img = C.noise(17, 9)
    h, w = img.shape
    want = np.full((h, w), border, np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    ok = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
    want[ok] = img[(ys + dy)[ok], (xs + dx)[ok]]
    got = remap_ref(img, C.shift_map(w, h, dx, dy), border)
    assert np.array_equal(got, want)
    assert (got == border).sum() >= (~ok).sum() > 0


def test_half_pixel_shift_is_the_rounded_mean():
    img = C.noise(17, 9)
    h, w = img.shape
    got = remap_ref(img, C.shift_map(w, h, 0, 0, q=16), 0)
    a, b = img[:, :-1].astype(np.int64), img[:, 1:].astype(np.int64)
    assert np.array_equal(got[:, :-1], ((a + b + 1) >> 1).astype(np.uint8))
    assert np.array_equal(got[:, -1], ((img[:, -1].astype(np.int64) + 0 + 1) >> 1).astype(np.uint8))  # border 0


def test_all_1024_fraction_pairs_match_the_closed_form():
    img = C.noise(17, 9)
    bx, by = 6, 3
    p00, p10, p01, p11 = (int(img[by, bx]), int(img[by, bx + 1]), int(img[by + 1, bx]), int(img[by + 1, bx + 1]))
    assert len({p00, p10, p01, p11}) == 4
    got = remap_ref(img, C.fraction_map(bx, by), 0)
    for j in range(32):
        for i in range(32):
            want = (p00 * (32 - i) * (32 - j) + p10 * i * (32 - j) + p01 * (32 - i) * j + p11 * i * j + 512) >> 10
            assert got[j, i] == want, (i, j)


@pytest.mark.parametrize("border", BORDERS)
def test_edge_taps_mix_in_the_border(border):
    img = C.noise(17, 9)
    h, w = img.shape
    fx, fy = 11, 20

    def one(sx, sy):
        m = C.as_map(np.array([[32 * sx + fx]]), np.array([[32 * sy + fy]]))
        return int(remap_ref(img, m, border)[0, 0])

    def px(x, y):
        return int(img[y, x]) if 0 <= x < w and 0 <= y < h else border

    for sx in (-1, w - 1, 4):
        for sy in (-1, h - 1, 2):
            want = (px(sx, sy) * (32 - fx) * (32 - fy) + px(sx + 1, sy) * fx * (32 - fy)
                    + px(sx, sy + 1) * (32 - fx) * fy + px(sx + 1, sy + 1) * fx * fy + 512) >> 10
            assert one(sx, sy) == want, (sx, sy)
    # whole maps of such taps, against a per-pixel loop
    m = C.edge_map(12, 10, w, h)
    got = remap_ref(img, m, border)
    for y in range(10):
        for x in range(12):
            iu, iv = int(m[y, x, 0]), int(m[y, x, 1])
            sx, sy, qx, qy = iu >> 5, iv >> 5, iu & 31, iv & 31
            want = (px(sx, sy) * (32 - qx) * (32 - qy) + px(sx + 1, sy) * qx * (32 - qy)
                    + px(sx, sy + 1) * (32 - qx) * qy + px(sx + 1, sy + 1) * qx * qy + 512) >> 10
            assert got[y, x] == want, (x, y)


@pytest.mark.parametrize("border", BORDERS)
def test_sentinel_and_far_entries_give_the_border(border):
    img = C.noise(17, 9)
    m = C.as_map(np.array([[SENTINEL, 2 ** 31 - 1, -2 ** 31, 40]]), np.array([[SENTINEL, 40, 40, 2 ** 31 - 1]]))
    assert np.array_equal(remap_ref(img, m, border), np.full((1, 4), border, np.uint8))
    assert np.all(remap_ref(img, C.outside_map(9, 7, 17, 9), border) == border)


def test_negative_coordinates_floor():
    img = np.array([[200, 100]], np.uint8)
    # iu = -1: sx = -1, fxq = 31 -> (border * 1 + p(0) * 31) * 32 rows' weight
    got = remap_ref(img, C.as_map(np.array([[-1]]), np.array([[0]])), 8)
    assert got[0, 0] == (8 * 1 * 32 + 200 * 31 * 32 + 512) >> 10
    got = remap_ref(img, C.as_map(np.array([[-33]]), np.array([[0]])), 8)  # sx = -2: nothing of the image
    assert got[0, 0] == 8


def test_remap_ref_checks_its_arguments():
    img = C.noise(17, 9)
    m = C.identity_map(3, 2)
    for bad in (-1, 256, 1.5):
        with pytest.raises(ValueError, match="border"):
            remap_ref(img, m, bad)
    with pytest.raises(ValueError, match="src"):
        remap_ref(img.astype(np.int32), m, 0)
    with pytest.raises(ValueError, match="map"):
        remap_ref(img, m.astype(np.int64), 0)
    view, buf = C.padded_buffer(img)
    assert np.array_equal(remap_ref(view, C.identity_map(17, 9), 0), img)  # a padded buffer's view: never its padding


# ------------------------------------------------------------------ 2. rectify_map_ref
@pytest.mark.parametrize("w,h", C.RECT_SIZES)
def test_identity_model_is_the_identity_map(w, h):
    cam, rect = C.models(w, h)["identity"]
    assert np.array_equal(rectify_map_ref(cam, rect), C.identity_map(w, h))


@pytest.mark.parametrize("w,h", C.RECT_SIZES)
def test_padded_camera_is_a_shift(w, h):
    cam, rect = C.models(w, h)["padcrop"]
    assert np.array_equal(rectify_map_ref(cam, rect), C.shift_map(w, h, C.PAD[0], C.PAD[1]))


def test_rays_behind_the_camera_get_the_sentinel():
    cam, rect = C.models(97, 61)["behind"]
    m = rectify_map_ref(cam, rect)
    u = np.arange(97, dtype=np.float64)[None, :]
    v = np.arange(61, dtype=np.float64)[:, None]
    x, y = (u - rect.cx) / rect.fx, (v - rect.cy) / rect.fy
    W = (np.float64(cam.R[2]) * x + np.float64(cam.R[5]) * y) + np.float64(cam.R[8])  # the same three operations
    sent = np.all(m == SENTINEL, -1)
    assert 0 < (W <= 0).sum() < W.size
    assert np.array_equal(sent, W <= 0)  # exactly there: no pixel of this model leaves the 2^24 range in front
    assert np.array_equal(sent, (m[..., 0] == SENTINEL) | (m[..., 1] == SENTINEL))


def test_far_pixels_of_a_large_k1_overflow_to_the_sentinel():
    cam, rect = C.models(97, 61)["overflow"]
    m = rectify_map_ref(cam, rect)
    sent = np.all(m == SENTINEL, -1)
    assert sent[0, 0] and sent[-1, -1] and 0 < sent.sum() < sent.size
    assert np.all(np.abs(m[~sent].astype(np.int64)) < 32 * 2 ** 24)


def _rn(q):
    """A rational rounded to the nearest double (ties to even): int / int division is correctly rounded."""
    return q.numerator / q.denominator


def _exact_entry(cam, rect, u, v):
    """One map entry with every operation computed exactly in rationals and rounded once, in the header's order."""
    F = Fraction
    add = lambda p, q: _rn(F(p) + F(q))  # noqa: E731
    sub = lambda p, q: _rn(F(p) - F(q))  # noqa: E731
    mul = lambda p, q: _rn(F(p) * F(q))  # noqa: E731
    div = lambda p, q: _rn(F(p) / F(q))  # noqa: E731
    R = cam.R
    k1, k2, p1, p2, k3 = cam.dist
    x = div(sub(float(u), rect.cx), rect.fx)
    y = div(sub(float(v), rect.cy), rect.fy)
    X = add(add(mul(R[0], x), mul(R[3], y)), R[6])
    Y = add(add(mul(R[1], x), mul(R[4], y)), R[7])
    W = add(add(mul(R[2], x), mul(R[5], y)), R[8])
    a, b = div(X, W), div(Y, W)
    a2, b2 = mul(a, a), mul(b, b)
    r2 = add(a2, b2)
    tab = mul(2.0, mul(a, b))
    rad = add(1.0, mul(r2, add(k1, mul(r2, add(k2, mul(r2, k3))))))
    xd = add(add(mul(a, rad), mul(p1, tab)), mul(p2, add(r2, mul(2.0, a2))))
    yd = add(add(mul(b, rad), mul(p1, add(r2, mul(2.0, b2)))), mul(p2, tab))
    us, vs = add(mul(cam.fx, xd), cam.cx), add(mul(cam.fy, yd), cam.cy)
    assert W > 0 and abs(us) < 2 ** 24 and abs(vs) < 2 ** 24
    return round(mul(us, 32.0)), round(mul(vs, 32.0))  # (round(): half to even, as rint)


def test_every_step_is_the_correctly_rounded_one():
    """20 pixels of the strong model: corners, edge midpoints, the centre, and
    pixels spread over the image.  A contraction, a reordering or a
    'simplified' expression moves at least one of them in the last place."""
    cam, rect = C.models(200, 130)["strong"]
    m = rectify_map_ref(cam, rect)
    pix = [(0, 0), (199, 0), (0, 129), (199, 129), (100, 65), (99, 64), (0, 65), (199, 65), (100, 0), (100, 129),
           (13, 7), (57, 101), (150, 33), (181, 120), (31, 88), (77, 19), (123, 77), (166, 5), (5, 111), (142, 126)]
    for u, v in pix:
        assert (int(m[v, u, 0]), int(m[v, u, 1])) == _exact_entry(cam, rect, u, v), (u, v)
    # and a camera of another size and focal length
    cam_o, rect_o = C.models(97, 61)["other"]
    mo = rectify_map_ref(cam_o, rect_o)
    for u, v in [(0, 0), (96, 60), (40, 30), (11, 50)]:
        assert (int(mo[v, u, 0]), int(mo[v, u, 1])) == _exact_entry(cam_o, rect_o, u, v), (u, v)


@pytest.mark.parametrize("name", C.MODEL_NAMES)
def test_map_entries_are_sentinel_pairs_or_in_range(name):
    cam, rect = C.models(97, 61)[name]
    m = rectify_map_ref(cam, rect).astype(np.int64)
    sent = m[..., 0] == SENTINEL
    assert np.array_equal(sent, m[..., 1] == SENTINEL)
    assert np.all(np.abs(m[~sent]) <= 32 * 2 ** 24)


# ------------------------------------------------------------------ 3. validation
GOOD = dict(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0)


@pytest.mark.parametrize("cls", [CameraModel, RectifiedModel])
@pytest.mark.parametrize("key,bad", [("fx", 0.0), ("fy", -1.0), ("fx", math.nan), ("cx", math.inf), ("cy", math.nan),
                                     ("width", 0), ("height", -3)])
def test_models_reject_bad_parameters(cls, key, bad):
    cls(**GOOD)
    with pytest.raises(ValueError):
        cls(**{**GOOD, key: bad})


def test_camera_model_rejects_bad_distortion_and_rotation():
    for kw in (dict(dist=(0.0, math.nan, 0.0, 0.0, 0.0)), dict(dist=(0.0,) * 4), dict(R=(1.0,) * 8),
               dict(R=(math.inf,) + (0.0,) * 8)):
        with pytest.raises(ValueError):
            CameraModel(**GOOD, **kw)
    assert CameraModel(**GOOD, R=np.eye(3)).R == tuple(np.eye(3).ravel())  # a 3 x 3 array is taken row-major


def test_rectifier_rejects_a_bad_border_and_wrong_raw_shapes():
    r = RectifiedModel(**GOOD)
    cam = C.padded_camera(r)
    for bad in (-1, 256, 0.5):
        with pytest.raises(ValueError, match="border"):
            StereoRectifier(cam, cam, r, border=bad)
    rig = StereoRectifier(cam, cam, r, border=3)
    with pytest.raises(ValueError, match="left"):
        rig.apply_ref(np.zeros((48, 64), np.uint8), np.zeros(cam.shape, np.uint8))
    with pytest.raises(ValueError, match="right"):
        rig.apply_ref(np.zeros(cam.shape, np.uint8), np.zeros((48, 64), np.uint8))
    L, R = rig.apply_ref(np.full(cam.shape, 9, np.uint8), np.full(cam.shape, 7, np.uint8))
    assert L.shape == R.shape == r.shape and np.all(L == 9) and np.all(R == 7)


def test_pipeline_config_checks_the_rectifier():
    cfg0 = KC.loop_config()
    _, K = KC.sequence()[:2]
    assert cfg0.rectify is None and PL.Backend.rectifier is None
    rig = C.padded_rectifier(cfg0.width, cfg0.height, K)
    assert KC.loop_config(rectify=rig).rectify is rig
    small = C.padded_rectifier(cfg0.width - 2, cfg0.height, K)
    with pytest.raises(ValueError, match="rectif"):
        KC.loop_config(rectify=small)
    with pytest.raises(ValueError, match="rectify"):
        KC.loop_config(rectify="maps.npz")
    # the rectified model is the loop's K
    from pipeline_oracle import OracleBackend

    K2 = np.array(K, np.float64)
    K2[0, 2] += 1.0
    with pytest.raises(ValueError, match="K"):
        PL.WindowedStereoVO(KC.loop_config(rectify=rig), OracleBackend(), K2)


def test_abi_version_and_exports():
    import ctypes

    from uasl_motion_estimation_amd import _lib

    lib = _lib.load_library()
    assert lib.me_abi_version() == 4
    for name in ("me_rectify_map", "me_remap_q5", "me_remap_tile_dims", "me_vo_loop_set_rectify"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.KT["RECTIFY"] == 12 and max(_lib.KT.values()) < 16
    assert not any("rect" in f[0] for f in _lib.VOLoopConfigC._fields_)  # a setter, not a configuration field
    tw, th, words = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.me_remap_tile_dims(ctypes.byref(tw), ctypes.byref(th), ctypes.byref(words)) == 0
    assert tw.value > 0 and tw.value % 4 == 0 and th.value > 0 and words.value > 0
    assert lib.me_remap_tile_dims(ctypes.byref(tw), ctypes.byref(th), None) == 0
    assert lib.me_remap_tile_dims(None, ctypes.byref(th), None) == -1
    # the structures the bindings pass are the header's
    assert ctypes.sizeof(_lib.CameraModelC) == 8 + 8 * 18 and ctypes.sizeof(_lib.RectifiedModelC) == 8 + 8 * 4


def test_cpp_setter_and_c_header_compile(tmp_path):
    """A C++ translation unit that calls WindowedStereoVO::setRectification (the flags of tests/cpp/Makefile), and
    the header as C: the setter is declared ahead of the model's definition."""
    import os
    import subprocess

    inc = "-I" + os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    src = tmp_path / "set_rect.cpp"
    src.write_text('#include "MotionEstimationAMD/motion_estimation_amd.hpp"\n'
                   "void on(me::WindowedStereoVO& vo, const me_camera_model& l, const me_camera_model& r) {\n"
                   "  vo.setRectification(l, r, 7);\n  vo.clearRectification();\n}\n")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", inc, "-c", str(src), "-o",
                    str(tmp_path / "set_rect.o")], check=True)
    csrc = tmp_path / "hdr.c"
    csrc.write_text('#include "me_hip.h"\n'
                    "int on(me_vo_loop* v, const me_camera_model* l, const me_camera_model* r) {\n"
                    "  me_rectified_model m = {1, 1, 1.0, 1.0, 0.0, 0.0};\n"
                    "  return me_vo_loop_set_rectify(v, l, r, m.width) + ME_KT_RECTIFY;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", inc, "-c", str(csrc), "-o",
                    str(tmp_path / "hdr.o")], check=True)


# ------------------------------------------------------------------ 4. the host loop
def test_oracle_loop_on_padded_frames_is_the_plain_loop(oracle):
    """Raw = the frames padded by (8, 5) with 77, the camera's principal point
    shifted by the padding: the warp is the crop, so the loop sees the plain
    loop's pixels and takes its every decision."""
    from pipeline_oracle import OracleBackend

    plain = KC.oracle_loop()
    _, K, p0, v, _ = KC.sequence()
    rig = C.padded_rectifier(plain.cfg.width, plain.cfg.height, K)
    L, R = rig.apply_ref(*C.padded_sequence()[0])
    fr = KC.sequence()[0]
    assert np.array_equal(L, fr[0].left) and np.array_equal(R, fr[0].right)
    vo = PL.WindowedStereoVO(KC.loop_config(rectify=rig), OracleBackend(), K, p0, v, log_events=True)
    C.run_raw(vo, C.padded_sequence())
    assert len(vo.results) == KC.N_KEYFRAMES and vo.results[-1].n_tracked > 0
    C.same_loop(vo, plain)
    with pytest.raises(ValueError, match="raw left"):
        vo.process(KC.N_KEYFRAMES, fr[0].left, fr[0].right)  # unpadded frames: not the camera's size
