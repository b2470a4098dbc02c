"""16-bit ingest, the parts that need no GPU: the numpy restatement
(tonemap.tonemap_ref) against the hand checks of include/me_hip.h (section
A12g) and a restatement by sorting, the temporal filter, imread_gray16, the
parameter checks of ToneMap and PipelineConfig, and the switch on the
oracle-backend loop -- the loop that starves on the high byte of a 16-bit
stream and tracks on its tone-mapped twin."""
import numpy as np
import pytest

import klt_fb_cases as KC
import tonemap_cases as TC
from uasl_motion_estimation_amd import file_io
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd.tonemap import (INT32_MAX, ToneMap, filter_state, frame_ranks, frame_window,
                                                tonemap_ref)


# ------------------------------------------------------------------ 1. the definition
def test_constant_images_widen_and_clamp():
    """Defaults, min_span 256.  0: lo = -128 -> 0, hi = 256, out = (0 + 128) / 256 = 0.  30 000: window 29 872 ..
    30 128, out = (128 * 255 + 128) / 256 = 128.  65 535: hi = 65 663 -> 65 535, lo = 65 279, out = (256 * 255 + 128)
    / 256 = 255."""
    for v, window, want in [(0, (0, 256), 0), (30000, (29872, 30128), 128), (65535, (65279, 65535), 255)]:
        img = np.full((48, 64), v, np.uint16)
        assert frame_window(img, ToneMap()) == window
        out, st = tonemap_ref(img, ToneMap())
        assert st == (window[0] << 8, window[1] << 8, 1)
        assert out.dtype == np.uint8 and out.shape == (48, 64) and np.all(out == want), (v, out[0, 0])


def test_one_pixel_image():
    out, st = tonemap_ref(np.array([[5]], np.uint16), ToneMap())
    assert st == (0, 256 << 8, 1) and out[0, 0] == (5 * 255 + 128) // 256 == 5
    out, st = tonemap_ref(np.array([[40000]], np.uint16), TC.EXACT)  # lo = hi = 40 000 widened to 40 000 .. 40 001
    assert st == (40000 << 8, 40001 << 8, 1) and out[0, 0] == 0


def test_image_of_exactly_lo_and_hi():
    img = np.full((48, 64), 1000, np.uint16)
    img[:, 32:] = 3000
    for p in (ToneMap(), ToneMap(0, 0, 256, 64)):  # k = 3 of 3072 pixels, and k = 0
        assert frame_window(img, p) == (1000, 3000)
        out, _ = tonemap_ref(img, p)
        assert np.all(out[:, :32] == 0) and np.all(out[:, 32:] == 255)


def test_twice_the_byte_maps_back_exactly():
    """ppm 0, alpha 256: a + 2 v with v over 0 .. 255 has the window a .. a + 510 and q / span = (510 v + 255) / 510 = v."""
    v8 = np.random.default_rng(2).integers(0, 256, (37, 53)).astype(np.uint8)
    v8[0, 0], v8[0, 1] = 0, 255
    for a in (0, 7000, 65535 - 510):
        out, st = tonemap_ref((a + 2 * v8.astype(np.int64)).astype(np.uint16), TC.EXACT)
        assert st == (a << 8, (a + 510) << 8, 1) and np.array_equal(out, v8)


@pytest.mark.parametrize("name", TC.SELECT_CASES)
def test_rank_rules_against_sorting(name):
    img, p = TC.select_case(name)
    lo, hi = TC.window_by_sorting(img, p)
    assert lo <= hi and frame_ranks(img, p) == (lo, hi)


def test_rank_cases_sit_on_the_bin_edges():
    first, p1 = TC.select_case("rank_on_first_pixel_of_a_bin")
    last, p2 = TC.select_case("rank_on_last_pixel_of_a_bin")
    lo, hi = frame_ranks(first, p1)
    assert lo >> 8 == 0x20 and lo == first[first >= 0x2000].min() and hi >> 8 == 0x20 and hi == first[first < 0x3000].max()
    assert frame_ranks(last, p2) == (0x1000, 0x3005)


@pytest.mark.parametrize("size", [(1, 1), (7, 3), (9, 5), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_brute_force_cross_check(size):
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    for k, p in enumerate([ToneMap(), ToneMap(0, 0, 1, 256), ToneMap(200000, 300000, 40, 100), ToneMap(499999, 499999, 65535, 1)]):
        st_a = st_b = None
        for t in range(3):
            img = rng.integers(0, 65536 if k % 2 else 2000, (h, w)).astype(np.uint16) + np.uint16(300 * t)
            a, st_a = tonemap_ref(img, p, st_a)
            b, st_b = TC.brute_force(img, p, st_b)
            assert st_a == st_b and np.array_equal(a, b), (size, p, t)


def test_strided_views_are_read_as_images():
    img = TC.noise14(61, 7)
    buf = np.full((7, 64), 9, np.uint16)
    buf[:, :61] = img
    a, sa = tonemap_ref(buf[:, :61], ToneMap())
    b, sb = tonemap_ref(img, ToneMap())
    assert sa == sb and np.array_equal(a, b)


# ------------------------------------------------------------------ 2. the filter
def _two(lo, hi):
    img = np.full((8, 8), lo, np.uint16)
    img[:, 4:] = hi
    return img


def test_filter_by_hand():
    """Windows 1000 .. 3000, 2000 .. 4000, 1000 .. 3000.  alpha 256: the frame's own.  alpha 64: 256 000 + 256 000 / 4
    = 320 000, then 320 000 + floor(-64 000 / 4) = 304 000.  alpha 100: 256 000 + 100 000 = 356 000, then 356 000 +
    floor(-100 000 * 100 / 256 = -39 062.5) = 316 937: floor, not truncation."""
    frames = [_two(1000, 3000), _two(2000, 4000), _two(1000, 3000)]
    want = {256: [(256000, 768000, 1), (512000, 1024000, 2), (256000, 768000, 3)],
            64: [(256000, 768000, 1), (320000, 832000, 2), (304000, 816000, 3)],
            100: [(256000, 768000, 1), (356000, 868000, 2), (316937, 828937, 3)]}
    for alpha, states in want.items():
        p, st = ToneMap(0, 0, 1, alpha), None
        for img, w in zip(frames, states):
            out, st = tonemap_ref(img, p, st)
            assert st == w, (alpha, st, w)
        # the window used after the last frame: lo_u floors, hi_u ceils
        lo_u, hi_u = st[0] >> 8, (st[1] + 255) >> 8
        assert out[0, 0] == (0 if 1000 < lo_u else ((1000 - lo_u) * 255 + (hi_u - lo_u) // 2) // (hi_u - lo_u))
    assert (316937 >> 8, (828937 + 255) >> 8) == (1238, 3239)


def test_frames_saturates_and_zero_frames_is_a_reset():
    p = ToneMap(0, 0, 1, 64)
    assert filter_state(1000, 3000, p, (256000, 768000, INT32_MAX))[2] == INT32_MAX
    assert filter_state(1000, 3000, p, (256000, 768000, INT32_MAX - 1))[2] == INT32_MAX
    img = _two(2000, 4000)
    a, sa = tonemap_ref(img, p, (123, 456, 0))  # frames = 0: the words are not read
    b, sb = tonemap_ref(img, p, None)
    assert sa == sb == (512000, 1024000, 1) and np.array_equal(a, b)


# ------------------------------------------------------------------ 3. files
def test_imread_gray16_round_trip(tmp_path):
    from PIL import Image

    a = (7000 + TC.noise14(33, 17) % 700).astype(np.uint16)
    a[0, 0], a[0, 1] = 0, 65535
    Image.fromarray(a).save(tmp_path / "wide.png")
    got = file_io.imread_gray16(str(tmp_path / "wide.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, a)
    assert np.array_equal(file_io.imread_gray(str(tmp_path / "wide.png")), (a >> 8).astype(np.uint8))  # as before
    b = np.random.default_rng(1).integers(0, 256, (9, 11)).astype(np.uint8)
    b[0, 0], b[0, 1] = 0, 255
    Image.fromarray(b).save(tmp_path / "narrow.png")
    got = file_io.imread_gray16(str(tmp_path / "narrow.png"))
    assert got.dtype == np.uint16 and np.array_equal(got, b.astype(np.uint16) * 257) and got[0, 1] == 65535
    (tmp_path / "broken.png").write_bytes(b"not a png")
    assert file_io.imread_gray16(str(tmp_path / "broken.png")) is None
    assert file_io.imread_gray16(str(tmp_path / "missing.png")) is None


# ------------------------------------------------------------------ 4. parameters
def test_tonemap_parameter_checks():
    d = ToneMap()
    assert (d.lo_ppm, d.hi_ppm, d.min_span, d.alpha_q8) == (1000, 1000, 256, 64)
    ToneMap(0, 999999, 1, 1), ToneMap(999999, 0, 65535, 256)
    for kw, word in [(dict(lo_ppm=-1), "lo_ppm"), (dict(hi_ppm=-1), "hi_ppm"), (dict(lo_ppm=1.5), "lo_ppm"),
                     (dict(lo_ppm=500000, hi_ppm=500000), "lo_ppm \\+ hi_ppm"), (dict(min_span=0), "min_span"),
                     (dict(min_span=65536), "min_span"), (dict(min_span=True), "min_span"),
                     (dict(alpha_q8=0), "alpha_q8"), (dict(alpha_q8=257), "alpha_q8"), (dict(alpha_q8="x"), "alpha_q8")]:
        with pytest.raises(ValueError, match=word):
            ToneMap(**kw)
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4,), np.uint16), np.zeros((0, 4), np.uint16)):
        with pytest.raises(ValueError, match="uint16"):
            tonemap_ref(bad, ToneMap())


def test_pipeline_config_checks_and_uint16_without_the_switch(oracle):
    from pipeline_oracle import OracleBackend

    assert PL.PipelineConfig.from_config(1).tonemap is None
    assert KC.loop_config(tonemap=ToneMap(0, 0, 16, 256)).tonemap == ToneMap(0, 0, 16, 256)
    for bad in ((1000, 1000, 256, 64), True):
        with pytest.raises(ValueError, match="ToneMap"):
            KC.loop_config(tonemap=bad)
    _, K, p0, v, _ = KC.sequence()
    vo = PL.WindowedStereoVO(KC.loop_config(), OracleBackend(), K, p0, v)
    with pytest.raises(ValueError, match="tonemap"):
        vo.process(0, *TC.wide_sequence()[0])


# ------------------------------------------------------------------ 5. the loop
def test_switch_equals_mapping_outside(oracle):
    """The loop with tonemap=ToneMap() fed the 16-bit stream holds what the loop holds that was fed tonemap_ref's
    8-bit output (a state per camera, carried from keyframe to keyframe), event for event and pose for pose."""
    from rectify_cases import same_loop

    on = TC.oracle_loop("wide", tonemap=ToneMap())
    outside = TC.oracle_loop("outside")
    assert on.events == outside.events and len(on.events) > 0
    same_loop(on, outside)
    assert all(np.array_equal(a.pose, b.pose) for a, b in zip(on.results, outside.results))


def test_loop_tracks_more_than_on_the_high_byte(oracle):
    """Config 1, 6 keyframes, the stream 7000 + 40 t + 2 v.  Features tracked per keyframe on the oracle backend
    (DESIGN.md 5.12 has the table): the plain 8-bit stream, its high byte (three levels: what imread_gray hands on
    today) and the tone-mapped stream."""
    plain = TC.oracle_loop("plain")
    high = TC.oracle_loop("high")
    on = TC.oracle_loop("wide", tonemap=ToneMap())
    rows = {k: [r.n_tracked for r in vo.results] for k, vo in (("plain", plain), ("high", high), ("tonemap", on))}
    print(rows)
    assert sum(rows["tonemap"][1:6]) > sum(rows["high"][1:6])


def test_switch_off_is_the_plain_loop(oracle):
    """tonemap=None runs the loop it ran before the switch existed (the cached plain oracle loop of klt_fb_cases)."""
    from rectify_cases import same_loop

    same_loop(TC.oracle_loop("plain", tonemap=None), KC.oracle_loop())
