"""Stereo rectification on the device (me_rectify_map / me_remap_q5,
csrc/rectify.hip) against the numpy restatement (rectify.rectify_map_ref /
remap_ref), bit for bit: every model, every tap case, both tile paths of the
remap (reported through tile_path), both memory modes; and the loop switch --
PipelineConfig.rectify on the Python GPU loop and me_vo_loop_set_rectify on the
native loop -- against the plain loops and the oracle loop."""
import ctypes
import functools
import types

import numpy as np
import pytest

import klt_fb_cases as KC
import rectify_cases as C
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import MEError
from uasl_motion_estimation_amd.rectify import (CameraModel, rectify_map, rectify_map_ref, remap, remap_ref,
                                                tile_dims, tile_grid)

pytestmark = pytest.mark.gpu

FILL = 0xA5  # pre-fill of every destination buffer: padding must keep it


# ------------------------------------------------------------------ 5. the map
@pytest.mark.parametrize("size", C.RECT_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", C.MODEL_NAMES)
def test_map_matches_the_restatement(ctx, name, size):
    cam, rect = C.models(*size)[name]
    want = rectify_map_ref(cam, rect)
    for device in (False, True):
        got = rectify_map(cam, rect, ctx, device=device)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, size, device)


def test_map_rejects_bad_models(ctx):
    cam, rect = C.models(5, 7)["identity"]
    out = np.zeros((7, 5, 2), np.int32)

    def call(cc, rc):
        return ctx.lib.me_rectify_map(ctx.h, 0, ctypes.byref(cc), ctypes.byref(rc), ctypes.c_void_p(out.ctypes.data))

    assert call(cam.to_c(), rect.to_c()) == 0
    for side, field, bad, word in [(0, "fx", 0.0, "fx"), (0, "fy", float("nan"), "fx"), (0, "width", 0, "width"),
                                   (1, "fy", -1.0, "fy"), (1, "cx", float("inf"), "cx"), (1, "height", 0, "height")]:
        cc, rc = cam.to_c(), rect.to_c()
        setattr((cc, rc)[side], field, bad)
        assert call(cc, rc) == -1
        msg = ctx.lib.me_last_error(ctx.h).decode()
        assert word in msg and ("camera", "rectified")[side] in msg, msg
    cc = cam.to_c()
    cc.dist[1] = float("nan")
    assert call(cc, rect.to_c()) == -1 and "dist" in ctx.lib.me_last_error(ctx.h).decode()
    cc = cam.to_c()
    cc.R[4] = float("inf")
    assert call(cc, rect.to_c()) == -1 and " R " in ctx.lib.me_last_error(ctx.h).decode()


# ------------------------------------------------------------------ 6. the remap
def _dst_shapes():
    tw, th, _ = tile_dims()
    return {"1x1": (1, 1, 0), "3x2": (3, 2, 0), "5x7": (5, 7, 0), "tile": (tw, th, 0), "tile+1": (tw + 1, th + 1, 0),
            "97x61": (97, 61, 0), "200x130s": (200, 130, 3)}  # (dst_w, dst_h, bytes of row padding)


DST = ["1x1", "3x2", "5x7", "tile", "tile+1", "97x61", "200x130s"]
SRC = {"1x1": (1, 1, 0), "17x9": (17, 9, 0), "80x64s": (80, 64, 3), "200x130": (200, 130, 0)}


@functools.lru_cache(maxsize=None)
def _model_maps(dw, dh):
    return {"model_" + n: rectify_map_ref(*C.models(dw, dh)[n]) for n in C.MODEL_NAMES}


def _source(img_fn, sw, sh, extra):
    img = img_fn(sw, sh)
    return C.padded_buffer(img, extra)[0] if extra else img


def run_remap(ctx, src, m, border, extra=0, device=False, tile_path=True):
    """me_remap_q5 into a view of a buffer pre-filled with FILL; checks that the padding kept it."""
    dh, dw = m.shape[:2]
    buf = np.full((dh, dw + extra), FILL, np.uint8)
    res = remap(src, m, border=border, ctx=ctx, tile_path=tile_path, out=buf[:, :dw], device=device)
    assert np.all(buf[:, dw:] == FILL), "the destination's row padding was written"
    return (buf[:, :dw].copy(), res[1]) if tile_path else (buf[:, :dw].copy(), None)


@pytest.mark.parametrize("src_id", list(SRC))
@pytest.mark.parametrize("dst_id", DST)
def test_remap_matches_the_restatement(ctx, dst_id, src_id):
    dw, dh, d_extra = _dst_shapes()[dst_id]
    sw, sh, s_extra = SRC[src_id]
    maps = dict(C.user_maps(dw, dh, sw, sh))
    maps["fractions"] = C.fraction_map(min(6, sw - 1), min(3, sh - 1))  # (32 x 32, whatever the destination)
    maps.update(_model_maps(dw, dh))
    both_modes = dst_id in ("97x61", "200x130s") or src_id == "80x64s"
    paths = set()
    for k, (name, m) in enumerate(maps.items()):
        for img_fn, border in ((C.noise, 0), (C.checker, 255)):
            src = _source(img_fn, sw, sh, s_extra)
            want = remap_ref(src, m, border)
            extra = d_extra if m.shape[:2] == (dh, dw) else 0
            for device in ((False, True) if both_modes and k % 3 == 0 else (False,)):
                got, tp = run_remap(ctx, src, m, border, extra, device)
                assert np.array_equal(got, want), (name, border, device, np.argwhere(got != want)[:4])
                assert tp.shape == tile_grid(m.shape[1], m.shape[0])[::-1]
                assert np.array_equal(tp, C.tile_paths_ref(m, sw, sh, *tile_dims())), (name, tp)
                paths |= set(tp.ravel().tolist())
    # the random maps' taps span the 200 x 130 source, more than the staging holds; every other source fits whole
    big = src_id == "200x130" and dst_id != "1x1"
    assert paths == ({0, 1} if big else {0}), paths


def test_remap_rejects_bad_arguments(ctx):
    src, m = C.noise(17, 9), C.identity_map(5, 7)
    dst = np.zeros((7, 5), np.uint8)
    V = ctypes.c_void_p

    def call(sw=17, sh=9, ss=17, dw=5, dh=7, border=0, ds=5, s=src, mp=m, d=dst):
        rc = ctx.lib.me_remap_q5(ctx.h, 0, V(s.ctypes.data) if s is not None else None, sw, sh, ss,
                                 V(mp.ctypes.data) if mp is not None else None, dw, dh, border,
                                 V(d.ctypes.data) if d is not None else None, ds, None)
        return rc, ctx.lib.me_last_error(ctx.h).decode()

    assert call()[0] == 0
    for kw, word in [(dict(sw=0), "src_w"), (dict(sh=0), "src_h"), (dict(ss=16), "src_stride"), (dict(dw=0), "dst_w"),
                     (dict(dh=-1), "dst_h"), (dict(ds=4), "dst_stride"), (dict(border=-1), "border"),
                     (dict(border=256), "border"), (dict(s=None), "src"), (dict(mp=None), "map"), (dict(d=None), "dst")]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)


# ------------------------------------------------------------------ 7. the paths
def test_each_path_is_reached_by_the_remap_cases(ctx):
    """The two cases of test_remap_matches_the_restatement that pin the paths:
    the identity map stages every tile, the random map over the 200 x 130
    source spans more than the staging buffer holds in every full tile."""
    src = C.noise(200, 130)
    m0, m1 = C.identity_map(200, 130), C.random_map(200, 130, 200, 130, 11)
    got0, tp0 = run_remap(ctx, src, m0, 0)
    got1, tp1 = run_remap(ctx, src, m1, 0)
    assert np.array_equal(got0, remap_ref(src, m0, 0)) and np.array_equal(got1, remap_ref(src, m1, 0))
    assert np.all(tp0 == 0) and np.all(tp1 == 1)
    # a tile none of whose entries touches the image stages nothing: path 0
    got2, tp2 = run_remap(ctx, src, C.outside_map(200, 130, 200, 130), 9)
    assert np.all(got2 == 9) and np.all(tp2 == 0)


def _capacity_boxes():
    """(words, rows) of a box that fills the staging buffer exactly: an odd row stride that divides the capacity."""
    tw, th, cap = tile_dims()
    stride = next(s for s in range(63, 2, -2) if cap % s == 0)
    return stride - 1, cap // stride, cap


def test_box_at_and_past_the_staging_capacity(ctx):
    tw, th, cap = tile_dims()
    words, rows, _ = _capacity_boxes()
    assert ((words + 1) | 1) * rows == cap
    sw, sh = 4 * (words + 1) + 3, rows + 3
    src = C.noise(sw, sh, seed=5)
    dw, dh = min(tw, 16), min(th, 8)  # one tile
    cases = {
        "exact": (C.box_map(dw, dh, 0, 0, 4 * words - 1, rows - 1), 0),
        "one_more_row": (C.box_map(dw, dh, 0, 0, 4 * words - 1, rows), 1),
        "one_more_word": (C.box_map(dw, dh, 0, 0, 4 * words, rows - 1), 1),
        # the same boxes away from the origin and off the word grid
        "exact_moved": (C.box_map(dw, dh, 5, 2, 4 * words + 3, rows + 1), 0),
        "one_more_word_moved": (C.box_map(dw, dh, 3, 2, 4 * words + 4, rows + 1), 1),
    }
    for name, (m, path) in cases.items():
        got, tp = run_remap(ctx, src, m, 31)
        assert np.array_equal(got, remap_ref(src, m, 31)), name
        assert tp.shape == (1, 1) and tp[0, 0] == path, (name, tp)


def test_realistic_model_share_of_global_tiles(ctx):
    cam, rect = C.realistic(320, 180)
    m = rectify_map(cam, rect, ctx)
    assert np.array_equal(m, rectify_map_ref(cam, rect))
    src = C.noise(320, 180)
    got, tp = run_remap(ctx, src, m, 0)
    assert np.array_equal(got, remap_ref(src, m, 0))
    print("realistic model at 320 x 180: %d of %d tiles on the global path" % (int(tp.sum()), tp.size))


def test_output_without_tile_path_is_the_same(ctx):
    src = C.noise(200, 130)
    for m in (C.identity_map(97, 61), C.random_map(97, 61, 200, 130, 11), C.edge_map(97, 61, 200, 130)):
        for device in (False, True):
            a, _ = run_remap(ctx, src, m, 255, 3, device, tile_path=True)
            b, _ = run_remap(ctx, src, m, 255, 3, device, tile_path=False)
            assert np.array_equal(a, b) and np.array_equal(a, remap_ref(src, m, 255))


def test_rectifier_apply_matches_apply_ref(ctx):
    rig, frames = C.rig_sequence()
    try:
        L, R = rig.apply(ctx, *frames[0])
    finally:
        rig.release(ctx)
    rl, rr = rig.apply_ref(*frames[0])
    assert np.array_equal(L, rl) and np.array_equal(R, rr)


def test_stereo_stream_with_a_rectifier_yields_raw_frames_per_camera(tmp_path, ctx):
    """file_io.StereoImageStream(rectifier=...): slots of each camera's own size, both sizes in the tuple, the
    device copies are the files' pixels and warp to apply_ref's output; a frame of another size is refused."""
    from PIL import Image

    from test_file_io import YML
    from uasl_motion_estimation_amd import file_io as F
    from uasl_motion_estimation_amd.rectify import RectifiedModel, StereoRectifier

    out = RectifiedModel(64, 48, 60.0, 60.0, 32.0, 24.0)
    rig = StereoRectifier(CameraModel(72, 50, 62.0, 61.0, 36.5, 25.0, (-0.05, 0.0, 0.0, 0.0, 0.0)),
                          CameraModel(60, 44, 55.0, 55.0, 30.0, 22.0, (0.05, 0.0, 0.0, 0.0, 0.0)), out, border=9)
    rng = np.random.default_rng(2)
    frames = {}
    for nb in range(2, 7):
        L = rng.integers(0, 256, rig.left.shape, dtype=np.uint8)
        R = rng.integers(0, 256, rig.right.shape, dtype=np.uint8)
        Image.fromarray(L).save(tmp_path / f"cam0_image{nb:05d}_rect.png")
        Image.fromarray(R).save(tmp_path / f"cam1_image{nb:05d}_rect.png")
        frames[nb] = (L, R)
    (tmp_path / "image_data.csv").write_text("#img,stamp\n" + "".join(f"{nb},{nb * 100}\n" for nb in range(2, 7)))
    (tmp_path / "cfg.yml").write_text(YML.format(dir=str(tmp_path)))
    cfg = F.loadYML(str(tmp_path / "cfg.yml"))
    seen = []
    n = out.width * out.height
    d_out = ctx.malloc(2 * n)
    try:
        for nb, stamp, dL, dR, wl, hl, wr, hr in F.StereoImageStream(cfg, ctx, rectifier=rig):
            assert (hl, wl) == rig.left.shape and (hr, wr) == rig.right.shape and stamp == 100 * nb
            rig.apply_device(ctx, dL, dR, d_out, d_out + n)
            got = np.zeros((2,) + out.shape, np.uint8)
            ctx.synchronize()
            ctx.d2h(got, d_out)
            rl, rr = rig.apply_ref(*frames[nb])
            assert np.array_equal(got[0], rl) and np.array_equal(got[1], rr)
            seen.append(nb)
    finally:
        ctx.free(d_out)
        rig.release(ctx)
    assert seen == [2, 3, 4, 5, 6]
    swapped = StereoRectifier(rig.right, rig.left, out)
    with pytest.raises(ValueError, match="frame 2"):
        next(iter(F.StereoImageStream(cfg, ctx, rectifier=swapped)))


# ------------------------------------------------------------------ 8. the loops
def snap(vo):
    """What the comparisons read, detached from the loop (a native loop is closed afterwards)."""
    return types.SimpleNamespace(events=list(vo.events), ids=np.array(vo.ids), X=np.array(vo.X),
                                 active=np.array(vo.active), poses={t: np.array(p) for t, p in vo.poses.items()},
                                 results=list(vo.results), K=np.array(vo.K), cfg=vo.cfg)


_LOOPS = {}


def gpu_loop(ctx, kind, frames_id, rectify=None, **cfg_kw):
    """A config-1 loop on the GPU (kind "native" / "python"), cached per (kind, input, switches)."""
    key = (kind, frames_id, tuple(sorted(cfg_kw.items())))
    if key in _LOOPS:
        return _LOOPS[key]
    fr, K, p0, v, _ = KC.sequence()
    frames = {"plain": [(fr[t].left, fr[t].right) for t in range(KC.N_KEYFRAMES)], "padded": C.padded_sequence(),
              "rig": C.rig_sequence()[1]}[frames_id]
    cfg = KC.loop_config(rectify=rectify, **cfg_kw)
    if kind == "native":
        g = PL.NativeStereoVO(cfg, ctx, K, p0, v, log_events=True)
        try:
            _LOOPS[key] = snap(C.run_raw(g, frames))
        finally:
            g.close()
    else:
        be = PL.GPUBackend(ctx)
        try:
            _LOOPS[key] = snap(C.run_raw(PL.WindowedStereoVO(cfg, be, K, p0, v, log_events=True, overlap=True), frames))
        finally:
            be.close()
    return _LOOPS[key]


def check_against_oracle(g, o):
    from test_pipeline import _check_against_oracle  # the bar the loops are already held to (events exact, 1e-6)

    assert [r.n_tracked for r in g.results] == [r.n_tracked for r in o.results]
    _check_against_oracle(g, o, 4, KC.N_KEYFRAMES)


def _padded_rig():
    cfg = KC.loop_config()
    return C.padded_rectifier(cfg.width, cfg.height, KC.sequence()[1])


@pytest.mark.parametrize("kind", ["native", "python"])
def test_loop_on_padded_frames_is_the_plain_loop(ctx, oracle, kind):
    """8a: raw = the frames padded by (8, 5) with 77 and the camera that crops
    them back: the loop sees the plain loop's pixels, so everything it holds
    is the plain GPU loop's bit for bit, and the oracle loop's at the loops' bar."""
    plain = gpu_loop(ctx, kind, "plain")
    g = gpu_loop(ctx, kind, "padded", rectify=_padded_rig())
    assert g.results[-1].n_tracked > 100
    C.same_loop(g, plain)
    check_against_oracle(g, KC.oracle_loop())


@functools.lru_cache(maxsize=None)
def _rig_oracle():
    """The oracle-backend loop fed the rig's pairs rectified outside (apply_ref), no rectifier inside."""
    from pipeline_oracle import OracleBackend

    rig, frames = C.rig_sequence()
    _, K, p0, v, _ = KC.sequence()
    vo = PL.WindowedStereoVO(KC.loop_config(), OracleBackend(), K, p0, v, log_events=True)
    return C.run_raw(vo, [rig.apply_ref(L, R) for L, R in frames])


@pytest.mark.parametrize("kind", ["native", "python"])
def test_loop_with_two_different_cameras_rectifies_as_outside(ctx, oracle, kind):
    """8b: raw images of 600 x 452 and 704 x 520, each camera its own model
    (k1 +0.02 / -0.02, small tangential terms, 0.2 degree rotations): the GPU
    loop that rectifies inside holds what the oracle loop holds that was fed
    apply_ref's output.  Not vacuous: the oracle loop tracks 135 features at
    the last keyframe, the plain config-1 loop 163."""
    o = _rig_oracle()
    plain = KC.oracle_loop()
    assert 2 * o.results[-1].n_tracked >= plain.results[-1].n_tracked > 0, (o.results[-1], plain.results[-1])
    rig = C.rig_sequence()[0]
    assert rig.left.shape != rig.right.shape and rig.left.shape != rig.out.shape
    g = gpu_loop(ctx, kind, "rig", rectify=rig)
    check_against_oracle(g, o)


def test_native_setter_after_the_first_keyframe_is_a_state_error(ctx):
    fr, K, p0, v, _ = KC.sequence()
    rig = _padded_rig()
    cl, cr = rig.left.to_c(), rig.right.to_c()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        lib = g.lib
        assert lib.me_vo_loop_set_rectify(g.h, ctypes.byref(cl), ctypes.byref(cr), 0) == 0  # before: any number of times
        assert lib.me_vo_loop_set_rectify(g.h, None, None, 0) == 0
        assert lib.me_vo_loop_set_rectify(g.h, ctypes.byref(cl), None, 0) == -1
        assert b"both" in lib.me_vo_loop_last_error(g.h)
        assert lib.me_vo_loop_set_rectify(g.h, ctypes.byref(cl), ctypes.byref(cr), 256) == -1
        assert b"border" in lib.me_vo_loop_last_error(g.h)
        bad = rig.left.to_c()
        bad.fx = float("nan")
        assert lib.me_vo_loop_set_rectify(g.h, ctypes.byref(bad), ctypes.byref(cr), 0) == -1
        assert b"fx" in lib.me_vo_loop_last_error(g.h)
        g.process(0, fr[0].left, fr[0].right)  # (the failed calls left it off: plain frames)
        assert lib.me_vo_loop_set_rectify(g.h, ctypes.byref(cl), ctypes.byref(cr), 0) == -5  # ME_ERR_STATE
        assert b"before the first" in lib.me_vo_loop_last_error(g.h)
        assert lib.me_vo_loop_set_rectify(g.h, None, None, 0) == -5
        g.finish()
    finally:
        g.close()


def test_wrong_raw_sizes_are_refused(ctx):
    import torch

    fr, K, p0, v, _ = KC.sequence()
    rig, frames = C.rig_sequence()
    L, R = frames[0]
    g = PL.NativeStereoVO(KC.loop_config(rectify=rig), ctx, K, p0, v, overlap=False)
    try:
        for a, b, word in [(fr[0].left, R, "left"), (L, fr[0].right, "right"), (R, L, "left"), (L[:-1], R, "left")]:
            with pytest.raises(ValueError, match=word):
                g.process(0, a, b)
        with pytest.raises(ValueError, match="right"):
            g.process(0, torch.from_numpy(L).cuda(), torch.from_numpy(L).cuda())
        g.process(0, L, R)  # the refused calls left the loop untouched
        g.process(1, torch.from_numpy(frames[1][0]).cuda(), torch.from_numpy(frames[1][1]).cuda())
        g.finish()
        assert [r.n_tracked for r in g.results] == [r.n_tracked for r in _rig_oracle().results[:2]]
    finally:
        g.close()
    be = PL.GPUBackend(ctx)
    try:
        vo = PL.WindowedStereoVO(KC.loop_config(rectify=rig), be, K, p0, v)
        with pytest.raises(ValueError, match="left"):
            vo.process(0, fr[0].left, R)
        with pytest.raises(ValueError, match="right"):
            be.frame_images_device(0, torch.from_numpy(L).cuda(), torch.from_numpy(L).cuda())
    finally:
        be.close()
    # a rectifier whose model is not the loop's K
    K2 = np.array(K, np.float64)
    K2[1, 1] *= 1.01
    with pytest.raises(ValueError, match="K"):
        PL.NativeStereoVO(KC.loop_config(rectify=rig), ctx, K2, p0, v, overlap=False)


def test_null_models_restore_the_plain_loop(ctx):
    fr, K, p0, v, _ = KC.sequence()
    rig = _padded_rig()
    cl, cr = rig.left.to_c(), rig.right.to_c()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, log_events=True)
    try:
        assert g.lib.me_vo_loop_set_rectify(g.h, ctypes.byref(cl), ctypes.byref(cr), 0) == 0
        assert g.lib.me_vo_loop_set_rectify(g.h, None, None, 0) == 0
        C.run_raw(g, [(fr[t].left, fr[t].right) for t in range(KC.N_KEYFRAMES)])
        C.same_loop(snap(g), gpu_loop(ctx, "native", "plain"))
    finally:
        g.close()


# ------------------------------------------------------------------ 9. with the other switches
@pytest.mark.parametrize("kind", ["native", "python"])
def test_rectified_loop_with_corners_and_both_checks(ctx, kind):
    """The rectified buffers are the images every later stage reads: the
    corner detector, the forward-backward KLT and the left-right matcher on
    the padded frames give the plain loop's results with the same switches."""
    sw = dict(detector="corners", klt_fb_max=0.5, match_lr_max=1.0)
    plain = gpu_loop(ctx, kind, "plain", **sw)
    g = gpu_loop(ctx, kind, "padded", rectify=_padded_rig(), **sw)
    assert g.results[-1].n_tracked > 0 and any(e[0] == "add" for e in g.events)
    C.same_loop(g, plain)
