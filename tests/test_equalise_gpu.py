"""Local contrast equalisation on the device (me_clahe, csrc/clahe.hip) against
the numpy restatement (equalise.clahe_ref), bit for bit, image and tables:
every shape, image and clip limit of equalise_cases, both memory modes, in
place, with and without lut_out; the C++ mirror; and the loop switch --
PipelineConfig.equalise on the Python GPU loop and me_vo_loop_set_equalise on
the native loop -- against the oracle loop that was equalised outside."""
import ctypes
import subprocess

import numpy as np
import pytest

import equalise_cases as EC
import klt_fb_cases as KC
import rectify_cases as RC
from test_rectify_gpu import check_against_oracle, snap
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import ClaheParamsC
from uasl_motion_estimation_amd.equalise import Clahe, clahe, clahe_ref

pytestmark = pytest.mark.gpu

FILL = 0xA5  # pre-fill of every destination buffer: padding must keep it


def run_clahe(ctx, img, params, extra=0, device=False, lut=True, in_place=False):
    """me_clahe on a view of a padded source into a view of a buffer pre-filled
    with FILL (or in place); checks that the padding on both sides kept its bytes."""
    h, w = img.shape
    sbuf = np.full((h, w + extra), RC.PAD_VALUE, np.uint8)
    sbuf[:, :w] = img
    if in_place:  # dst == src with equal strides: the kernels read and write the same device bytes
        view = sbuf[:, :w]
        res = clahe(view, params, ctx, device=device, out=view, lut=lut)
        assert np.all(sbuf[:, w:] == RC.PAD_VALUE), "the row padding was written"
        got = sbuf[:, :w].copy()
    else:
        dbuf = np.full((h, w + extra), FILL, np.uint8)
        res = clahe(sbuf[:, :w], params, ctx, device=device, out=dbuf[:, :w], lut=lut)
        assert np.all(dbuf[:, w:] == FILL), "the destination's row padding was written"
        assert np.array_equal(sbuf[:, :w], img) and np.all(sbuf[:, w:] == RC.PAD_VALUE), "the source was written"
        got = dbuf[:, :w].copy()
    return got, (res[1] if lut else None)


# ------------------------------------------------------------------ 1. the primitive
@pytest.mark.parametrize("shape", EC.SHAPES, ids=EC.shape_id)
def test_clahe_matches_the_restatement(ctx, shape):
    w, h, tx, ty, extra = shape
    k = 0
    for name in EC.IMAGES:
        img = EC.image(name, w, h)
        for clip in EC.CLIPS:
            want, want_lut = EC.reference(name, shape, clip)
            p = Clahe(tx, ty, clip)
            # the host form for every case; the device form, in place and without lut_out in turn
            variants = [dict(device=False), [dict(device=True), dict(device=True, in_place=True),
                                             dict(device=False, in_place=True), dict(device=True, lut=False),
                                             dict(device=False, lut=False)][(k + k // 5) % 5]]  # (crosses with the clips)
            k += 1
            for kw in variants:
                got, lut = run_clahe(ctx, img, p, extra, **kw)
                if lut is not None:  # the tables first: a wrong table is not a wrong blend
                    assert lut.shape == (ty, tx, 256) and np.array_equal(lut, want_lut), \
                        (name, clip, kw, np.argwhere(lut != want_lut)[:4])
                assert np.array_equal(got, want), (name, clip, kw, np.argwhere(got != want)[:4])


def test_in_place_calls_run_with_dst_equal_to_src(ctx, monkeypatch):
    """What run_clahe(in_place=True) relies on: the binding hands me_clahe one
    pointer for both images and equal strides, in both memory modes (ME_HOST then
    runs the kernels in place on its staged copy); image, tables and the
    padding are compared bit for bit, on a staged-table shape and a
    global-gather one."""
    calls = []
    real = ctx.lib.me_clahe

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(ctx.lib, "me_clahe", spy)
    for shape in (EC.SHAPES[7], EC.SHAPES[8], EC.SHAPES[4]):  # 200 x 130 padded, 640 x 480, 64 x 48 with 16 x 16 tiles
        w, h, tx, ty, extra = shape
        for name in ("noise", "low"):
            want, want_lut = EC.reference(name, shape, 3.0)
            for device in (False, True):
                del calls[:]
                got, lut = run_clahe(ctx, EC.image(name, w, h), Clahe(tx, ty, 3.0), extra, device=device, in_place=True)
                (a,) = calls
                assert a[1] == int(device) and a[2].value == a[7].value and a[5] == a[8] == w + extra, a
                assert np.array_equal(lut, want_lut) and np.array_equal(got, want), (shape, name, device)


# (w, h, tiles_x, tiles_y): sizes at which me_clahe takes the four-rows-per-thread apply kernel on a whole MI355X
# (1 024 workgroups of 64 x 64 pixels and more), ragged in both directions; the first stages its tables, most of the
# second one's workgroups touch more than nine (tiles 19 pixels wide: 6 x 2 past the first column of workgroups) and
# gather from global memory
BIG = [(2050, 2061, 8, 8), (300, 13200, 16, 16)]


@pytest.mark.parametrize("big", BIG, ids=lambda b: "%dx%d_%dx%d" % b)
def test_large_images_take_the_four_row_kernel(ctx, big):
    w, h, tx, ty = big
    assert ctx.lib.me_clahe_apply_rows(ctx.h, w, h) == 4
    assert ctx.lib.me_clahe_apply_rows(ctx.h, 1280, 720) == 1 and ctx.lib.me_clahe_apply_rows(ctx.h, 0, 5) == -1
    img = np.array(EC.image("low", w, h))
    img[:, w // 2:] = EC.image("noise", w, h)[:, w // 2:]  # both kinds of content in one reference
    p = Clahe(tx, ty, 3.0)
    want, want_lut = clahe_ref(img, p)
    for kw in (dict(device=True), dict(device=True, in_place=True), dict(device=False)):
        got, lut = run_clahe(ctx, img, p, 3, **kw)
        assert np.array_equal(lut, want_lut), (kw, np.argwhere(lut != want_lut)[:4])
        assert np.array_equal(got, want), (kw, np.argwhere(got != want)[:4])


def test_hand_checks_on_the_device(ctx):
    c = np.full((48, 64), 77, np.uint8)
    assert np.all(clahe(c, Clahe(4, 4, 3.0), ctx) == 106)
    assert np.all(clahe(c, Clahe(4, 4, 0.0), ctx) == 255)
    a = np.zeros((4, 4), np.uint8)
    a[:, 2:] = 200
    got = clahe(a, Clahe(1, 1, 0.0), ctx)
    assert np.all(got[:, :2] == 128) and np.all(got[:, 2:] == 255)


def test_clahe_rejects_bad_arguments(ctx):
    src = np.array(EC.image("noise", 33, 17))
    dst = np.zeros((17, 33), np.uint8)
    V = ctypes.c_void_p

    def call(w=33, h=17, ss=33, ds=33, tx=8, ty=8, clip=3.0, s=src, d=dst, params=True):
        pc = ClaheParamsC(tx, ty, clip)
        rc = ctx.lib.me_clahe(ctx.h, 0, V(s.ctypes.data) if s is not None else None, w, h, ss,
                              ctypes.byref(pc) if params else None, V(d.ctypes.data) if d is not None else None, ds,
                              None)
        return rc, ctx.lib.me_last_error(ctx.h).decode()

    assert call()[0] == 0
    assert call(tx=16, ty=16)[0] == 0 and call(tx=1, ty=17 - 1)[0] == 0
    for kw, word in [(dict(w=0), "width"), (dict(h=0), "height"), (dict(ss=32), "src_stride"),
                     (dict(ds=32), "dst_stride"), (dict(tx=0), "tiles_x"), (dict(tx=17), "tiles_x"),
                     (dict(w=7, ss=33, tx=8), "tiles_x"), (dict(ty=0), "tiles_y"), (dict(ty=17), "tiles_y"),
                     (dict(h=5, ty=6), "tiles_y"), (dict(clip=-1.0), "clip_limit"),
                     (dict(clip=float("nan")), "clip_limit"), (dict(clip=float("inf")), "clip_limit"),
                     (dict(s=None), "src"), (dict(d=None), "dst"), (dict(params=False), "params")]:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # a stride too long for the image's height: its own message (refused before anything is read)
    rc, msg = call(ss=2 ** 27, ds=2 ** 27)
    assert rc == -1 and "src_stride * height" in msg, msg
    rc, msg = call(ds=2 ** 27)
    assert rc == -1 and "dst_stride * height" in msg, msg
    # area > 2^20: one tile of 2049 x 512 (refused before anything is read)
    rc, msg = call(w=2049, h=512, ss=2049, ds=2049, tx=1, ty=1)
    assert rc == -1 and "area" in msg, msg


def test_default_params(ctx):
    pc = ClaheParamsC(0, 0, 0.0)
    ctx.lib.me_clahe_default_params(ctypes.byref(pc))
    assert (pc.tiles_x, pc.tiles_y, pc.clip_limit) == (8, 8, 3.0) == (Clahe().tiles_x, Clahe().tiles_y, Clahe().clip_limit)


def test_cpp_mirror(ctx, tmp_path):
    exe = EC.build_cli(tmp_path)
    w, h, tx, ty, clip, step = 97, 61, 8, 8, 3.0, 100
    img = EC.image("low", w, h)
    buf = np.full((h, step), RC.PAD_VALUE, np.uint8)
    buf[:, :w] = img
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([w, h, step, tx, ty], np.int32).tobytes() + np.array([clip]).tobytes() + buf.tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    want, want_lut = clahe_ref(img, Clahe(tx, ty, clip))
    assert raw.size == w * h + ty * tx * 256
    assert np.array_equal(raw[w * h:].reshape(ty, tx, 256), want_lut)
    assert np.array_equal(raw[:w * h].reshape(h, w), want)


# ------------------------------------------------------------------ 2. the loops
_LOOPS = {}


def _frames(frames_id):
    fr = KC.sequence()[0]
    if frames_id == "low":
        return EC.low_sequence()
    if frames_id == "low_padded":
        return [(RC.pad_frame(L), RC.pad_frame(R)) for L, R in EC.low_sequence()]
    return [(fr[t].left, fr[t].right) for t in range(KC.N_KEYFRAMES)]


def gpu_loop(ctx, kind, frames_id, tensors=False, **cfg_kw):
    """A config-1 loop on the GPU (kind "native" / "python"), cached per (kind, input, switches)."""
    key = (kind, frames_id, tensors, tuple(sorted(cfg_kw.items(), key=lambda kv: kv[0])))
    if key in _LOOPS:
        return _LOOPS[key]
    _, K, p0, v, _ = KC.sequence()
    frames = _frames(frames_id)
    cfg = KC.loop_config(**cfg_kw)
    if tensors:  # device-resident frames of the caller's: they must come back unchanged
        import torch

        dev = [(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()) for L, R in frames]
    if kind == "native":
        g = PL.NativeStereoVO(cfg, ctx, K, p0, v, log_events=True)
        try:
            _LOOPS[key] = snap(EC.run_frames(g, dev if tensors else frames))
        finally:
            g.close()
    else:
        be = PL.GPUBackend(ctx)
        try:
            vo = PL.WindowedStereoVO(cfg, be, K, p0, v, log_events=True, overlap=True)
            if tensors:
                for t, (L, R) in enumerate(dev):
                    be.frame_images_device(t, L, R)
                    vo.process(t, None, None)
                vo.finish()
            else:
                EC.run_frames(vo, frames)
            _LOOPS[key] = snap(vo)
        finally:
            be.close()
    if tensors:
        for (dL, dR), (L, R) in zip(dev, frames):
            assert np.array_equal(dL.cpu().numpy(), L) and np.array_equal(dR.cpu().numpy(), R), \
                "the caller's device images were written"
    return _LOOPS[key]


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["native", "python"])
def test_loop_on_the_low_stream_equalises_as_outside(ctx, oracle, kind, tensors):
    """The low stream with the switch on holds what the oracle loop holds that
    was fed clahe_ref's output; host frames and the caller's device frames
    (which come back unchanged: gpu_loop checks it)."""
    o = EC.oracle_low_loop("outside")
    assert o.results[-1].n_tracked >= 100
    g = gpu_loop(ctx, kind, "low", tensors=tensors, equalise=Clahe())
    assert g.results[-1].n_tracked >= 100
    check_against_oracle(g, o)


@pytest.mark.parametrize("kind", ["native", "python"])
def test_rectified_equalised_loop_with_corners_and_both_checks(ctx, kind):
    """Padded frames + the cropping rectifier + equalise + corners + both
    checks = plain frames + equalise + the same switches: the remap runs
    first, and every later stage reads the equalised pair."""
    sw = dict(detector="corners", klt_fb_max=0.5, match_lr_max=1.0, equalise=Clahe())
    cfg = KC.loop_config()
    rig = RC.padded_rectifier(cfg.width, cfg.height, KC.sequence()[1])
    plain = gpu_loop(ctx, kind, "low", **sw)
    g = gpu_loop(ctx, kind, "low_padded", rectify=rig, **sw)
    assert g.results[-1].n_tracked > 0 and any(e[0] == "add" for e in g.events)
    RC.same_loop(g, plain)
    # not the unequalised loop's: the switch changed what the stages read
    off = gpu_loop(ctx, kind, "low", detector="corners", klt_fb_max=0.5, match_lr_max=1.0)
    assert [r.n_tracked for r in off.results] != [r.n_tracked for r in plain.results]


def test_native_setter_after_the_first_keyframe_is_a_state_error(ctx):
    fr, K, p0, v, _ = KC.sequence()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        lib = g.lib
        ok = Clahe().to_c()
        assert lib.me_vo_loop_set_equalise(g.h, ctypes.byref(ok)) == 0  # before: any number of times
        assert lib.me_vo_loop_set_equalise(g.h, None) == 0
        assert lib.me_vo_loop_set_equalise(g.h, ctypes.byref(ok)) == 0
        for bad, word in [(ClaheParamsC(0, 8, 3.0), b"tiles_x"), (ClaheParamsC(8, 17, 3.0), b"tiles_y"),
                          (ClaheParamsC(8, 8, -1.0), b"clip_limit"), (ClaheParamsC(8, 8, float("nan")), b"clip_limit")]:
            assert lib.me_vo_loop_set_equalise(g.h, ctypes.byref(bad)) == -1
            assert word in lib.me_vo_loop_last_error(g.h)
        g.process(0, fr[0].left, fr[0].right)  # (the failed calls left it off)
        assert lib.me_vo_loop_set_equalise(g.h, ctypes.byref(ok)) == -5  # ME_ERR_STATE
        assert b"before the first" in lib.me_vo_loop_last_error(g.h)
        assert lib.me_vo_loop_set_equalise(g.h, None) == -5
        g.process(1, fr[1].left, fr[1].right)
        g.finish()
        plain = KC.oracle_loop()
        assert [r.n_tracked for r in g.results] == [r.n_tracked for r in plain.results[:2]]
    finally:
        g.close()


def test_null_params_restore_the_plain_loop(ctx):
    fr, K, p0, v, _ = KC.sequence()
    ok = Clahe().to_c()
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, log_events=True)
    try:
        assert g.lib.me_vo_loop_set_equalise(g.h, ctypes.byref(ok)) == 0
        assert g.lib.me_vo_loop_set_equalise(g.h, None) == 0
        EC.run_frames(g, _frames("plain"))
        RC.same_loop(snap(g), gpu_loop(ctx, "native", "plain"))
    finally:
        g.close()
