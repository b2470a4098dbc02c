"""16-bit ingest on the device (me_tonemap16, csrc/tonemap.hip) against the
numpy restatement (tonemap.tonemap_ref), bit for bit, image and state: ragged
and unaligned access, the radix select's cases, every numerator of a set of
spans in front of the apply kernel's division, states (filter, interleaving,
re-arming, both memory modes), the argument checks of the C ABI, the C++
mirror, and the loop switch -- PipelineConfig.tonemap on the Python GPU loop
and me_vo_loop_set_tonemap / me_vo_loop_process16 on the native loop -- against
the oracle loop with the same switch (which runs tonemap_ref: in-loop and
stand-alone bytes are the same bytes)."""
import ctypes
import subprocess

import numpy as np
import pytest

import klt_fb_cases as KC
import rectify_cases as RC
import tonemap_cases as TC
from test_rectify_gpu import check_against_oracle, snap
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd._lib import ToneMapParamsC
from uasl_motion_estimation_amd.equalise import Clahe
from uasl_motion_estimation_amd.tonemap import ToneMap, ToneMapState, tonemap, tonemap_ref

pytestmark = pytest.mark.gpu

FILL = 0xA5  # pre-fill of every destination buffer: padding must keep it


def offset_view(shape, dtype, off, align):
    """A (h, w) view whose first element sits `off` elements past an `align`-byte boundary, and its buffer."""
    h, w = shape
    item = np.dtype(dtype).itemsize
    buf = np.zeros(h * w + 2 * align, dtype)
    start = (-(buf.ctypes.data // item)) % (align // item) + off
    view = buf[start:start + h * w].reshape(h, w)
    assert view.ctypes.data % align == off * item
    return view, buf


def run_tonemap(ctx, img, params, layout="dense", device=False, state=None):
    """me_tonemap16 on a dense image, on views of padded buffers (stride = width
    + 3, source and destination) or on views one element past an aligned
    address; checks that source and padding kept their bytes."""
    h, w = img.shape
    if layout == "padded":
        sbuf = np.full((h, w + 3), 0xBEEF, np.uint16)
        sbuf[:, :w] = img
        dbuf = np.full((h, w + 3), FILL, np.uint8)
        got = tonemap(sbuf[:, :w], params, ctx, state=state, device=device, out=dbuf[:, :w])
        assert np.all(dbuf[:, w:] == FILL), "the destination's row padding was written"
        assert np.array_equal(sbuf[:, :w], img) and np.all(sbuf[:, w:] == 0xBEEF), "the source was written"
        return got.copy()
    if layout == "offset":
        src, sbuf = offset_view((h, w), np.uint16, 1, 16)
        src[:] = img
        dst, dbuf = offset_view((h, w), np.uint8, 1, 8)
        dbuf[:] = FILL
        before = dbuf.copy()
        got = tonemap(src, params, ctx, state=state, device=device, out=dst)
        dst_start = (dst.ctypes.data - dbuf.ctypes.data)
        assert np.array_equal(dbuf[:dst_start], before[:dst_start]) and np.all(dbuf[dst_start + h * w:] == FILL)
        return got.copy()
    return tonemap(np.array(img), params, ctx, state=state, device=device)


# ------------------------------------------------------------------ 1. access
@pytest.mark.parametrize("layout", ["dense", "padded", "offset"])
@pytest.mark.parametrize("size", TC.SIZES, ids=lambda s: "%dx%d" % s)
def test_ragged_and_unaligned_access(ctx, size, layout):
    w, h = size
    img = TC.noise14(w, h)
    for p in (ToneMap(), TC.EXACT, ToneMap(100000, 200000, 1, 256)):
        want, _ = tonemap_ref(img, p)
        for device in (True, False):
            got = run_tonemap(ctx, img, p, layout, device)
            assert np.array_equal(got, want), (p, device, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ 2. the select
@pytest.mark.parametrize("name", TC.SELECT_CASES)
def test_radix_select(ctx, name):
    img, p = TC.select_case(name)
    want, want_st = tonemap_ref(img, p)
    st = ToneMapState(ctx)
    try:
        for device in (True, False):
            st.reset()
            got = run_tonemap(ctx, img, p, "dense", device, state=st)
            assert st.read() == want_st, (device, st.read(), want_st)
            assert np.array_equal(got, want), (device, np.argwhere(got != want)[:4])
    finally:
        st.close()


# ------------------------------------------------------------------ 3. the division
def test_exact_division_for_every_numerator(ctx):
    """For each span: 256 x 257 pixels lo + (i mod (span + 1)), no clipping, no widening, no memory: the window is lo ..
    lo + span and every q of that span reaches the apply kernel."""
    for span in TC.SPANS:
        img = TC.division_image(span)
        want, st = tonemap_ref(img, TC.EXACT)
        assert (st[1] - st[0]) >> 8 == span
        got = tonemap(img, TC.EXACT, ctx, device=True)
        assert np.array_equal(got, want), (span, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ 4. states
def _stepped(k, w=70, h=45):
    """Frame k of a stream whose level steps: 14-bit noise squeezed to 600 counts on a level that jumps."""
    level = [7000, 7040, 9000, 9000, 6500, 6540][k]
    return (level + TC.noise14(w, h, seed=k) % 600).astype(np.uint16)


def test_six_calls_on_one_state_and_a_second_state_interleaved(ctx):
    p = ToneMap(1000, 1000, 256, 64)
    a, b = ToneMapState(ctx), ToneMapState(ctx)
    try:
        assert a.read() == (0, 0, 0)
        ra = rb = None
        for k in range(6):
            ia, ib = _stepped(k), _stepped(5 - k, 61, 7)
            want_a, ra = tonemap_ref(ia, p, ra)
            want_b, rb = tonemap_ref(ib, p, rb)
            got_a = tonemap(ia, p, ctx, state=a, device=bool(k & 1))  # (both memory modes feed one state)
            got_b = tonemap(ib, p, ctx, state=b, device=not (k & 1))
            assert a.read() == ra and b.read() == rb, (k, a.read(), ra, b.read(), rb)
            assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b), k
        assert ra[2] == 6
        a.reset()  # frames = 0: the next call starts a new window
        want, r0 = tonemap_ref(_stepped(2), p, None)
        got = tonemap(_stepped(2), p, ctx, state=a, device=True)
        assert a.read() == r0 and r0[2] == 1 and np.array_equal(got, want)
    finally:
        a.close()
        b.close()


def test_stateless_calls_repeat_and_both_memory_modes_agree(ctx):
    """NULL state: every call is frames = 0, whatever ran before on the ctx (tickets and tables re-armed)."""
    p = ToneMap()
    for k in (0, 2, 4, 2, 0, 0):
        img = _stepped(k, 300, 200)
        want, _ = tonemap_ref(img, p)
        dev, host = tonemap(img, p, ctx, device=True), tonemap(img, p, ctx, device=False)
        assert np.array_equal(dev, host) and np.array_equal(dev, want), k


def test_in_loop_and_stand_alone_give_the_same_bytes(ctx):
    """The 8-bit pairs GPUBackend.frame_images makes of three 16-bit keyframes (host arrays, then device tensors) are
    the bytes of stand-alone me_tonemap16 calls on a state per camera, and tonemap_ref's."""
    import torch

    p = ToneMap()
    frames = [(_stepped(k, 70, 45), _stepped(k + 3, 70, 45)) for k in range(3)]
    sl, sr = ToneMapState(ctx), ToneMapState(ctx)
    alone, rl, rr = [], None, None
    try:
        for L, R in frames:
            alone.append((tonemap(L, p, ctx, state=sl, device=True), tonemap(R, p, ctx, state=sr, device=True)))
            wl, rl = tonemap_ref(L, p, rl)
            wr, rr = tonemap_ref(R, p, rr)
            assert np.array_equal(alone[-1][0], wl) and np.array_equal(alone[-1][1], wr)
    finally:
        sl.close()
        sr.close()
    for tensors in (False, True):
        be = PL.GPUBackend(ctx)
        be.tonemapper = p
        try:
            for t, (L, R) in enumerate(frames):
                if tensors:
                    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
                    h = be.frame_images_device(t, dl, dr)
                else:
                    h = be.frame_images(t, L, R)
                be.tctx.synchronize()
                for side in (0, 1):
                    got = np.zeros(L.shape, np.uint8)
                    be.tctx.d2h(got, h[side])
                    assert np.array_equal(got, alone[t][side]), (tensors, t, side)
                be.release(t)
        finally:
            be.close()


def test_backend_refuses_a_bad_uint16_pair_before_it_allocates(ctx, monkeypatch):
    import torch

    L, R = _stepped(0, 70, 45), _stepped(1, 70, 45)
    be = PL.GPUBackend(ctx)
    try:
        def no_malloc(n):
            raise AssertionError("allocated before the checks")

        monkeypatch.setattr(be.tctx, "malloc", no_malloc)
        with pytest.raises(ValueError, match="tonemap"):  # the switch is off
            be.frame_images(0, L, R)
        be.tonemapper = ToneMap()
        for bad, word in [(R[:, :-1], "right"), (R.astype(np.uint8), "uint8")]:
            with pytest.raises(ValueError, match=word):
                be.frame_images(0, L, bad)
        dl = torch.from_numpy(L).cuda()
        for bad, word in [(torch.from_numpy(R.astype(np.uint8)).cuda(), "right"), (torch.from_numpy(R).cuda()[:, ::2], "right"),
                          (torch.from_numpy(R[:-1]).cuda(), "right")]:
            with pytest.raises(ValueError, match=word):
                be.frame_images_device(0, dl, bad)
        assert not be._imgs and not be._raw
    finally:
        monkeypatch.undo()
        be.close()


# ------------------------------------------------------------------ 5. arguments
def test_tonemap16_rejects_bad_arguments(ctx):
    src = np.array(TC.noise14(33, 17))
    dst = np.zeros((17, 33), np.uint8)
    V = ctypes.c_void_p

    def call(w=33, h=17, ss=33, ds=33, lo=1000, hi=1000, span=256, alpha=64, s=src, d=dst, params=True):
        pc = ToneMapParamsC(lo, hi, span, alpha)
        rc = ctx.lib.me_tonemap16(ctx.h, 0, V(s.ctypes.data) if s is not None else None, w, h, ss,
                                  V(d.ctypes.data) if d is not None else None, ds,
                                  ctypes.byref(pc) if params else None, None)
        return rc, ctx.lib.me_last_error(ctx.h).decode()

    assert call()[0] == 0
    assert call(lo=0, hi=999999, span=1, alpha=1)[0] == 0 and call(span=65535, alpha=256)[0] == 0
    for kw, word in [(dict(s=None), "src"), (dict(d=None), "dst"), (dict(params=False), "params"),
                     (dict(w=0), "width"), (dict(h=0), "height"), (dict(ss=32), "src_stride"),
                     (dict(ds=32), "dst_stride"), (dict(lo=-1), "lo_ppm"), (dict(hi=-1), "hi_ppm"),
                     (dict(lo=500000, hi=500000), "lo_ppm + hi_ppm"), (dict(span=0), "min_span"),
                     (dict(span=65536), "min_span"), (dict(alpha=0), "alpha_q8"), (dict(alpha=257), "alpha_q8"),
                     (dict(ss=2 ** 26, ds=2 ** 26), "src_stride * height"), (dict(ds=2 ** 26), "dst_stride * height")]:
        rc, msg = call(**kw)  # (every one is refused before anything is read)
        assert rc == -1 and word in msg, (kw, msg)
    assert ctx.lib.me_tonemap16(None, 0, V(src.ctypes.data), 33, 17, 33, V(dst.ctypes.data), 33, None, None) == -1
    # a state of another ctx
    from uasl_motion_estimation_amd._lib import Context

    other = Context(0)
    st = ToneMapState(other)
    try:
        pc = ToneMap().to_c()
        rc = ctx.lib.me_tonemap16(ctx.h, 0, V(src.ctypes.data), 33, 17, 33, V(dst.ctypes.data), 33, ctypes.byref(pc), st.h)
        assert rc == -1 and "state" in ctx.lib.me_last_error(ctx.h).decode()
    finally:
        st.close()
        other.close()
    assert ctx.lib.me_tonemap_state_create(ctx.h, None) == -1 and ctx.lib.me_tonemap_state_reset(None) == -1
    assert ctx.lib.me_tonemap_state_read(None, (ctypes.c_int32 * 3)()) == -1


def test_default_params(ctx):
    pc = ToneMapParamsC(0, 0, 0, 0)
    ctx.lib.me_tonemap_default_params(ctypes.byref(pc))
    d = ToneMap()
    assert (pc.lo_ppm, pc.hi_ppm, pc.min_span, pc.alpha_q8) == (1000, 1000, 256, 64) == \
        (d.lo_ppm, d.hi_ppm, d.min_span, d.alpha_q8)


def test_cpp_mirror(ctx, tmp_path):
    exe = TC.build_cli(tmp_path)
    w, h, step = 97, 53, 100
    img, p = TC.select_case("adjacent_high_bytes")
    buf = np.full((h, step), 0xBEEF, np.uint16)
    buf[:, :w] = img
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([w, h, step, p.lo_ppm, p.hi_ppm, p.min_span, p.alpha_q8], np.int32).tobytes() + buf.tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    assert raw.size == w * h + 3
    assert np.array_equal(raw[:w * h].reshape(h, w), tonemap_ref(img, p)[0])
    assert list(raw[w * h:]) == [1, 1, 1]  # process16 without the switch, bad parameters, set / clear


# ------------------------------------------------------------------ 6. the loops
WIDE_PAD = 7300  # the border of the padded 16-bit frames: inside the scene's range, so that the window stays on it


def _frames(frames_id):
    if frames_id == "wide":
        return TC.wide_sequence()
    if frames_id == "wide_padded":
        pad = lambda a: np.pad(a, ((RC.PAD[1], RC.PAD[1]), (RC.PAD[0], RC.PAD[0])), constant_values=WIDE_PAD)
        return [(pad(L), pad(R)) for L, R in TC.wide_sequence()]
    fr = KC.sequence()[0]
    return [(fr[t].left, fr[t].right) for t in range(KC.N_KEYFRAMES)]


def gpu_loop(ctx, kind, frames_id, tensors=False, **cfg_kw):
    """A config-1 loop on the GPU (kind "native" / "python"); with tensors=True the frames are the caller's device
    tensors, which must come back unchanged."""
    _, K, p0, v, _ = KC.sequence()
    frames = _frames(frames_id)
    cfg = KC.loop_config(**cfg_kw)
    if tensors:
        import torch

        dev = [(torch.from_numpy(np.array(L)).cuda(), torch.from_numpy(np.array(R)).cuda()) for L, R in frames]
    if kind == "native":
        g = PL.NativeStereoVO(cfg, ctx, K, p0, v, log_events=True)
        try:
            out = snap(TC.run_frames(g, dev if tensors else frames))
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
                TC.run_frames(vo, frames)
            out = snap(vo)
        finally:
            be.close()
    if tensors:
        for (dL, dR), (L, R) in zip(dev, frames):
            assert np.array_equal(dL.cpu().numpy(), L) and np.array_equal(dR.cpu().numpy(), R), \
                "the caller's device images were written"
    return out


@pytest.mark.parametrize("tensors", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("kind", ["native", "python"])
def test_loop_on_the_16_bit_stream_is_the_oracle_loop(ctx, oracle, kind, tensors):
    o = TC.oracle_loop("wide", tonemap=ToneMap())
    assert o.results[-1].n_tracked >= 100
    g = gpu_loop(ctx, kind, "wide", tensors=tensors, tonemap=ToneMap())
    check_against_oracle(g, o)


@pytest.mark.parametrize("kind", ["native", "python"])
def test_tone_map_then_remap_then_clahe(ctx, oracle, kind):
    """Padded 16-bit frames + the cropping rectifier + equalise + tonemap against the oracle backend with the same
    switches, which maps (tonemap_ref), then warps (apply_ref), then equalises (clahe_ref): the order is fixed."""
    from pipeline_oracle import OracleBackend

    cfg0 = KC.loop_config()
    rig = RC.padded_rectifier(cfg0.width, cfg0.height, KC.sequence()[1])
    sw = dict(rectify=rig, equalise=Clahe(), tonemap=ToneMap())
    key = "wide_padded_oracle"
    if key not in TC._RUNS:
        _, K, p0, v, _ = KC.sequence()
        vo = PL.WindowedStereoVO(KC.loop_config(**sw), OracleBackend(), K, p0, v, log_events=True)
        TC._RUNS[key] = TC.run_frames(vo, _frames("wide_padded"))
    o = TC._RUNS[key]
    assert o.results[-1].n_tracked > 0 and any(e[0] == "add" for e in o.events)
    g = gpu_loop(ctx, kind, "wide_padded", **sw)
    check_against_oracle(g, o)


def test_native_entry_points_and_their_state_errors(ctx):
    fr, K, p0, v, _ = KC.sequence()
    wide = TC.wide_sequence()
    V = ctypes.c_void_p

    def p16(g, t, pair):
        return g.lib.me_vo_loop_process16(g.h, t, V(pair[0].ctypes.data), V(pair[1].ctypes.data), 0)

    # without the switch: process16 is a state error and leaves the loop usable
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        lib = g.lib
        assert p16(g, 0, wide[0]) == -5 and b"me_vo_loop_set_tonemap" in lib.me_vo_loop_last_error(g.h)
        ok = ToneMap().to_c()
        assert lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(ok)) == 0  # before: any number of times
        assert lib.me_vo_loop_set_tonemap(g.h, None) == 0
        for bad, word in [(ToneMapParamsC(-1, 0, 256, 64), b"lo_ppm"), (ToneMapParamsC(0, 10 ** 6, 256, 64), b"hi_ppm"),
                          (ToneMapParamsC(0, 0, 0, 64), b"min_span"), (ToneMapParamsC(0, 0, 256, 300), b"alpha_q8")]:
            assert lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(ok)) == 0
            assert lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(bad)) == -1
            assert word in lib.me_vo_loop_last_error(g.h)
            assert p16(g, 0, wide[0]) == -5  # (the failed call left it off)
        g.process(0, fr[0].left, fr[0].right)
        assert lib.me_vo_loop_set_tonemap(g.h, ctypes.byref(ok)) == -5  # ME_ERR_STATE
        assert b"before the first" in lib.me_vo_loop_last_error(g.h)
        g.process(1, fr[1].left, fr[1].right)
        g.finish()
        assert [r.n_tracked for r in g.results] == [r.n_tracked for r in KC.oracle_loop().results[:2]]
    finally:
        g.close()
    # with it: the two entries do not mix, in either order
    g = PL.NativeStereoVO(KC.loop_config(tonemap=ToneMap()), ctx, K, p0, v, overlap=False)
    try:
        g.process(0, *wide[0])
        rc = g.lib.me_vo_loop_process(g.h, 1, V(fr[1].left.ctypes.data), V(fr[1].right.ctypes.data), 0)
        assert rc == -5 and b"me_vo_loop_process16" in g.lib.me_vo_loop_last_error(g.h)
        g.process(1, *wide[1])  # (the refused call did not break the loop)
        g.finish()
        assert len(g.results) == 2
        with pytest.raises(ValueError, match="uint16"):
            g.process(2, wide[2][0][:, :-1], wide[2][1])
    finally:
        g.close()
    g = PL.NativeStereoVO(KC.loop_config(tonemap=ToneMap()), ctx, K, p0, v, overlap=False)
    try:
        g.process(0, fr[0].left, fr[0].right)  # 8-bit frames with the switch on: the plain entry
        assert p16(g, 1, wide[1]) == -5 and b"me_vo_loop_process" in g.lib.me_vo_loop_last_error(g.h)
    finally:
        g.close()
    # uint16 frames without the switch never reach the library
    g = PL.NativeStereoVO(KC.loop_config(), ctx, K, p0, v, overlap=False)
    try:
        with pytest.raises(ValueError, match="uint8"):
            g.process(0, *wide[0])
    finally:
        g.close()
