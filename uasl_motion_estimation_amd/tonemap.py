"""16-bit ingest (include/me_hip.h, section A12g): a 16 -> 8-bit tone map ahead
of the VO loop -- a percentile window with a minimum span, a temporal filter
on the window and a rounded linear map.

The definition is this library's own and integer-only: it restates no OpenCV
function and parity is unpinned.  tonemap_ref restates the header in numpy and
Python integers: it is the checker of the device kernels (csrc/tonemap.hip) and
the tone map the host backends run.  tonemap is the binding of me_tonemap16;
ToneMap holds the parameters and is what PipelineConfig.tonemap takes;
ToneMapState is a device state (me_tonemap_state).  Image and state are
bit-exact.

The defaults (1000, 1000, 256, 64) are a choice, not a measurement."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import ME_DEVICE, ME_HOST, Context, ToneMapParamsC, default_context

INT32_MAX = 2 ** 31 - 1


@dataclass(frozen=True)
class ToneMap:
    """me_tonemap_params: parts per million of the pixels below / above the
    window (>= 0, their sum below 10^6), the window's minimum span in counts
    (1 .. 65535) and the weight of a new frame's window in 1/256 (1 .. 256;
    256: no memory)."""
    lo_ppm: int = 1000
    hi_ppm: int = 1000
    min_span: int = 256
    alpha_q8: int = 64

    def __post_init__(self):
        for name in ("lo_ppm", "hi_ppm", "min_span", "alpha_q8"):
            v = getattr(self, name)
            if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool)):
                raise ValueError(f"{name} must be an integer")
        if self.lo_ppm < 0:
            raise ValueError("lo_ppm must be >= 0")
        if self.hi_ppm < 0:
            raise ValueError("hi_ppm must be >= 0")
        if self.lo_ppm + self.hi_ppm >= 10 ** 6:
            raise ValueError("lo_ppm + hi_ppm must be < 10^6")
        if not 1 <= self.min_span <= 65535:
            raise ValueError("min_span must be in 1 .. 65535")
        if not 1 <= self.alpha_q8 <= 256:
            raise ValueError("alpha_q8 must be in 1 .. 256")

    def to_c(self) -> ToneMapParamsC:
        return ToneMapParamsC(int(self.lo_ppm), int(self.hi_ppm), int(self.min_span), int(self.alpha_q8))


def _image16(img, what="img"):
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint16 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what} must be a (h, w) uint16 image, h and w >= 1")
    return a


# ------------------------------------------------------------------ the definition
def frame_ranks(img16, params: ToneMap):
    """Step 1 of the header: (lo, hi), the two order statistics of one frame, Python integers."""
    a = _image16(img16)
    n = a.size
    c = np.cumsum(np.bincount(a.ravel(), minlength=65536).astype(np.int64))
    k_lo, k_hi = params.lo_ppm * n // 10 ** 6, params.hi_ppm * n // 10 ** 6
    lo = int(np.searchsorted(c, k_lo, side="right"))  # the smallest v with c[v] > k_lo
    hi = int(np.searchsorted(c, n - k_hi, side="left"))  # the smallest v with c[v] >= N - k_hi
    return lo, hi


def frame_window(img16, params: ToneMap):
    """Steps 1 and 2 of the header: (lo, hi) of one frame, at least min_span apart."""
    lo, hi = frame_ranks(img16, params)
    s = hi - lo
    if s < params.min_span:
        lo -= (params.min_span - s) // 2  # (non-negative operands: C division)
        if lo < 0:
            lo = 0
        hi = lo + params.min_span
        if hi > 65535:
            hi, lo = 65535, 65535 - params.min_span
    return lo, hi


def filter_state(lo, hi, params: ToneMap, state=None):
    """Step 3: the state (lo_q8, hi_q8, frames) after a frame whose window is (lo, hi)."""
    if state is None or state[2] == 0:
        lo_q8, hi_q8, frames = lo << 8, hi << 8, 0
    else:
        lo_q8, hi_q8, frames = (int(v) for v in state)
        lo_q8 += ((lo << 8) - lo_q8) * params.alpha_q8 >> 8  # (Python's >> floors)
        hi_q8 += ((hi << 8) - hi_q8) * params.alpha_q8 >> 8
    return lo_q8, hi_q8, min(frames + 1, INT32_MAX)


def window_used(state):
    """Step 4: (lo_u, hi_u, span) of a state."""
    lo_u, hi_u = state[0] >> 8, (state[1] + 255) >> 8
    return lo_u, hi_u, max(1, hi_u - lo_u)


def tonemap_ref(img16, params: ToneMap | None = None, state=None):
    """me_tonemap16 restated: `img16` (h, w) uint16 (any strides), `state`
    None (frames = 0) or (lo_q8, hi_q8, frames) -> (img8 (h, w) uint8, state)."""
    params = params or ToneMap()
    a = _image16(img16)
    lo, hi = frame_window(a, params)
    state = filter_state(lo, hi, params, state)
    lo_u, hi_u, span = window_used(state)
    v = a.astype(np.int64)
    q = (np.minimum(v, hi_u) - lo_u) * 255 + span // 2
    out = np.where(v < lo_u, 0, np.minimum(255, q // span))
    return out.astype(np.uint8), state


# ------------------------------------------------------------------ the device
class ToneMapState:
    """A me_tonemap_state of `ctx`: the window's filter state on the device."""

    def __init__(self, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.me_tonemap_state_create(self.ctx.h, ctypes.byref(h)), "me_tonemap_state_create")
        self.h = h

    def reset(self):
        self.ctx.check(self.ctx.lib.me_tonemap_state_reset(self.h), "me_tonemap_state_reset")

    def read(self):
        out = (ctypes.c_int32 * 3)()
        self.ctx.check(self.ctx.lib.me_tonemap_state_read(self.h, out), "me_tonemap_state_read")
        return int(out[0]), int(out[1]), int(out[2])

    def close(self):
        if getattr(self, "h", None) is not None:
            if getattr(self.ctx, "h", None):  # (a closed ctx took its streams along: nothing left to free through)
                self.ctx.lib.me_tonemap_state_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rows16(a, what):
    """(array, stride in elements) of a (h, w) uint16 image with contiguous
    rows (a padded buffer's view keeps its padding); anything else is copied."""
    a = _image16(a, what)
    h, w = a.shape
    if not (a.strides[1] == 2 and (h == 1 or (a.strides[0] >= 2 * w and a.strides[0] % 2 == 0))):
        a = np.ascontiguousarray(a)
    return a, (int(a.strides[0]) // 2 if h > 1 else w)


def _span(a, stride):
    """The elements from the first to the last pixel of a strided image, as a flat view."""
    h, w = a.shape
    return np.lib.stride_tricks.as_strided(a, shape=(stride * (h - 1) + w,), strides=(a.itemsize,))


def tonemap(img16, params: ToneMap | None = None, ctx: Context | None = None, state: ToneMapState | None = None,
            device: bool = False, out=None):
    """me_tonemap16.  `img16`: (h, w) uint16, a view into a padded buffer keeps
    its row stride (and its base address); `out`: optional (h, w) uint8 view to
    write (its padding is not touched), else a new array.  `state`: a
    ToneMapState of `ctx`, or None (stateless).  device=False runs the ME_HOST
    form (staged by the library), device=True the ME_DEVICE form on uploaded
    copies that keep the source's offset from a 16-byte boundary."""
    ctx = ctx or default_context()
    params = params or ToneMap()
    src, s_stride = _rows16(img16, "img16")
    h, w = src.shape
    if out is None:
        out = np.zeros((h, w), np.uint8)
    if out.shape != (h, w) or out.dtype != np.uint8 or out.strides[1] != 1 or not out.flags.writeable:
        raise ValueError("out must be a writeable (h, w) uint8 array with contiguous rows")
    d_stride = int(out.strides[0]) if h > 1 else w
    if d_stride < w:
        raise ValueError("out: row stride below the width")
    pc = params.to_c()
    V = ctypes.c_void_p
    sh = state.h if state is not None else None
    if not device:
        ctx.check(ctx.lib.me_tonemap16(ctx.h, ME_HOST, V(src.ctypes.data), w, h, s_stride, V(out.ctypes.data),
                                       d_stride, ctypes.byref(pc), sh), "me_tonemap16")
        return out
    s_flat, o_flat = _span(src, s_stride), _span(out, d_stride)
    s_off, o_off = src.ctypes.data % 16, out.ctypes.data % 8  # device allocations are aligned: keep the views' offsets
    bufs = [ctx.malloc(s_flat.nbytes + 16), ctx.malloc(o_flat.nbytes + 8)]
    try:
        d_src, d_out = bufs[0] + s_off, bufs[1] + o_off
        ctx.h2d(d_src, s_flat)
        ctx.h2d(d_out, o_flat)  # (the padding's bytes travel both ways: the kernel must leave them alone)
        ctx.check(ctx.lib.me_tonemap16(ctx.h, ME_DEVICE, V(d_src), w, h, s_stride, V(d_out), d_stride,
                                       ctypes.byref(pc), sh), "me_tonemap16")
        ctx.synchronize()
        back = np.empty(o_flat.shape, np.uint8)
        ctx.d2h(back, d_out)
        o_flat[:] = back
    finally:
        for b in bufs:
            ctx.free(b)
    return out


def tonemap_device(ctx: Context, params: ToneMap, state: ToneMapState | None, d_src: int, width: int, height: int,
                   d_dst: int):
    """One me_tonemap16 queued on ctx's stream: a dense device image -> a dense device image."""
    pc = params.to_c()
    V = ctypes.c_void_p
    ctx.check(ctx.lib.me_tonemap16(ctx.h, ME_DEVICE, V(d_src), width, height, width, V(d_dst), width, ctypes.byref(pc),
                                   state.h if state is not None else None), "me_tonemap16")
