"""Local contrast equalisation (include/me_hip.h, section A12e): a
contrast-limited adaptive histogram equalisation (CLAHE) of an 8-bit image,
ahead of the VO loop's tracker.

The definition is build-defined and integer-only: OpenCV's float CLAHE is not
restated and parity with it is unpinned.  clahe_ref restates the header in
numpy (int64): it is the checker of the device kernels (csrc/clahe.hip) and
the equalisation the host backends run.  clahe is the binding of me_clahe;
Clahe holds the parameters and is what PipelineConfig.equalise takes.  Image
and tables are bit-exact."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import ME_DEVICE, ME_HOST, ClaheParamsC, Context, default_context

MAX_TILES = 16
MAX_AREA = 2 ** 20


@dataclass(frozen=True)
class Clahe:
    """me_clahe_params: tiles_x x tiles_y tiles (1 .. 16 each, and at most the
    image's width / height) and the clip limit (finite, >= 0; 0: no clipping)."""
    tiles_x: int = 8
    tiles_y: int = 8
    clip_limit: float = 3.0

    def __post_init__(self):
        for name in ("tiles_x", "tiles_y"):
            v = getattr(self, name)
            if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= v <= MAX_TILES):
                raise ValueError(f"{name} must be an integer in 1 .. {MAX_TILES}")
        try:
            clip = float(self.clip_limit)
        except (TypeError, ValueError):
            raise ValueError("clip_limit must be a finite number >= 0") from None
        if not (math.isfinite(clip) and clip >= 0.0):
            raise ValueError("clip_limit must be a finite number >= 0")

    def check_size(self, width: int, height: int, who: str = "Clahe"):
        """The checks of me_clahe that need the image's size; returns (tw, th)."""
        if width < 1 or height < 1:
            raise ValueError(f"{who}: width and height must be >= 1")
        if self.tiles_x > width:
            raise ValueError(f"{who}: tiles_x must be in 1 .. min(width, {MAX_TILES}), got {self.tiles_x} for width {width}")
        if self.tiles_y > height:
            raise ValueError(f"{who}: tiles_y must be in 1 .. min(height, {MAX_TILES}), got {self.tiles_y} for height "
                             f"{height}")
        tw, th = -(-width // self.tiles_x), -(-height // self.tiles_y)
        if tw * th > MAX_AREA:
            raise ValueError(f"{who}: area (tile width * tile height) must be <= 2^20, got {tw * th}")
        return tw, th

    def to_c(self) -> ClaheParamsC:
        c = ClaheParamsC()
        c.tiles_x, c.tiles_y, c.clip_limit = int(self.tiles_x), int(self.tiles_y), float(self.clip_limit)
        return c


def clip_count(clip_limit: float, area: int) -> int:
    """lim of the header: FP64, once."""
    if clip_limit == 0.0:
        return area
    q = float(clip_limit) * float(area) / 256.0
    if q >= float(area):
        return area
    return max(1, int(math.floor(q)))


def _image(img, what="img"):
    a = np.asarray(img)
    if a.ndim != 2 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what} must be a (h, w) uint8 image, h and w >= 1")
    return a


# ------------------------------------------------------------------ the definition
def clahe_tables_ref(img, params: Clahe | None = None):
    """(hist, lut): the clipped and redistributed histograms (tiles_y,
    tiles_x, 256) int64 and the tables (tiles_y, tiles_x, 256) uint8."""
    params = params or Clahe()
    a = _image(img)
    h, w = a.shape
    tx, ty = int(params.tiles_x), int(params.tiles_y)
    tw, th = params.check_size(w, h, "clahe_ref")
    area = tw * th
    lim = clip_count(float(params.clip_limit), area)
    xi, yi = np.arange(tw * tx), np.arange(th * ty)
    xi = np.where(xi >= w, 2 * (w - 1) - xi, xi)  # reflect-101
    yi = np.where(yi >= h, 2 * (h - 1) - yi, yi)
    ext = a[yi][:, xi].astype(np.int64)
    tiles = ext.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, area)
    idx = tiles + 256 * np.arange(ty * tx, dtype=np.int64)[:, None]
    hist = np.bincount(idx.ravel(), minlength=256 * ty * tx).reshape(ty * tx, 256).astype(np.int64)
    excess = np.maximum(hist - lim, 0).sum(axis=1)
    hist = np.minimum(hist, lim) + (excess // 256)[:, None]
    r = excess % 256
    step = np.maximum(256 // np.maximum(r, 1), 1)
    bins = np.arange(256, dtype=np.int64)[None, :]
    hist = hist + ((r[:, None] > 0) & (bins % step[:, None] == 0) & (bins // step[:, None] < r[:, None]))
    c = np.cumsum(hist, axis=1)
    lut = (255 * c + area // 2) // area
    return hist.reshape(ty, tx, 256), lut.astype(np.uint8).reshape(ty, tx, 256)


def clahe_ref(img, params: Clahe | None = None):
    """me_clahe restated: `img` (h, w) uint8 (any strides) -> (out (h, w)
    uint8, lut (tiles_y, tiles_x, 256) uint8).  int64 arithmetic."""
    params = params or Clahe()
    a = _image(img)
    h, w = a.shape
    tx, ty = int(params.tiles_x), int(params.tiles_y)
    tw, th = params.check_size(w, h, "clahe_ref")
    _, lut = clahe_tables_ref(a, params)

    def axis(n, t, tiles):
        p = 2 * np.arange(n, dtype=np.int64) + 1 - t
        k0 = p // (2 * t)  # floor
        f = p - k0 * 2 * t
        return np.clip(k0, 0, tiles - 1), np.clip(k0 + 1, 0, tiles - 1), f

    i0, i1, fx = (v[None, :] for v in axis(w, tw, tx))
    j0, j1, fy = (v[:, None] for v in axis(h, th, ty))
    L = lut.astype(np.int64)
    v = a.astype(np.int64)
    top = L[j0, i0, v] * (2 * tw - fx) + L[j0, i1, v] * fx
    bot = L[j1, i0, v] * (2 * tw - fx) + L[j1, i1, v] * fx
    out = (top * (2 * th - fy) + bot * fy + 2 * tw * th) // (4 * tw * th)
    return out.astype(np.uint8), lut


# ------------------------------------------------------------------ the device
def _span(a, stride):
    """The bytes from the first to the last pixel of a strided image, as a flat view."""
    h, w = a.shape
    return np.lib.stride_tricks.as_strided(a, shape=(stride * (h - 1) + w,), strides=(1,))


def _rows(a, what):
    """(array, stride) of a (h, w) uint8 image with contiguous rows (a padded
    buffer's view keeps its padding); anything else is copied to a dense array."""
    a = _image(a, what)
    h, w = a.shape
    if not (a.strides[1] == 1 and (h == 1 or a.strides[0] >= w)):
        a = np.ascontiguousarray(a)
    return a, (int(a.strides[0]) if h > 1 else w)


def clahe(img, params: Clahe | None = None, ctx: Context | None = None, device: bool = False, out=None,
          lut: bool = False):
    """me_clahe.  `img`: (h, w) uint8, a view into a padded buffer keeps its
    row stride; `out`: optional (h, w) uint8 view to write (its padding is not
    touched; a view of `img`'s own memory with its strides runs in place:
    dst == src), else a new array.  Returns the image, or (image, tables
    (tiles_y, tiles_x, 256) uint8) with lut=True.
    device=False runs the ME_HOST form (staged by the library), device=True the
    ME_DEVICE form on uploaded copies."""
    ctx = ctx or default_context()
    params = params or Clahe()
    src, s_stride = _rows(img, "img")
    # in place: `out` is the source's own memory with the source's row stride (the same view, or another view of it)
    in_place = (isinstance(out, np.ndarray) and out.shape == src.shape and out.ctypes.data == src.ctypes.data
                and out.strides == src.strides)
    h, w = src.shape
    params.check_size(w, h, "clahe")
    if out is None:
        out = np.zeros((h, w), np.uint8)
    if out.shape != (h, w) or out.dtype != np.uint8 or out.strides[1] != 1 or not out.flags.writeable:
        raise ValueError("out must be a writeable (h, w) uint8 array with contiguous rows")
    d_stride = int(out.strides[0]) if h > 1 else w
    if d_stride < w:
        raise ValueError("out: row stride below the width")
    tables = np.full((params.tiles_y, params.tiles_x, 256), 0xEE, np.uint8) if lut else None
    pc = params.to_c()
    V = ctypes.c_void_p
    if not device:
        ctx.check(ctx.lib.me_clahe(ctx.h, ME_HOST, V(src.ctypes.data), w, h, s_stride, ctypes.byref(pc),
                                   V(out.ctypes.data), d_stride, V(tables.ctypes.data) if lut else None), "me_clahe")
        return (out, tables) if lut else out
    s_flat, o_flat = _span(src, s_stride), _span(out, d_stride)
    bufs = [ctx.malloc(s_flat.nbytes)]
    try:
        ctx.h2d(bufs[0], s_flat)
        if in_place:
            d_out = bufs[0]
        else:
            bufs.append(ctx.malloc(o_flat.nbytes))
            d_out = bufs[-1]
            ctx.h2d(d_out, o_flat)  # (the padding's bytes travel both ways: the kernel must leave them alone)
        d_lut = None
        if lut:
            bufs.append(ctx.malloc(tables.nbytes))
            d_lut = bufs[-1]
        ctx.check(ctx.lib.me_clahe(ctx.h, ME_DEVICE, V(bufs[0]), w, h, s_stride, ctypes.byref(pc), V(d_out), d_stride,
                                   V(d_lut) if lut else None), "me_clahe")
        ctx.synchronize()
        back = np.empty(o_flat.shape, np.uint8)
        ctx.d2h(back, d_out)
        o_flat[:] = back
        if lut:
            ctx.d2h(tables, d_lut)
    finally:
        for b in bufs:
            ctx.free(b)
    return (out, tables) if lut else out


def clahe_device(ctx: Context, params: Clahe, d_src: int, width: int, height: int, d_dst: int):
    """One me_clahe queued on ctx's stream: a dense device image -> a dense
    device image (d_dst == d_src: in place)."""
    pc = params.to_c()
    V = ctypes.c_void_p
    ctx.check(ctx.lib.me_clahe(ctx.h, ME_DEVICE, V(d_src), width, height, width, ctypes.byref(pc), V(d_dst), width,
                               None), "me_clahe")
