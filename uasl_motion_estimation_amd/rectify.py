"""Stereo rectification (include/me_hip.h, section A12d): a fixed-point (Q5)
map built from a Brown-Conrady camera model and a rotation into the rectified
frame, and a bilinear 8-bit remap through any such map.

rectify_map_ref / remap_ref restate the definition in numpy (elementwise
float64 / int64, one rounding per operation, in the header's order): they are
the checker of the device kernels (csrc/rectify.hip) and the warp the host
backends run.  rectify_map / remap are the bindings of me_rectify_map /
me_remap_q5; StereoRectifier holds the two cameras of a rig and is what
PipelineConfig.rectify takes.  Both results are bit-exact."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import ME_DEVICE, ME_HOST, CameraModelC, Context, RectifiedModelC, default_context, load_library

SENTINEL = -(2 ** 31)  # both halves of a map entry without a source
LIMIT = float(2 ** 24)  # |source coordinate| an entry can hold
IDENTITY_R = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _check_size(what, width, height):
    if not (isinstance(width, (int, np.integer)) and isinstance(height, (int, np.integer))):
        raise ValueError(f"{what}: width and height must be integers")
    if width < 1 or height < 1:
        raise ValueError(f"{what}: width and height must be >= 1")
    if width * height >= 2 ** 31:
        raise ValueError(f"{what}: width * height must be < 2^31")


def _check_k(what, fx, fy, cx, cy):
    if not all(math.isfinite(float(v)) for v in (fx, fy, cx, cy)):
        raise ValueError(f"{what}: fx, fy, cx, cy must be finite")
    if not (fx > 0.0 and fy > 0.0):
        raise ValueError(f"{what}: fx and fy must be > 0")


def check_border(border):
    if not (isinstance(border, (int, np.integer)) and 0 <= border <= 255):
        raise ValueError("border must be an integer in 0..255")
    return int(border)


@dataclass(frozen=True)
class CameraModel:
    """me_camera_model: the raw image size, the pinhole parameters, dist =
    (k1, k2, p1, p2, k3) and R (row-major, 9 values or 3 x 3): raw camera ->
    rectified camera, the R1 / R2 of a stereo calibration, used as given."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    dist: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)
    R: tuple = IDENTITY_R

    def __post_init__(self):
        _check_size("camera model", self.width, self.height)
        _check_k("camera model", self.fx, self.fy, self.cx, self.cy)
        dist = tuple(float(v) for v in np.asarray(self.dist, np.float64).ravel())
        R = tuple(float(v) for v in np.asarray(self.R, np.float64).ravel())
        if len(dist) != 5 or not all(math.isfinite(v) for v in dist):
            raise ValueError("camera model: dist must be 5 finite values (k1, k2, p1, p2, k3)")
        if len(R) != 9 or not all(math.isfinite(v) for v in R):
            raise ValueError("camera model: R must be 9 finite values (row-major 3 x 3)")
        object.__setattr__(self, "dist", dist)
        object.__setattr__(self, "R", R)

    @property
    def shape(self):
        return (int(self.height), int(self.width))

    def to_c(self) -> CameraModelC:
        c = CameraModelC()
        c.width, c.height = int(self.width), int(self.height)
        c.fx, c.fy, c.cx, c.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        c.dist[:] = self.dist
        c.R[:] = self.R
        return c


@dataclass(frozen=True)
class RectifiedModel:
    """me_rectified_model: the size and pinhole parameters both rectified
    images share (the VO loop's width, height and K)."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float

    def __post_init__(self):
        _check_size("rectified model", self.width, self.height)
        _check_k("rectified model", self.fx, self.fy, self.cx, self.cy)

    @staticmethod
    def from_K(width: int, height: int, K) -> "RectifiedModel":
        K = np.asarray(K, np.float64).reshape(3, 3)
        return RectifiedModel(int(width), int(height), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))

    @property
    def shape(self):
        return (int(self.height), int(self.width))

    def matches_K(self, K) -> bool:
        K = np.asarray(K, np.float64).reshape(3, 3)
        return (self.fx, self.fy, self.cx, self.cy) == (K[0, 0], K[1, 1], K[0, 2], K[1, 2])

    def to_c(self) -> RectifiedModelC:
        c = RectifiedModelC()
        c.width, c.height = int(self.width), int(self.height)
        c.fx, c.fy, c.cx, c.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        return c


# ------------------------------------------------------------------ the definition
def rectify_map_ref(cam: CameraModel, rect: RectifiedModel) -> np.ndarray:
    """The Q5 map of me_rectify_map, (height, width, 2) int32: FP64, every
    operation on its own line of the header, rounded once."""
    f8 = np.float64
    u = np.arange(rect.width, dtype=f8)[None, :]
    v = np.arange(rect.height, dtype=f8)[:, None]
    R = [f8(r) for r in cam.R]
    k1, k2, p1, p2, k3 = (f8(d) for d in cam.dist)
    with np.errstate(all="ignore"):
        x = (u - f8(rect.cx)) / f8(rect.fx)
        y = (v - f8(rect.cy)) / f8(rect.fy)
        X = (R[0] * x + R[3] * y) + R[6]
        Y = (R[1] * x + R[4] * y) + R[7]
        W = (R[2] * x + R[5] * y) + R[8]
        a = X / W
        b = Y / W
        a2 = a * a
        b2 = b * b
        r2 = a2 + b2
        tab = f8(2.0) * (a * b)
        rad = f8(1.0) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (a * rad + p1 * tab) + p2 * (r2 + f8(2.0) * a2)
        yd = (b * rad + p1 * (r2 + f8(2.0) * b2)) + p2 * tab
        us = f8(cam.fx) * xd + f8(cam.cx)
        vs = f8(cam.fy) * yd + f8(cam.cy)
        ok = (W > 0.0) & (np.abs(us) < LIMIT) & (np.abs(vs) < LIMIT)  # (all false for NaN)
        iu = np.rint(np.where(ok, us, 0.0) * f8(32.0)).astype(np.int64)  # rint: to nearest-even
        iv = np.rint(np.where(ok, vs, 0.0) * f8(32.0)).astype(np.int64)
    out = np.empty((rect.height, rect.width, 2), np.int32)
    out[..., 0] = np.where(ok, iu, SENTINEL)
    out[..., 1] = np.where(ok, iv, SENTINEL)
    return out


def remap_ref(src, map, border: int = 0) -> np.ndarray:
    """me_remap_q5 restated: `src` (h, w) uint8 (any strides), `map`
    (dst_h, dst_w, 2) int32 -> (dst_h, dst_w) uint8.  int64 arithmetic."""
    border = check_border(border)
    src = np.asarray(src)
    m = np.asarray(map)
    if src.ndim != 2 or src.dtype != np.uint8 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("src must be a (h, w) uint8 image, h and w >= 1")
    if m.ndim != 3 or m.shape[2] != 2 or m.dtype != np.int32 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("map must be (dst_h, dst_w, 2) int32, dst_h and dst_w >= 1")
    h, w = src.shape
    iu, iv = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    sx, fxq = iu >> 5, iu & 31  # (arithmetic shift: floor)
    sy, fyq = iv >> 5, iv & 31

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)  # each tap judged on its own
        px = src[np.where(ok, yy, 0), np.where(ok, xx, 0)].astype(np.int64)
        return np.where(ok, px, border)

    p00, p10, p01, p11 = tap(sx, sy), tap(sx + 1, sy), tap(sx, sy + 1), tap(sx + 1, sy + 1)
    out = (p00 * (32 - fxq) * (32 - fyq) + p10 * fxq * (32 - fyq) + p01 * (32 - fxq) * fyq + p11 * fxq * fyq
           + 512) >> 10
    out = np.where((iu == SENTINEL) & (iv == SENTINEL), border, out)
    return out.astype(np.uint8)


# ------------------------------------------------------------------ the device
def tile_dims():
    """(tile width, tile height, staging capacity in 32-bit words) of
    me_remap_q5 (me_remap_tile_dims).  Needs the library, not a device."""
    tw, th, sw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    load_library().me_remap_tile_dims(ctypes.byref(tw), ctypes.byref(th), ctypes.byref(sw))
    return tw.value, th.value, sw.value


def tile_grid(dst_w: int, dst_h: int):
    """(tiles per row, tile rows) of a destination."""
    tw, th, _ = tile_dims()
    return (dst_w + tw - 1) // tw, (dst_h + th - 1) // th


def rectify_map(cam: CameraModel, rect: RectifiedModel, ctx: Context | None = None, device: bool = False):
    """me_rectify_map: the map as a host array.  device=False runs the
    ME_HOST form (staged by the library), device=True the ME_DEVICE form on a
    buffer of the caller's (allocated, read back and freed here)."""
    ctx = ctx or default_context()
    out = np.empty((rect.height, rect.width, 2), np.int32)
    cc, rc = cam.to_c(), rect.to_c()
    V = ctypes.c_void_p
    if not device:
        ctx.check(ctx.lib.me_rectify_map(ctx.h, ME_HOST, ctypes.byref(cc), ctypes.byref(rc), V(out.ctypes.data)),
                  "me_rectify_map")
        return out
    d = ctx.malloc(out.nbytes)
    try:
        ctx.check(ctx.lib.me_rectify_map(ctx.h, ME_DEVICE, ctypes.byref(cc), ctypes.byref(rc), V(d)), "me_rectify_map")
        ctx.synchronize()
        ctx.d2h(out, d)
    finally:
        ctx.free(d)
    return out


def _rows(a, what):
    """(array, stride) of a (h, w) uint8 image whose rows are contiguous
    (columns 1 byte apart, rows `stride` >= w bytes apart: a padded buffer's
    view keeps its padding); anything else is copied to a dense array."""
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what} must be a (h, w) uint8 image, h and w >= 1")
    h, w = a.shape
    if not (a.strides[1] == 1 and (h == 1 or a.strides[0] >= w)):
        a = np.ascontiguousarray(a)
    return a, (int(a.strides[0]) if h > 1 else w)


def _span(a, stride):
    """The bytes from the first to the last pixel of a strided image, as a flat view."""
    h, w = a.shape
    return np.lib.stride_tricks.as_strided(a, shape=(stride * (h - 1) + w,), strides=(1,))


def remap(src, map, dst_shape=None, border: int = 0, ctx: Context | None = None, tile_path: bool = False,
          out=None, device: bool = False):
    """me_remap_q5.  `src`: (h, w) uint8, a view into a padded buffer keeps
    its row stride; `map`: (dst_h, dst_w, 2) int32; `out`: optional (dst_h,
    dst_w) uint8 view to write (its padding is not touched), else a new array.
    Returns the image, or (image, tile paths (tiles_y, tiles_x) uint8) with
    tile_path.  device=True runs the ME_DEVICE form on uploaded copies."""
    ctx = ctx or default_context()
    border = check_border(border)
    src, s_stride = _rows(src, "src")
    m = np.ascontiguousarray(map, np.int32)
    if m.ndim != 3 or m.shape[2] != 2:
        raise ValueError("map must be (dst_h, dst_w, 2) int32")
    dh, dw = m.shape[:2]
    if dst_shape is not None and tuple(dst_shape) != (dh, dw):
        raise ValueError(f"dst_shape {tuple(dst_shape)} is not the map's {(dh, dw)}")
    if out is None:
        out = np.zeros((dh, dw), np.uint8)
    if out.shape != (dh, dw) or out.dtype != np.uint8 or out.strides[1] != 1 or not out.flags.writeable:
        raise ValueError("out must be a writeable (dst_h, dst_w) uint8 array with contiguous rows")
    d_stride = int(out.strides[0]) if dh > 1 else dw
    if d_stride < dw:
        raise ValueError("out: row stride below the width")
    sh, sw = src.shape
    tx, ty = tile_grid(dw, dh)
    paths = np.full(tx * ty, 255, np.uint8) if tile_path else None
    V = ctypes.c_void_p
    if not device:
        ctx.check(ctx.lib.me_remap_q5(ctx.h, ME_HOST, V(src.ctypes.data), sw, sh, s_stride, V(m.ctypes.data), dw, dh,
                                      border, V(out.ctypes.data), d_stride,
                                      V(paths.ctypes.data) if tile_path else None), "me_remap_q5")
    else:
        s_flat, o_flat = _span(src, s_stride), _span(out, d_stride)
        bufs = [ctx.malloc(s_flat.nbytes), ctx.malloc(m.nbytes), ctx.malloc(o_flat.nbytes), ctx.malloc(tx * ty)]
        try:
            ctx.h2d(bufs[0], s_flat)
            ctx.h2d(bufs[1], m)
            ctx.h2d(bufs[2], o_flat)  # (the padding's bytes travel both ways: the kernel must leave them alone)
            if tile_path:
                ctx.h2d(bufs[3], paths)
            ctx.check(ctx.lib.me_remap_q5(ctx.h, ME_DEVICE, V(bufs[0]), sw, sh, s_stride, V(bufs[1]), dw, dh, border,
                                          V(bufs[2]), d_stride, V(bufs[3]) if tile_path else None), "me_remap_q5")
            ctx.synchronize()
            back = np.empty(o_flat.shape, np.uint8)
            ctx.d2h(back, bufs[2])
            o_flat[:] = back
            if tile_path:
                ctx.d2h(paths, bufs[3])
        finally:
            for b in bufs:
                ctx.free(b)
    return (out, paths.reshape(ty, tx)) if tile_path else out


class StereoRectifier:
    """The two cameras of a rig and the rectified model they share.  Holds
    the two maps: on the host (the numpy restatement, built on first use) and,
    per context, on the device (me_rectify_map).  apply_ref warps a raw pair
    on the host, apply on the device; both give the same bytes."""

    def __init__(self, left: CameraModel, right: CameraModel, out: RectifiedModel, border: int = 0):
        if not (isinstance(left, CameraModel) and isinstance(right, CameraModel) and isinstance(out, RectifiedModel)):
            raise ValueError("StereoRectifier(left: CameraModel, right: CameraModel, out: RectifiedModel)")
        self.left, self.right, self.out = left, right, out
        self.border = check_border(border)
        self._ref = None
        self._dev = {}  # id(ctx) -> (ctx, d_map_left, d_map_right)

    # ---- host
    @property
    def maps_ref(self):
        if self._ref is None:
            self._ref = (rectify_map_ref(self.left, self.out), rectify_map_ref(self.right, self.out))
            for a in self._ref:
                a.setflags(write=False)
        return self._ref

    def check_raw(self, left_shape, right_shape, who: str = "StereoRectifier"):
        """The raw images' shapes against the two camera models."""
        for name, shape, cam in (("left", left_shape, self.left), ("right", right_shape, self.right)):
            if tuple(shape) != cam.shape:
                raise ValueError(f"{who}: the raw {name} image must have its camera model's shape {cam.shape}, "
                                 f"got {tuple(shape)}")

    def apply_ref(self, left, right):
        left, right = np.asarray(left), np.asarray(right)
        self.check_raw(left.shape, right.shape, "StereoRectifier.apply_ref")
        mL, mR = self.maps_ref
        return remap_ref(left, mL, self.border), remap_ref(right, mR, self.border)

    # ---- device
    def device_maps(self, ctx: Context):
        """(left map, right map) device pointers on ctx, built once per context."""
        ent = self._dev.get(id(ctx))
        if ent is None:
            cr = self.out.to_c()
            ptrs = []
            try:
                for cam in (self.left, self.right):
                    cc = cam.to_c()
                    d = ctx.malloc(8 * self.out.width * self.out.height)
                    ptrs.append(d)
                    ctx.check(ctx.lib.me_rectify_map(ctx.h, ME_DEVICE, ctypes.byref(cc), ctypes.byref(cr),
                                                     ctypes.c_void_p(d)), "me_rectify_map")
            except Exception:
                for d in ptrs:
                    ctx.free(d)
                raise
            ent = self._dev[id(ctx)] = (ctx, ptrs[0], ptrs[1])
        return ent[1], ent[2]

    def apply_device(self, ctx: Context, d_left: int, d_right: int, d_out_left: int, d_out_right: int):
        """Two me_remap_q5 queued on ctx's stream: raw device images (dense
        rows, the models' sizes) -> rectified device images (dense rows)."""
        mL, mR = self.device_maps(ctx)
        V = ctypes.c_void_p
        W, H = self.out.width, self.out.height
        for cam, d_in, d_map, d_out in ((self.left, d_left, mL, d_out_left), (self.right, d_right, mR, d_out_right)):
            ctx.check(ctx.lib.me_remap_q5(ctx.h, ME_DEVICE, V(d_in), cam.width, cam.height, cam.width, V(d_map), W, H,
                                          self.border, V(d_out), W, None), "me_remap_q5")

    def apply(self, ctx: Context | None, left, right):
        """apply_ref on the device: host arrays in, host arrays out."""
        ctx = ctx or default_context()
        L, R = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        self.check_raw(L.shape, R.shape, "StereoRectifier.apply")
        n = self.out.width * self.out.height
        bufs = [ctx.malloc(L.nbytes), ctx.malloc(R.nbytes), ctx.malloc(2 * n)]
        try:
            ctx.h2d(bufs[0], L)
            ctx.h2d(bufs[1], R)
            self.apply_device(ctx, bufs[0], bufs[1], bufs[2], bufs[2] + n)
            ctx.synchronize()
            out = np.empty((2,) + self.out.shape, np.uint8)
            ctx.d2h(out, bufs[2])
        finally:
            for b in bufs:
                ctx.free(b)
        return out[0], out[1]

    def release(self, ctx: Context | None = None):
        """Frees the device maps (of one context, or of all)."""
        for key in [k for k, e in self._dev.items() if ctx is None or e[0] is ctx]:
            c, a, b = self._dev.pop(key)
            if getattr(c, "h", None):
                c.free(a)
                c.free(b)
