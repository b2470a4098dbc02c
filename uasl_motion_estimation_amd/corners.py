"""Corner detector of the VO loop (csrc/corners.hip).

Build-defined, like the KLT and the epipolar matcher (the reference has no
detector: the application that drove it is absent).  A new track starts where
the KLT's own acceptance test is strongest: the response of a pixel is the
minimum eigenvalue of the structure tensor of the win x win window centred on
it, in the KLT's integer formulation, so at an integer position it equals the
minEig that klt.hip / oracle/klt.cpp compute there, bit for bit.

This module states the definition once, in numpy (`corner_response_ref`,
`corner_mask_ref`, `select_corners_ref`, `new_corners_ref`): the host backends
of the loop and the tests use it; the device calls (`corner_response`,
`new_corners`) must reproduce it exactly.

Response R(x, y), FP64, of an 8-bit image w x h, odd window win (3..31),
half = (win - 1) / 2:
  dx, dy  level-0 Scharr derivatives (3/10/3, reflect-101), int16;
  A11 = sum dx^2, A12 = sum dx dy, A22 = sum dy^2 over the window, exact
  integers (they need more than 32 bits);
  a = A * 2^-20;  R = (a22 + a11 - sqrt((a11 - a22) (a11 - a22) + 4 a12 a12)) / (2 win win)
  where the KLT accepts the window at level 0 (x - half >= 0, y - half >= 0,
  x - half + win < w, y - half + win < h); R = 0 elsewhere.
Corner: R(p) >= min_eig (> 0) and p beats its 8 neighbours inside the image
in the total order "larger R first, then smaller row-major index".
New features of a keyframe: the grid and the good tracked features of
pipeline.new_cells; every cell keeps its best corner inside the margin; the
first max(0, n_feats - #good) unoccupied cells that hold one, in ascending
order, emit (float32 x, float32 y).  No jitter, no dependence on t.

Out of scope: minimum-distance suppression across cell borders, sub-pixel
refinement, detection on pyramid levels above 0.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import ME_HOST, Context, CornerParamsC, default_context, vptr

WIN_MIN, WIN_MAX = 3, 31
MAX_CELLS = 65536


def corner_params(win: int = 21, min_eig: float = 1e-4) -> CornerParamsC:
    p = CornerParamsC()
    p.win, p.min_eig = int(win), float(min_eig)
    return p


def _check_params(win, min_eig=1e-4):
    if not (WIN_MIN <= win <= WIN_MAX and win % 2 == 1):
        raise ValueError(f"corner window must be odd and in [{WIN_MIN}, {WIN_MAX}]")
    if not min_eig > 0:
        raise ValueError("min_eig must be > 0")


# ------------------------------------------------------------------ the definition (numpy)
def scharr_ref(img: np.ndarray):
    """Level-0 Scharr derivatives of the KLT (oracle_scharr): int16 dx, dy."""
    I = np.ascontiguousarray(img, np.uint8).astype(np.int32)
    h, w = I.shape
    # one pixel of reflect-101 border (an axis of one pixel reflects onto itself: refl(i, 1) = 0)
    ry = np.array([min(1, h - 1)] + list(range(h)) + [max(h - 2, 0)])
    rx = np.array([min(1, w - 1)] + list(range(w)) + [max(w - 2, 0)])
    P = I[ry][:, rx]
    r0, r1, r2 = P[:-2], P[1:-1], P[2:]
    t0 = 3 * (r0 + r2) + 10 * r1          # vertical smoothing, every padded column
    t1 = r2 - r0                          # vertical difference
    dx = t0[:, 2:] - t0[:, :-2]
    dy = 3 * (t1[:, 2:] + t1[:, :-2]) + 10 * t1[:, 1:-1]
    return dx.astype(np.int16), dy.astype(np.int16)


def _box_valid(P: np.ndarray, win: int) -> np.ndarray:
    """Sums of P (int64) over every win x win window that lies inside the
    array: (h - win + 1, w - win + 1)."""
    h, w = P.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = P.cumsum(0).cumsum(1)
    return S[win:, win:] - S[:-win, win:] - S[win:, :-win] + S[:-win, :-win]


def structure_tensor_ref(img: np.ndarray, win: int = 21):
    """(A11, A12, A22, valid): the window sums as int64 (0 where invalid) and
    the validity mask of the definition."""
    _check_params(win)
    dx, dy = scharr_ref(img)
    h, w = dx.shape
    half = (win - 1) // 2
    valid = np.zeros((h, w), bool)
    out = [np.zeros((h, w), np.int64) for _ in range(3)]
    # x - half >= 0 and x - half + win < w  <=>  half <= x <= w - half - 2
    x1, y1 = w - half - 2, h - half - 2
    if x1 >= half and y1 >= half:
        valid[half:y1 + 1, half:x1 + 1] = True
        dx64, dy64 = dx.astype(np.int64), dy.astype(np.int64)
        for o, P in zip(out, (dx64 * dx64, dx64 * dy64, dy64 * dy64)):
            B = _box_valid(P, win)  # B[y - half, x - half] = the window centred on (x, y)
            o[half:y1 + 1, half:x1 + 1] = B[:y1 + 1 - half, :x1 + 1 - half]
    return out[0], out[1], out[2], valid


def corner_response_ref(img: np.ndarray, win: int = 21) -> np.ndarray:
    """The response map of the definition, (h, w) float64."""
    A11, A12, A22, valid = structure_tensor_ref(img, win)
    scale = 1.0 / (1 << 20)
    a11, a12, a22 = A11.astype(np.float64) * scale, A12.astype(np.float64) * scale, A22.astype(np.float64) * scale
    R = (a22 + a11 - np.sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / (2.0 * win * win)
    return np.where(valid, R, 0.0)


def corner_mask_ref(R: np.ndarray, min_eig: float = 1e-4) -> np.ndarray:
    """Corners of a response map: R >= min_eig and the key (larger R, then
    smaller row-major index) beats the keys of the 8 neighbours inside it."""
    _check_params(3, min_eig)
    R = np.ascontiguousarray(R, np.float64)
    h, w = R.shape
    P = np.full((h + 2, w + 2), -np.inf)
    P[1:-1, 1:-1] = R
    m = R >= min_eig
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            N = P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            m &= (R > N) if (dy, dx) < (0, 0) else (R >= N)  # an earlier neighbour wins a tie
    return m


def _cells_of(u, v, margin, nx, ny, cw, ch):
    m = np.float64(np.float32(margin))
    cx = np.clip(((u.astype(np.float64) - m) / cw).astype(np.int64), 0, nx - 1)
    cy = np.clip(((v.astype(np.float64) - m) / ch).astype(np.int64), 0, ny - 1)
    return cy * nx + cx


def _in_margin(u, v, width, height, margin):
    m = np.float32(margin)
    return (u >= m) & (u < np.float32(width) - m) & (v >= m) & (v < np.float32(height) - m)


def select_corners_ref(R: np.ndarray, uv, status, ok, margin, nx, ny, cw, ch, n_feats, d_min=0, min_eig=1e-4):
    """New features from a response map: (uv (k, 2) float32, lo (k,) int32).
    uv / status / ok are the tracked features (None: none)."""
    if nx <= 0 or ny <= 0 or nx * ny > MAX_CELLS:
        raise ValueError(f"bad grid (at most {MAX_CELLS} cells)")
    R = np.ascontiguousarray(R, np.float64)
    h, w = R.shape
    ncell = nx * ny
    occ = np.zeros(ncell, bool)
    n_good = 0
    if uv is not None and len(uv):
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        good = ((np.asarray(status) == 1) & (np.asarray(ok) != 0)
                & _in_margin(uv[:, 0], uv[:, 1], w, h, margin))
        n_good = int(good.sum())
        occ[_cells_of(uv[good, 0], uv[good, 1], margin, nx, ny, cw, ch)] = True
    ys, xs = np.nonzero(corner_mask_ref(R, min_eig))
    xf, yf = xs.astype(np.float32), ys.astype(np.float32)
    el = _in_margin(xf, yf, w, h, margin)
    xs, ys, xf, yf = xs[el], ys[el], xf[el], yf[el]
    cell = _cells_of(xf, yf, margin, nx, ny, cw, ch)
    idx = ys.astype(np.int64) * w + xs
    order = np.lexsort((idx, -R[ys, xs], cell))  # per cell: larger R first, then smaller index
    cs = cell[order]
    first = np.ones(len(cs), bool)
    first[1:] = cs[1:] != cs[:-1]
    best = order[first]                          # ascending cell order
    best = best[~occ[cell[best]]][: max(0, n_feats - n_good)]
    out = np.stack([xf[best], yf[best]], -1).astype(np.float32).reshape(-1, 2)
    return out, np.full(len(out), d_min, np.int32)


def new_corners_ref(img, uv, status, ok, margin, nx, ny, cw, ch, n_feats, d_min=0, win=21, min_eig=1e-4):
    """me_vo_new_corners restated: the new features of a keyframe."""
    _check_params(win, min_eig)
    return select_corners_ref(corner_response_ref(img, win), uv, status, ok, margin, nx, ny, cw, ch, n_feats, d_min,
                              min_eig)


# ------------------------------------------------------------------ the device
def corner_response(img, win: int = 21, ctx: Context | None = None) -> np.ndarray:
    """The response map computed on the device (me_corner_response)."""
    ctx = ctx or default_context()
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 2:
        raise ValueError("img must be a grayscale image")
    h, w = img.shape
    out = np.zeros((h, w), np.float64)
    p = corner_params(win)
    ctx.check(ctx.lib.me_corner_response(ctx.h, ME_HOST, vptr(img), w, h, w, ctypes.byref(p), vptr(out)),
              "me_corner_response")
    return out


def new_corners(img, uv, status, ok, margin, nx, ny, cw, ch, n_feats, d_min=0, win=21, min_eig=1e-4,
                ctx: Context | None = None):
    """me_vo_new_corners on host arrays (uploaded, run, read back):
    (uv (k, 2) float32, lo (k,) int32).  uv / status / ok may be None."""
    ctx = ctx or default_context()
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    n = 0 if uv is None else len(uv)
    m = max(int(n_feats), 1)
    V = ctypes.c_void_p
    d_img = ctx.malloc(img.nbytes)
    d_in = ctx.malloc(10 * max(n, 1))
    d_out = ctx.malloc(16 + 12 * m)
    try:
        ctx.h2d(d_img, img)
        if n:
            ctx.h2d(d_in, np.ascontiguousarray(uv, np.float32).reshape(n, 2))
            ctx.h2d(d_in + 8 * n, np.ascontiguousarray(status, np.uint8))
            ctx.h2d(d_in + 9 * n, np.ascontiguousarray(np.asarray(ok) != 0, np.uint8))
        p = corner_params(win, min_eig)
        ctx.check(ctx.lib.me_vo_new_corners(ctx.h, V(d_img), w, h, w, V(d_in) if n else None,
                                            V(d_in + 8 * n) if n else None, V(d_in + 9 * n) if n else None, n,
                                            float(margin), nx, ny, float(cw), float(ch), int(n_feats), int(d_min),
                                            ctypes.byref(p), V(d_out + 16), V(d_out + 16 + 8 * m), V(d_out)),
                  "me_vo_new_corners")
        buf = np.zeros(16 + 12 * m, np.uint8)
        ctx.d2h(buf, d_out)
    finally:
        ctx.free(d_img)
        ctx.free(d_in)
        ctx.free(d_out)
    k = int(buf[:4].view(np.int32)[0])
    return (buf[16:16 + 8 * k].view(np.float32).reshape(k, 2).copy(),
            buf[16 + 8 * m:16 + 8 * m + 4 * k].view(np.int32).copy())
