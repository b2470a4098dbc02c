"""Numpy restatement of the pyramidal Lucas-Kanade tracker and of its guided
forms (include/me_hip.h A12, A12f): the checker of me_klt_track_guided and
me_klt_track_guided_fb, and the tracker of the host backends when the VO loop
runs with PipelineConfig.klt_predict.

float32 and int64 arithmetic in the order of oracle/klt.cpp, vectorised over
the features: every feature runs the serial tracker's operations on its own
values, so without a guess the result is oracle/klt.cpp's bit for bit
(tests/test_klt_guided.py anchors it there).  With a guess only the start of
the top pyramid level's search moves.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
_K5 = np.array([1, 4, 6, 4, 1], np.int64)


def _refl(i, n):
    """reflect-101 of the index array i into 0 .. n - 1 (repeated for indices further out)."""
    if n == 1:
        return np.zeros_like(i)
    i = i.copy()
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    """5 x 5 binomial [1 4 6 4 1]^2 / 256, reflect-101, (s + 128) >> 8; (h, w) -> ((h + 1) // 2, (w + 1) // 2)."""
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    a = img.astype(np.int64)
    rows = np.zeros((h, dw), np.int64)
    xs = 2 * np.arange(dw)
    for b in range(5):
        rows += _K5[b] * a[:, _refl(xs + b - 2, w)]
    s = np.zeros((dh, dw), np.int64)
    ys = 2 * np.arange(dh)
    for k in range(5):
        s += _K5[k] * rows[_refl(ys + k - 2, h)]
    return ((s + 128) >> 8).astype(np.uint8)


def scharr(img):
    """Scharr derivatives (3 / 10 / 3 smoothing, reflect-101) of an 8-bit image, int16 each."""
    h, w = img.shape
    a = img.astype(np.int64)
    r0, r2 = a[_refl(np.arange(h) - 1, h)], a[_refl(np.arange(h) + 1, h)]
    xm, xp = _refl(np.arange(w) - 1, w), _refl(np.arange(w) + 1, w)
    t0 = 3 * (r0 + r2) + 10 * a
    t1 = r2 - r0
    dx = t0[:, xp] - t0[:, xm]
    dy = 3 * (t1[:, xp] + t1[:, xm]) + 10 * t1
    return dx.astype(np.int16), dy.astype(np.int16)


def pyramid(img, max_level):
    levels = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(max_level):
        levels.append(pyr_down(levels[-1]))
    return levels


def usable(guess, w, h):
    """(n,) bool: both components finite, 0 <= gx < w and 0 <= gy < h, compared as floats."""
    g = np.asarray(guess, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return (g[:, 0] >= F32(0)) & (g[:, 0] < F32(w)) & (g[:, 1] >= F32(0)) & (g[:, 1] < F32(h))


def start_points(pts, guess, w, h):
    """s_i = usable ? guess_i : pts_i, float32 (n, 2)."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    if guess is None:
        return pts
    g = np.ascontiguousarray(guess, F32).reshape(-1, 2)
    if g.shape != pts.shape:
        raise ValueError("guess must hold one (x, y) per feature")
    return np.where(usable(g, w, h)[:, None], g, pts)


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _weights(a, b):
    """Bilinear weights of the fractions (a, b), float32 products rounded to integers, 2^14 in all."""
    one, s = F32(1), F32(16384)
    w00 = np.rint((one - a) * (one - b) * s).astype(np.int64)
    w01 = np.rint(a * (one - b) * s).astype(np.int64)
    w10 = np.rint((one - a) * b * s).astype(np.int64)
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _floor_int(v):
    with np.errstate(invalid="ignore"):
        f = np.floor(v.astype(np.float64))
        f = np.where(np.isfinite(f), np.clip(f, -2.0**31, 2.0**31 - 1), -2.0**31)  # ((int) of NaN / out of range)
    return f.astype(np.int64)


def _bilinear(flat, w, x0, y0, wts, oy, ox):
    """Weighted tap sums (int64) of the win x win windows with origins (x0, y0): (k, win * win)."""
    o = (y0[:, None] + oy[None, :]) * w + x0[:, None] + ox[None, :]
    w00, w01, w10, w11 = (t[:, None] for t in wts)
    return flat[o] * w00 + flat[o + 1] * w01 + flat[o + w] * w10 + flat[o + w + 1] * w11


TRACE_COUNTS = ("reject_l0", "reject_upper", "left_image", "iters", "iters_w11_neg", "templates_w11_neg",
                "oscillation", "exhausted")
TRACE_MAXIMA = ("max_a11", "max_abs_a12", "max_a22", "max_abs_b1", "max_abs_b2")


def _trace_add(trace, key, v):
    trace[key] = trace.get(key, 0) + int(v)


def _trace_max(trace, key, a):
    trace[key] = max(trace.get(key, 0), int(np.abs(a).max()) if len(a) else 0)


def klt_track_ref(prev, next, pts, guess=None, win=21, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4,
                  trace: dict | None = None):
    """me_klt_track (guess None) / me_klt_track_guided: (pts_out (n, 2) float32, status (n,) uint8).

    trace: a dict that accumulates, over the calls it is passed to, which paths the features took (the tests
    prove from it that an input reaches the path it is named for).  Per (feature, level): "outside" {level:
    templates skipped because their window was outside}, "reject_l0" / "reject_upper" (minimum eigenvalue or
    determinant, level 0 / levels above), "left_image" (search window left the level), "oscillation" (the
    half-step exit), "exhausted" (ran all max_iters iterations), "templates_w11_neg" (fourth template weight
    -1).  "iters" / "iters_w11_neg": iterations run / with the fourth weight -1.  "max_a11", "max_abs_a12",
    "max_a22", "max_abs_b1", "max_abs_b2": the largest window sums seen, integers before FLT_SCALE."""
    prev = np.ascontiguousarray(prev, np.uint8)
    nxt = np.ascontiguousarray(next, np.uint8)
    if prev.shape != nxt.shape or prev.ndim != 2:
        raise ValueError("prev/next must be equal-size grayscale images")
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    n = len(pts)
    H0, W0 = prev.shape
    start = start_points(pts, guess, W0, H0)
    st = np.ones(n, np.uint8)
    nx, ny = np.zeros(n, F32), np.zeros(n, F32)
    if trace is not None:
        trace.setdefault("outside", {})
        for key in TRACE_COUNTS + TRACE_MAXIMA:
            trace.setdefault(key, 0)
    if n == 0:
        return np.zeros((0, 2), F32), st
    P, N = pyramid(prev, max_level), pyramid(nxt, max_level)
    half = (win - 1) // 2
    hf = F32(half)
    FLT_SCALE = 1.0 / (1 << 20)
    eps2 = float(eps) * float(eps)
    oy, ox = (a.ravel() for a in np.meshgrid(np.arange(win), np.arange(win), indexing="ij"))
    for L in range(max_level, -1, -1):
        I = P[L]
        H, W = I.shape
        dxL, dyL = scharr(I)
        If, Dxf, Dyf = I.astype(np.int64).ravel(), dxL.astype(np.int64).ravel(), dyL.astype(np.int64).ravel()
        Jf = N[L].astype(np.int64).ravel()
        sc = F32(1.0) / F32(1 << L)
        px, py = pts[:, 0] * sc, pts[:, 1] * sc
        if L == max_level:
            nx, ny = start[:, 0] * sc, start[:, 1] * sc
        else:
            nx, ny = nx * F32(2), ny * F32(2)
        pxw, pyw = px - hf, py - hf
        ix0, iy0 = _floor_int(pxw), _floor_int(pyw)
        inside = (ix0 >= 0) & (iy0 >= 0) & (ix0 + win < W) & (iy0 + win < H)
        if L == 0:
            st[~inside] = 0
        k = np.flatnonzero(inside)
        if trace is not None:
            trace["outside"][L] = trace["outside"].get(L, 0) + int(n - len(k))
        if len(k) == 0:
            continue
        x0, y0 = ix0[k], iy0[k]
        wts = _weights(pxw[k] - x0.astype(F32), pyw[k] - y0.astype(F32))
        if trace is not None:
            _trace_add(trace, "templates_w11_neg", (wts[3] < 0).sum())
        iv = _descale(_bilinear(If, W, x0, y0, wts, oy, ox), 9)
        gx = _descale(_bilinear(Dxf, W, x0, y0, wts, oy, ox), 14)
        gy = _descale(_bilinear(Dyf, W, x0, y0, wts, oy, ox), 14)
        A11, A12, A22 = (gx * gx).sum(1), (gx * gy).sum(1), (gy * gy).sum(1)
        if trace is not None:
            _trace_max(trace, "max_a11", A11)
            _trace_max(trace, "max_abs_a12", A12)
            _trace_max(trace, "max_a22", A22)
        a11 = A11.astype(np.float64) * FLT_SCALE
        a12 = A12.astype(np.float64) * FLT_SCALE
        a22 = A22.astype(np.float64) * FLT_SCALE
        D = a11 * a22 - a12 * a12
        min_e = (a22 + a11 - np.sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / (2.0 * win * win)
        good = ~((min_e < min_eig) | (D < 1.1920928955078125e-07))
        if L == 0:
            st[k[~good]] = 0
        if trace is not None:
            _trace_add(trace, "reject_l0" if L == 0 else "reject_upper", (~good).sum())
        k, iv, gx, gy = k[good], iv[good], gx[good], gy[good]
        a11, a12, a22, D = a11[good], a12[good], a22[good], D[good]
        if len(k) == 0:
            continue
        with np.errstate(divide="ignore"):
            Dinv = 1.0 / D
        nxw, nyw = nx[k] - hf, ny[k] - hf
        pdx, pdy = np.zeros(len(k), F32), np.zeros(len(k), F32)
        run = np.ones(len(k), bool)  # features still iterating at this level
        for j in range(max_iters):
            r = np.flatnonzero(run)
            if len(r) == 0:
                break
            jx0, jy0 = _floor_int(nxw[r]), _floor_int(nyw[r])
            ins = (jx0 >= 0) & (jy0 >= 0) & (jx0 + win < W) & (jy0 + win < H)
            if L == 0:
                st[k[r[~ins]]] = 0
            run[r[~ins]] = False
            if trace is not None:
                _trace_add(trace, "left_image", (~ins).sum())
            r, jx0, jy0 = r[ins], jx0[ins], jy0[ins]
            if len(r) == 0:
                break
            wj = _weights(nxw[r] - jx0.astype(F32), nyw[r] - jy0.astype(F32))
            diff = _descale(_bilinear(Jf, W, jx0, jy0, wj, oy, ox), 9) - iv[r]
            B1, B2 = (diff * gx[r]).sum(1), (diff * gy[r]).sum(1)
            if trace is not None:
                _trace_add(trace, "iters", len(r))
                _trace_add(trace, "iters_w11_neg", (wj[3] < 0).sum())
                _trace_max(trace, "max_abs_b1", B1)
                _trace_max(trace, "max_abs_b2", B2)
            b1d = B1.astype(np.float64) * FLT_SCALE
            b2d = B2.astype(np.float64) * FLT_SCALE
            with np.errstate(invalid="ignore", over="ignore"):
                ddx = ((a12[r] * b2d - a22[r] * b1d) * Dinv[r]).astype(F32)
                ddy = ((a12[r] * b1d - a11[r] * b2d) * Dinv[r]).astype(F32)
                nxw[r] = nxw[r] + ddx
                nyw[r] = nyw[r] + ddy
                nx[k[r]] = nxw[r] + hf
                ny[k[r]] = nyw[r] + hf
                small = ddx.astype(np.float64) * ddx.astype(np.float64) + ddy.astype(np.float64) * ddy.astype(
                    np.float64) <= eps2
                back = np.zeros(len(r), bool)
                if j > 0:
                    back = ~small & (np.abs(ddx + pdx[r]) < F32(0.01)) & (np.abs(ddy + pdy[r]) < F32(0.01))
                    kb = k[r[back]]
                    nx[kb] = nx[kb] - ddx[back] * F32(0.5)
                    ny[kb] = ny[kb] - ddy[back] * F32(0.5)
            run[r[small | back]] = False
            pdx[r], pdy[r] = ddx, ddy
            if trace is not None:
                _trace_add(trace, "oscillation", back.sum())
        if trace is not None:
            _trace_add(trace, "exhausted", run.sum())
    return np.stack([nx, ny], -1).astype(F32), st


def klt_guided_fb_ref(prev, next, pts, guess, fb_max, **kw):
    """me_klt_track_guided_fb (include/me_hip.h A12f): (pts_out of the forward
    pass, combined status, fb_err float32: the round-trip distance, inf where
    a pass failed).  guess None: me_klt_track_fb."""
    if not fb_max > 0.0:  # (false for NaN)
        raise ValueError("fb_max must be > 0")
    prev = np.ascontiguousarray(prev, np.uint8)
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    h, w = prev.shape
    q, sf = klt_track_ref(prev, next, pts, guess, **kw)
    with np.errstate(invalid="ignore", over="ignore"):
        e = start_points(pts, guess, w, h) - pts  # float32, then b = q - e: two roundings
        b = q - e
    r, sb = klt_track_ref(next, prev, q, b, **kw)
    both = (sf == 1) & (sb == 1)  # (the pass of a feature with sf = 0 is skipped: it counts as lost)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = r[:, 0].astype(np.float64) - pts[:, 0].astype(np.float64)
        dy = r[:, 1].astype(np.float64) - pts[:, 1].astype(np.float64)
        d2 = dx * dx + dy * dy
        status = (both & (d2 <= np.float64(fb_max) * np.float64(fb_max))).astype(np.uint8)
        fb_err = np.where(both, np.sqrt(d2), np.inf).astype(F32)
    return q, status, fb_err
