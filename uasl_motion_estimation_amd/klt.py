"""Pyramidal Lucas-Kanade tracking on MI355X (klt.hip).

Build-defined (the reference has no tracker): OpenCV-style
calcOpticalFlowPyrLK defaults (21x21 window, 3 pyramid levels, 30 iterations,
eps 0.01, min-eigenvalue 1e-4) with an integer/fixed-point formulation that
makes the device result bit-identical to its CPU restatement (oracle/klt.cpp).

With fb_max set the call is the forward-backward check (me_klt_track_fb,
include/me_hip.h A12c): prev -> next, back next -> prev from the result, and a
feature keeps status 1 only if both passes tracked it and it returns within
fb_max pixels of where it started.

With guess (n, 2) the search starts at each feature's guess instead of at its
old position (me_klt_track_guided / me_klt_track_guided_fb, include/me_hip.h
A12f); a guess that is not finite or lies outside the image is ignored.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import ME_HOST, Context, KLTParamsC, default_context, vptr


def klt_params(win=21, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4) -> KLTParamsC:
    k = KLTParamsC()
    k.win, k.max_level, k.max_iters, k.eps, k.min_eig = win, max_level, max_iters, eps, min_eig
    return k


def calcOpticalFlowPyrLK(prev, nxt, pts, ctx: Context | None = None, fb_max: float | None = None, guess=None, **kw):
    """Track pts (n, 2) float32 from prev to nxt.  Returns (pts_out (n,2), status (n,) uint8); with fb_max
    (pixels, > 0) the status is the forward-backward check's and the return value is (pts_out, status,
    fb_err (n,) float32: the round-trip distance, inf where a pass failed).  guess (n, 2) float32: where each
    feature's search starts in nxt (level-0 pixels); None: at the feature's position in prev."""
    ctx = ctx or default_context()
    prev = np.ascontiguousarray(prev, np.uint8)
    nxt = np.ascontiguousarray(nxt, np.uint8)
    if prev.shape != nxt.shape or prev.ndim != 2:
        raise ValueError("prev/next must be equal-size grayscale images")
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    h, w = prev.shape
    out = np.zeros_like(pts)
    st = np.zeros(len(pts), np.uint8)
    kp = klt_params(**kw)
    if guess is not None:
        guess = np.ascontiguousarray(guess, np.float32).reshape(-1, 2)
        if guess.shape != pts.shape:
            raise ValueError("guess must hold one (x, y) per feature")
        if fb_max is not None:
            err = np.zeros(len(pts), np.float32)
            ctx.check(ctx.lib.me_klt_track_guided_fb(ctx.h, ME_HOST, vptr(prev), vptr(nxt), w, h, w, vptr(pts),
                                                     vptr(guess), vptr(out), vptr(st), vptr(err), len(pts),
                                                     ctypes.byref(kp), float(fb_max)), "me_klt_track_guided_fb")
            return out, st, err
        ctx.check(ctx.lib.me_klt_track_guided(ctx.h, ME_HOST, vptr(prev), vptr(nxt), w, h, w, vptr(pts), vptr(guess),
                                              vptr(out), vptr(st), len(pts), ctypes.byref(kp)), "me_klt_track_guided")
        return out, st
    if fb_max is not None:
        err = np.zeros(len(pts), np.float32)
        ctx.check(ctx.lib.me_klt_track_fb(ctx.h, ME_HOST, vptr(prev), vptr(nxt), w, h, w, vptr(pts), vptr(out),
                                          vptr(st), vptr(err), len(pts), ctypes.byref(kp), float(fb_max)),
                  "me_klt_track_fb")
        return out, st, err
    ctx.check(ctx.lib.me_klt_track(ctx.h, ME_HOST, vptr(prev), vptr(nxt), w, h, w, vptr(pts), vptr(out), vptr(st),
                                   len(pts), ctypes.byref(kp)), "me_klt_track")
    return out, st
