"""Keyframe selection between the VO loop's keyframes (include/me_hip.h,
section A12i): the features of the last keyframe are followed through the
frames in between, and a frame becomes the next keyframe once too few of them
survive, their median displacement from the keyframe is large enough, or the
gap is too long.

The definition is build-defined, exact integers and FP64.  kf_update_ref
restates the header in numpy with a plain stable sort: it is the checker of the
device kernel (csrc/keyframe.hip, a radix select) and what the host backends
run.  kf_update is the binding of me_kf_update; KeyframeSelect holds the
parameters and is what PipelineConfig.keyframe_select takes.  cur_uv, alive and
every byte of the info block are bit-exact."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import Context, KfParamsC, default_context

INFO_BYTES = 32  # int32 n, m, rank, flags; double med2; 8 zero bytes
FEW, PARALLAX, GAP = 1, 2, 4  # the flag bits


@dataclass(frozen=True)
class KeyframeSelect:
    """me_kf_params.  The defaults are a starting point for a 30 - 60 Hz rig,
    not measurements of real data."""
    min_parallax: float = 12.0   # pixels: median displacement from the last keyframe that declares one (>= 0; 0: rule off)
    min_tracked_pct: int = 60    # a keyframe once fewer than this share of the seeded features is alive (0 .. 100)
    max_gap: int = 10            # a keyframe at the latest this many frames after the last one (>= 1)

    def __post_init__(self):
        def integer(name, lo, hi):
            v = getattr(self, name)
            if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi):
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}")

        try:
            v = float(self.min_parallax)
        except (TypeError, ValueError):
            raise ValueError("min_parallax must be a finite number >= 0") from None
        if isinstance(self.min_parallax, bool) or not (math.isfinite(v) and v >= 0.0):
            raise ValueError("min_parallax must be a finite number >= 0")
        integer("min_tracked_pct", 0, 100)
        integer("max_gap", 1, 2 ** 31 - 1)

    def to_c(self) -> KfParamsC:
        c = KfParamsC()
        c.min_parallax, c.min_tracked_pct, c.max_gap = float(self.min_parallax), int(self.min_tracked_pct), int(self.max_gap)
        return c


# ------------------------------------------------------------------ the definition
def kf_update_ref(ref_uv, cur_uv, alive, new_uv, status, width, height, margin, gap, params: KeyframeSelect | None = None):
    """me_kf_update restated.  ref_uv, cur_uv, new_uv (n, 2) float32, alive and
    status (n,) bytes.  Returns (cur_uv (n, 2) float32, alive (n,) uint8, info):
    info is a dict with n, m, rank, flags, med2 and keyframe."""
    p = params or KeyframeSelect()
    ref_uv = np.asarray(ref_uv, np.float32).reshape(-1, 2)
    cur_uv = np.asarray(cur_uv, np.float32).reshape(-1, 2)
    new_uv = np.asarray(new_uv, np.float32).reshape(-1, 2)
    alive = np.asarray(alive).astype(np.uint8).reshape(-1)
    status = np.asarray(status).astype(np.uint8).reshape(-1)
    n = len(ref_uv)
    if not (len(cur_uv) == len(new_uv) == len(alive) == len(status) == n):
        raise ValueError("kf_update_ref: the per-feature arrays differ in length")
    if int(gap) < 1:
        raise ValueError("kf_update_ref: gap must be >= 1")
    mg = np.float32(margin)
    u, v = new_uv[:, 0], new_uv[:, 1]
    with np.errstate(all="ignore"):
        a = ((alive != 0) & (status == 1) & np.isfinite(u) & np.isfinite(v) & (u >= mg) & (u < np.float32(width) - mg)
             & (v >= mg) & (v < np.float32(height) - mg))
    cur = np.where(a[:, None], new_uv, cur_uv)  # (a bitwise select: the kept positions keep their bits)
    dx = cur[a, 0].astype(np.float64) - ref_uv[a, 0].astype(np.float64)
    dy = cur[a, 1].astype(np.float64) - ref_uv[a, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        d2 = (dx * dx) + (dy * dy)
    m = int(a.sum())
    rank = (m - 1) >> 1
    med2 = float(np.sort(d2, kind="stable")[rank]) if m else 0.0
    thr2 = float(p.min_parallax) * float(p.min_parallax)
    flags = 0
    if n == 0 or 100 * m < int(p.min_tracked_pct) * n:
        flags |= FEW
    if thr2 > 0.0 and med2 >= thr2:  # (min_parallax = 0: the rule is off)
        flags |= PARALLAX
    if int(gap) >= int(p.max_gap):
        flags |= GAP
    info = dict(n=n, m=m, rank=rank, flags=flags, med2=med2, keyframe=flags != 0)
    return cur, a.astype(np.uint8), info


def info_bytes(info) -> np.ndarray:
    """The device info block of a restated result, as its 32 bytes."""
    out = np.zeros(INFO_BYTES, np.uint8)
    out[:16] = np.array([info["n"], info["m"], info["rank"], info["flags"]], np.int32).view(np.uint8)
    out[16:24] = np.array([info["med2"]], np.float64).view(np.uint8)
    return out


def parse_info(raw) -> dict:
    """The info block me_kf_update wrote (32 bytes) as kf_update_ref's dict."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(INFO_BYTES)
    i = raw[:16].view(np.int32)
    return dict(n=int(i[0]), m=int(i[1]), rank=int(i[2]), flags=int(i[3]), med2=float(raw[16:24].view(np.float64)[0]),
                keyframe=int(i[3]) != 0)


# ------------------------------------------------------------------ the device call
def kf_update_device(ctx: Context, params: KeyframeSelect, d_ref_uv: int, d_cur_uv: int, d_alive: int, d_new_uv: int,
                     d_status: int, n: int, width, height, margin, gap, d_info: int):
    """One me_kf_update queued on ctx's stream, everything in device memory."""
    pc = params.to_c()
    V = ctypes.c_void_p

    def ptr(d):
        return V(d) if d else None

    ctx.check(ctx.lib.me_kf_update(ctx.h, ptr(d_ref_uv), ptr(d_cur_uv), ptr(d_alive), ptr(d_new_uv), ptr(d_status),
                                   int(n), int(width), int(height), float(margin), int(gap), ctypes.byref(pc),
                                   ptr(d_info)), "me_kf_update")


def kf_update(ref_uv, cur_uv, alive, new_uv, status, width, height, margin, gap, params: KeyframeSelect | None = None,
              ctx: Context | None = None):
    """me_kf_update on uploaded copies: kf_update_ref's arguments and results,
    the info dict with the block's raw bytes under "bytes"."""
    ctx = ctx or default_context()
    p = params or KeyframeSelect()
    parts = [np.ascontiguousarray(ref_uv, np.float32).reshape(-1, 2), np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2),
             np.ascontiguousarray(new_uv, np.float32).reshape(-1, 2), np.asarray(alive).astype(np.uint8).reshape(-1),
             np.asarray(status).astype(np.uint8).reshape(-1)]
    n = len(parts[0])
    if [len(a) for a in parts] != [n] * 5:
        raise ValueError("kf_update: the per-feature arrays differ in length")
    m = max(n, 1)
    # ref_uv | cur_uv | new_uv | alive | status, then the info block (filled with 0xEE)
    offs = np.cumsum([0, 8 * m, 8 * m, 8 * m, m, m])
    o_info = int(16 * ((offs[-1] + 15) // 16))
    host = np.full(o_info + INFO_BYTES, 0xEE, np.uint8)
    for a, o in zip(parts, offs):
        host[o:o + a.nbytes] = a.view(np.uint8).ravel()
    d = ctx.malloc(host.nbytes)
    try:
        ctx.h2d(d, host)
        o = [int(d + x) for x in offs]
        kf_update_device(ctx, p, o[0], o[1], o[3], o[2], o[4], n, width, height, margin, gap, d + o_info)
        ctx.synchronize()
        ctx.d2h(host, d)
    finally:
        ctx.free(d)
    info = parse_info(host[o_info:])
    info["bytes"] = host[o_info:].copy()
    return (host[offs[1]:offs[1] + 8 * n].view(np.float32).reshape(n, 2).copy(), host[offs[3]:offs[3] + n].copy(), info)
