"""Frame pose of the VO loop's pushed frames (include/me_hip.h, section A12j):
the rigid motion from the last keyframe's left camera to the current frame's,
estimated from the keyframe's stereo observations and the features' carried
positions in the current frame by an iteratively reweighted (Huber)
Gauss-Newton from a start pose, then an inlier count.  No RANSAC.

The definition is build-defined, integer and FP64 with + - * / sqrt only and
the gate's fixed order for every sum.  frame_pose_ref restates the header in
numpy (elementwise operations only, no dot / sum): it is the checker of the
device kernels (csrc/frame_pose.hip) and what the host backends run.
frame_pose is the binding of me_frame_pose; FramePose holds the parameters and
is what PipelineConfig.frame_pose takes.  err and every word of the info block
are bit-exact."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import Context, FramePoseParamsC, default_context
from .motion_gate import CHUNK, _cayley, _cholesky_solve, _cross

MAX_ITERS = 16
INFO_BYTES = 128  # 5 int32, 3 zero words, 12 doubles


@dataclass(frozen=True)
class FramePose:
    """me_frame_pose_params.  The defaults come from a CPU prototype on
    synthetic points (300 - 2000 points, 0.3 px noise, 20 - 40 % gross
    outliers: from identity it converged within 6 steps for motions up to 10
    degrees and 1 m), not from real data."""
    huber: float = 1.0      # pixels: residuals beyond it are down-weighted by huber / e (> 0)
    gate_max: float = 2.0   # inlier bound on the left-image reprojection error, pixels (> 0)
    min_disp: float = 0.5   # the keyframe disparity of a usable feature is at least this (> 0)
    iters: int = 6          # reweighted Gauss-Newton steps (0 .. 16)
    min_inliers: int = 6    # the pose is valid from this many final inliers (>= 3)

    def __post_init__(self):
        def integer(name, lo, hi):
            v = getattr(self, name)
            if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi):
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}")

        def positive(name):
            v = getattr(self, name)
            try:
                x = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a finite number > 0") from None
            if isinstance(v, bool) or not (math.isfinite(x) and x > 0.0):
                raise ValueError(f"{name} must be a finite number > 0")

        positive("huber")
        positive("gate_max")
        positive("min_disp")
        integer("iters", 0, MAX_ITERS)
        integer("min_inliers", 3, 2 ** 31 - 1)

    def to_c(self) -> FramePoseParamsC:
        c = FramePoseParamsC()
        c.huber, c.gate_max, c.min_disp = float(self.huber), float(self.gate_max), float(self.min_disp)
        c.iters, c.min_inliers = int(self.iters), int(self.min_inliers)
        return c


# ------------------------------------------------------------------ the definition
def _residual(R, t, P, uv, f, cxy):
    """Y (3 arrays), r (2 arrays), e2 of the features P (n, 3) against uv (n, 2) float64 under (R, t)."""
    Y = [((R[i, 0] * P[:, 0] + R[i, 1] * P[:, 1]) + R[i, 2] * P[:, 2]) + t[i] for i in range(3)]
    uh = f * Y[0] / Y[2] + cxy[0]
    vh = f * Y[1] / Y[2] + cxy[1]
    r = [uh - uv[:, 0], vh - uv[:, 1]]
    return Y, r, r[0] * r[0] + r[1] * r[1]


def _irls_step(R, t, P, uv, usable, f, cxy, huber):
    """One reweighted Gauss-Newton step: the new (R, t), or None where the Cholesky stops."""
    n = len(P)
    with np.errstate(all="ignore"):
        Y, r, e2 = _residual(R, t, P, uv, f, cxy)
        act = usable & (Y[2] > 0)
        e = np.sqrt(e2)
        w = np.where(e <= huber, 1.0, huber / e)
        a = f / Y[2]
        q = Y[2] * Y[2]
        z = np.zeros(n)
        g = [[a, z, -(f * Y[0]) / q], [z, a, -(f * Y[1]) / q]]
        J = [_cross(Y, g[m]) + g[m] for m in range(2)]  # row m: (Y x g, g), 6 entries
        terms = []
        for i in range(6):
            for j in range(i, 6):
                terms.append(w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]))
        for i in range(6):
            terms.append(w * (J[0][i] * r[0] + J[1][i] * r[1]))
    nc = -(-n // CHUNK)
    c = np.zeros((nc * CHUNK, 27))
    c[:n] = np.where(act[:, None], np.stack(terms, 1), 0.0)  # a slot that is not act adds +0.0
    c = c.reshape(nc, CHUNK, 27)
    with np.errstate(all="ignore"):
        part = np.zeros((nc, 27))
        for j in range(CHUNK):
            part = part + c[:, j]
        tot = np.zeros(27)
        for k in range(nc):
            tot = tot + part[k]
    A = [[0.0] * 6 for _ in range(6)]
    m = 0
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(tot[m])
            m += 1
    d = _cholesky_solve(A, [-float(tot[21 + i]) for i in range(6)])  # (None for a NaN pivot too: not > 0)
    if d is None:
        return None
    C = _cayley(d[:3])
    Rn = np.array([[(C[i][0] * R[0, j] + C[i][1] * R[1, j]) + C[i][2] * R[2, j] for j in range(3)] for i in range(3)])
    tn = np.array([((C[i][0] * t[0] + C[i][1] * t[1]) + C[i][2] * t[2]) + d[3 + i] for i in range(3)])
    return Rn, tn


def frame_pose_ref(ref, cur_uv, alive, f, cx, cy, baseline, params: FramePose | None = None, start=None):
    """me_frame_pose restated.  ref (n, 3) float32 (u, v, x_r) of the last
    keyframe, cur_uv (n, 2) float32 and alive (n,) bytes of the current frame;
    start: an info dict of this function (its R, t are the start pose iff its
    valid is 1) or None.  Returns (err (n,) float32, info): info is a dict
    with n_usable, n_act, n_inliers, steps, valid and R (3, 3), t (3,) float64."""
    p = params or FramePose()
    ref = np.asarray(ref, np.float32).reshape(-1, 3)
    cur_uv = np.asarray(cur_uv, np.float32).reshape(-1, 2)
    alive = np.asarray(alive).astype(np.uint8).reshape(-1)
    n = len(ref)
    if not (len(cur_uv) == len(alive) == n):
        raise ValueError("frame_pose_ref: the per-feature arrays differ in length")
    f, cxy, b = float(f), (float(cx), float(cy)), float(baseline)
    fb = f * b
    huber = float(p.huber)
    g2 = float(p.gate_max) * float(p.gate_max)
    iters = int(p.iters)
    if start is not None and int(start["valid"]) == 1:
        R, t = np.array(start["R"], np.float64).reshape(3, 3), np.array(start["t"], np.float64).reshape(3)
    else:
        R, t = np.eye(3), np.zeros(3)
    u1, v1 = cur_uv[:, 0], cur_uv[:, 1]
    with np.errstate(all="ignore"):
        d0 = ref[:, 0].astype(np.float64) - ref[:, 2].astype(np.float64)
        usable = (alive != 0) & np.isfinite(u1) & np.isfinite(v1) & (d0 >= float(p.min_disp))
        d = np.where(usable, d0, 1.0)
        Z = fb / d
        P = np.stack([(ref[:, 0].astype(np.float64) - cxy[0]) * Z / f, (ref[:, 1].astype(np.float64) - cxy[1]) * Z / f, Z], 1)
    uv = cur_uv.astype(np.float64)
    n_usable = int(usable.sum())
    steps = 0
    if n_usable >= 3:
        for _ in range(iters):
            step = _irls_step(R, t, P, uv, usable, f, cxy, huber)
            if step is None:
                break
            R, t = step
            steps += 1
    with np.errstate(all="ignore"):
        Y, _, e2 = _residual(R, t, P, uv, f, cxy)
        act = usable & (Y[2] > 0)
        inl = act & (e2 <= g2)
        err = np.where(act, np.sqrt(e2), np.inf).astype(np.float32)
    n_inl = int(inl.sum())
    info = dict(n_usable=n_usable, n_act=int(act.sum()), n_inliers=n_inl, steps=steps,
                valid=int(steps == iters and n_inl >= int(p.min_inliers)), R=R, t=t)
    return err, info


def info_words(info) -> np.ndarray:
    """The device info block of a restated result, as its 32 uint32 words."""
    out = np.zeros(INFO_BYTES // 4, np.uint32)
    out[:5] = np.array([info["n_usable"], info["n_act"], info["n_inliers"], info["steps"], info["valid"]],
                       np.int32).view(np.uint32)
    out[8:] = np.concatenate([np.asarray(info["R"], np.float64).ravel(), np.asarray(info["t"], np.float64)]).view(np.uint32)
    return out


def parse_info(raw) -> dict:
    """The info block me_frame_pose wrote (128 bytes) as frame_pose_ref's dict."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(INFO_BYTES)
    i = raw[:20].view(np.int32)
    d = raw[32:].view(np.float64)
    return dict(n_usable=int(i[0]), n_act=int(i[1]), n_inliers=int(i[2]), steps=int(i[3]), valid=int(i[4]),
                R=d[:9].reshape(3, 3).copy(), t=d[9:].copy())


# ------------------------------------------------------------------ the device call
def frame_pose_device(ctx: Context, params: FramePose, d_ref_uv: int, d_ref_xr: int, d_cur_uv: int, d_alive: int, n: int,
                      f, cx, cy, baseline, d_info: int, d_start: int = 0, d_err: int = 0):
    """One me_frame_pose queued on ctx's stream, everything in device memory."""
    pc = params.to_c()
    V = ctypes.c_void_p

    def ptr(d):
        return V(d) if d else None

    ctx.check(ctx.lib.me_frame_pose(ctx.h, ptr(d_ref_uv), ptr(d_ref_xr), ptr(d_cur_uv), ptr(d_alive), int(n), float(f),
                                    float(cx), float(cy), float(baseline), ctypes.byref(pc), ptr(d_start), ptr(d_err),
                                    ptr(d_info)), "me_frame_pose")


def frame_pose(ref, cur_uv, alive, f, cx, cy, baseline, params: FramePose | None = None, start=None,
               ctx: Context | None = None, alias: bool = False, want_err: bool = True):
    """me_frame_pose on uploaded copies: frame_pose_ref's arguments and results,
    the info dict with the block's raw words under "words" and the raw bytes of
    the whole device block (outputs and the 0xEE guards around them) under
    "block" (as uploaded: "sent") with "o_err" / "o_info", the outputs' offsets in it.  start: an
    info dict (uploaded as a block of its own), or None; alias=True uploads it
    into the info block itself and passes start == info.  want_err=False
    passes err_out = NULL."""
    ctx = ctx or default_context()
    p = params or FramePose()
    ref = np.ascontiguousarray(ref, np.float32).reshape(-1, 3)
    n = len(ref)
    parts = [np.ascontiguousarray(ref[:, :2]), np.ascontiguousarray(ref[:, 2]),
             np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2), np.asarray(alive).astype(np.uint8).reshape(-1)]
    if [len(a) for a in parts] != [n] * 4:
        raise ValueError("frame_pose: the per-feature arrays differ in length")
    m = max(n, 1)
    # ref_uv | ref_xr | cur_uv | alive | guard | err | guard | start | guard | info | guard: outputs and guards 0xEE
    up = lambda x: int(16 * ((x + 15) // 16))  # noqa: E731
    o_ruv, o_rxr, o_cuv, o_al = 0, 8 * m, 12 * m, 20 * m
    o_err = up(21 * m) + 16
    o_start = up(o_err + 4 * m) + 16
    o_info = o_start + INFO_BYTES + 16
    total = o_info + INFO_BYTES + 16
    host = np.full(total, 0xEE, np.uint8)
    for a, o in zip(parts, (o_ruv, o_rxr, o_cuv, o_al)):
        host[o:o + a.nbytes] = a.view(np.uint8).ravel()
    if start is not None:
        o = o_info if alias else o_start
        host[o:o + INFO_BYTES] = info_words(start).view(np.uint8)
    elif alias:
        raise ValueError("frame_pose: alias needs a start block")
    sent = host.copy()
    d = ctx.malloc(total)
    try:
        ctx.h2d(d, host)
        d_start = 0 if start is None else (d + o_info if alias else d + o_start)
        frame_pose_device(ctx, p, d + o_ruv if n else 0, d + o_rxr if n else 0, d + o_cuv if n else 0, d + o_al if n else 0,
                          n, f, cx, cy, baseline, d + o_info, d_start, d + o_err if want_err else 0)
        ctx.synchronize()
        ctx.d2h(host, d)
    finally:
        ctx.free(d)
    info = parse_info(host[o_info:o_info + INFO_BYTES])
    info["words"] = host[o_info:o_info + INFO_BYTES].view(np.uint32).copy()
    info["block"], info["sent"], info["o_err"], info["o_info"] = host, sent, o_err, o_info
    return host[o_err:o_err + 4 * n].view(np.float32).copy(), info
