"""Rigid-motion gate of the VO loop's tracked features (include/me_hip.h,
section A12h): the camera's frame-to-frame motion estimated from the tracked
stereo observations (a deterministic three-point RANSAC and a short
Gauss-Newton refinement), and the `ok` byte cleared of every track that does
not move with it.

The definition is build-defined, integer and FP64 with + - * / sqrt only and a
fixed order for every sum.  motion_gate_ref restates the header in numpy
(elementwise operations only, no dot / sum): it is the checker of the device
kernels (csrc/motion_gate.hip) and the gate the host backends run.
motion_gate is the binding of me_motion_gate; MotionGate holds the parameters
and is what PipelineConfig.motion_gate takes.  ok, err and every word of the
info block are bit-exact."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np

from ._lib import Context, MotionGateParamsC, default_context

MAX_HYP = 1024
MAX_REFINE = 8
CHUNK = 64  # feature indices per partial of the ordered normal-equation sums
INFO_BYTES = 128  # 5 int32, 3 words of padding, 12 doubles
_M32 = np.uint64(0xFFFFFFFF)


@dataclass(frozen=True)
class MotionGate:
    """me_motion_gate_params.  The defaults are the issue's prototype values on
    synthetic tracks, not measurements of real data."""
    gate_max: float = 2.0   # inlier bound on the stereo reprojection error, pixels (> 0)
    n_hyp: int = 256        # three-point hypotheses (1 .. 1024)
    refine: int = 3         # Gauss-Newton steps on the winner (0 .. 8)
    min_inliers: int = 10   # the gate abstains below this many final inliers (>= 3)
    min_disp: float = 0.5   # both disparities of a usable feature are at least this (> 0)
    seed: int = 0           # uint32

    def __post_init__(self):
        def integer(name, lo, hi):
            v = getattr(self, name)
            if not (isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi):
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}")

        def positive(name):
            try:
                v = float(getattr(self, name))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a finite number > 0") from None
            if not (math.isfinite(v) and v > 0.0):
                raise ValueError(f"{name} must be a finite number > 0")

        positive("gate_max")
        positive("min_disp")
        integer("n_hyp", 1, MAX_HYP)
        integer("refine", 0, MAX_REFINE)
        integer("min_inliers", 3, 2 ** 31 - 1)
        integer("seed", 0, 2 ** 32 - 1)

    def to_c(self) -> MotionGateParamsC:
        c = MotionGateParamsC()
        c.gate_max, c.min_disp = float(self.gate_max), float(self.min_disp)
        c.n_hyp, c.refine, c.min_inliers, c.seed = int(self.n_hyp), int(self.refine), int(self.min_inliers), int(self.seed)
        return c


# ------------------------------------------------------------------ the definition
def _mix(x):
    """lowbias32 on uint64 arrays holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def sample_ref(usable, t: int, p: MotionGate):
    """The three feature indices of every hypothesis: (idx (n_hyp, 3) int64,
    found (n_hyp,) bool).  Slot s takes the first of its 8 attempts that lands
    on a usable feature no earlier slot holds."""
    n = len(usable)
    H = int(p.n_hyp)
    h = np.arange(H, dtype=np.uint64)
    base = (np.uint64((int(t) & 0xFFFFFFFF) * 0x9E3779B1 & 0xFFFFFFFF) + ((h * np.uint64(0x85EBCA77)) & _M32)
            + np.uint64(int(p.seed))) & _M32
    idx = np.zeros((H, 3), np.int64)
    found = np.ones(H, bool)
    for s in range(3):
        got = np.zeros(H, bool)
        for a in range(8):
            key = (base + np.uint64(((s * 8 + a) * 0xC2B2AE3D) & 0xFFFFFFFF)) & _M32
            i = ((_mix(key) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
            take = ~got & usable[i]
            for s0 in range(s):
                take &= i != idx[:, s0]
            idx[take, s] = i[take]
            got |= take
        found &= got
    return idx, found


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _frame(a, b):
    """(e1, e2, e3, valid) of the triangle with edges a, b (lists of 3 arrays)."""
    aa, bb = _dot(a, a), _dot(b, b)
    c = _cross(a, b)
    cc = _dot(c, c)
    valid = cc > (1e-6 * aa) * bb
    la = np.sqrt(np.where(valid, aa, 1.0))
    lc = np.sqrt(np.where(valid, cc, 1.0))
    e1 = [a[k] / la for k in range(3)]
    e3 = [c[k] / lc for k in range(3)]
    return e1, _cross(e3, e1), e3, valid


def hypotheses_ref(P, Q, idx):
    """R (H, 3, 3), t (H, 3), valid (H,) of the sampled triples."""
    Pk = [[P[idx[:, s], k] for k in range(3)] for s in range(3)]
    Qk = [[Q[idx[:, s], k] for k in range(3)] for s in range(3)]
    with np.errstate(all="ignore"):
        e = _frame([Pk[1][k] - Pk[0][k] for k in range(3)], [Pk[2][k] - Pk[0][k] for k in range(3)])
        f = _frame([Qk[1][k] - Qk[0][k] for k in range(3)], [Qk[2][k] - Qk[0][k] for k in range(3)])
        H = len(idx)
        R = np.zeros((H, 3, 3))
        t = np.zeros((H, 3))
        for i in range(3):
            for j in range(3):
                R[:, i, j] = (f[0][i] * e[0][j] + f[1][i] * e[1][j]) + f[2][i] * e[2][j]
        for i in range(3):
            t[:, i] = Qk[0][i] - ((R[:, i, 0] * Pk[0][0] + R[:, i, 1] * Pk[0][1]) + R[:, i, 2] * Pk[0][2])
    return R, t, e[3] & f[3]


def _residual(R, t, P, obs, f, cx, fb):
    """Y (3 arrays), r (3 arrays), e2 for pose(s) R (..., 3, 3), t (..., 3)
    broadcast against the features P (n, 3), obs (n, 3) float64 (u, v, xr)."""
    Y = [((R[..., i, 0, None] * P[:, 0] + R[..., i, 1, None] * P[:, 1]) + R[..., i, 2, None] * P[:, 2])
         + t[..., i, None] for i in range(3)]
    uh = f * Y[0] / Y[2] + cx[0]
    vh = f * Y[1] / Y[2] + cx[1]
    xh = uh - fb / Y[2]
    r = [uh - obs[:, 0], vh - obs[:, 1], xh - obs[:, 2]]
    e2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
    return Y, r, e2


def _cholesky_solve(A, b):
    """x with A x = b by a textbook Cholesky (A: 6 x 6 symmetric, python floats
    are IEEE doubles), or None at the first pivot that is not > 0."""
    n = 6
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s / L[i][i]
    return x


def _cayley(w):
    c = [0.5 * w[0], 0.5 * w[1], 0.5 * w[2]]
    cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    den, om = 1.0 + cc, 1.0 - cc
    sk = [[0.0, -c[2], c[1]], [c[2], 0.0, -c[0]], [-c[1], c[0], 0.0]]
    return [[(om + 2.0 * (c[i] * c[i])) / den if i == j else (2.0 * (c[i] * c[j]) + 2.0 * sk[i][j]) / den
             for j in range(3)] for i in range(3)]


def _gn_step(R, t, P, obs, usable, f, cx, fb, g2):
    """One Gauss-Newton step on the inliers of (R, t): the new (R, t), or None
    where the Cholesky stops."""
    n = len(P)
    with np.errstate(all="ignore"):
        Y, r, e2 = _residual(R, t, P, obs, f, cx, fb)
        inl = usable & (Y[2] > 0) & (e2 <= g2)
        a = f / Y[2]
        q = Y[2] * Y[2]
        z = np.zeros(n)
        g = [[a, z, -(f * Y[0]) / q], [z, a, -(f * Y[1]) / q], [a, z, (fb - f * Y[0]) / q]]
        J = [_cross(Y, g[m]) + g[m] for m in range(3)]  # row m: (Y x g, g), 6 entries
        terms = []
        for i in range(6):
            for j in range(i, 6):
                terms.append((J[0][i] * J[0][j] + J[1][i] * J[1][j]) + J[2][i] * J[2][j])
        for i in range(6):
            terms.append((J[0][i] * r[0] + J[1][i] * r[1]) + J[2][i] * r[2])
    nc = -(-n // CHUNK)
    c = np.zeros((nc * CHUNK, 27))
    c[:n] = np.where(inl[:, None], np.stack(terms, 1), 0.0)  # a slot without an inlier adds +0.0
    c = c.reshape(nc, CHUNK, 27)
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
    d = _cholesky_solve(A, [-float(tot[21 + i]) for i in range(6)])
    if d is None:
        return None
    C = _cayley(d[:3])
    Rn = np.array([[(C[i][0] * R[0, j] + C[i][1] * R[1, j]) + C[i][2] * R[2, j] for j in range(3)] for i in range(3)])
    tn = np.array([((C[i][0] * t[0] + C[i][1] * t[1]) + C[i][2] * t[2]) + d[3 + i] for i in range(3)])
    return Rn, tn


def motion_gate_ref(prev, cur_uv, cur_xr, status, ok, f, cx, cy, baseline, width, height, margin, t,
                    params: MotionGate | None = None):
    """me_motion_gate restated.  prev (n, 3) float32 (u, v, xr) of keyframe
    t - 1, cur_uv (n, 2) and cur_xr (n,) float32 of keyframe t, status / ok
    (n,) bytes.  Returns (ok_out (n,) uint8, err (n,) float32, info): info is a
    dict with n_usable, n_valid, winner (-1: none), n_inliers, abstained and
    R (3, 3), t (3,) float64 (zeros where no hypothesis was valid)."""
    p = params or MotionGate()
    prev = np.asarray(prev, np.float32).reshape(-1, 3)
    cur_uv = np.asarray(cur_uv, np.float32).reshape(-1, 2)
    cur_xr = np.asarray(cur_xr, np.float32).reshape(-1)
    status = np.asarray(status).astype(np.uint8).reshape(-1)
    ok = np.asarray(ok).astype(np.uint8).reshape(-1)
    n = len(prev)
    if not (len(cur_uv) == len(cur_xr) == len(status) == len(ok) == n):
        raise ValueError("motion_gate_ref: the per-feature arrays differ in length")
    f, cxy, b = float(f), (float(cx), float(cy)), float(baseline)
    fb = f * b
    g2 = float(p.gate_max) * float(p.gate_max)
    mg = np.float32(margin)
    info = dict(n_usable=0, n_valid=0, winner=-1, n_inliers=0, abstained=1, R=np.zeros((3, 3)), t=np.zeros(3))
    ok_out = ok.copy()  # (the bytes as they came: a rejected feature's becomes 0)
    err = np.full(n, np.inf, np.float32)
    if n == 0:
        return ok_out, err, info
    u, v = cur_uv[:, 0], cur_uv[:, 1]
    with np.errstate(all="ignore"):
        good = ((status == 1) & (ok != 0) & (u >= mg) & (u < np.float32(width) - mg) & (v >= mg)
                & (v < np.float32(height) - mg))
        d0 = prev[:, 0].astype(np.float64) - prev[:, 2].astype(np.float64)
        d1 = u.astype(np.float64) - cur_xr.astype(np.float64)
        usable = good & (d0 >= float(p.min_disp)) & (d1 >= float(p.min_disp))

        def tri(uu, vv, d):
            d = np.where(usable, d, 1.0)
            Z = fb / d
            return np.stack([(uu.astype(np.float64) - cxy[0]) * Z / f, (vv.astype(np.float64) - cxy[1]) * Z / f, Z], 1)

        P = tri(prev[:, 0], prev[:, 1], d0)
        Q = tri(u, v, d1)
    obs = np.stack([u, v, cur_xr], 1).astype(np.float64)
    info["n_usable"] = int(usable.sum())
    idx, found = sample_ref(usable, t, p)
    Rh, th, valid = hypotheses_ref(P, Q, idx)
    valid &= found
    info["n_valid"] = int(valid.sum())
    if not valid.any():
        return ok_out, err, info
    with np.errstate(all="ignore"):
        Y, _, e2 = _residual(Rh, th, P, obs, f, cxy, fb)
        cnt = (usable[None, :] & (Y[2] > 0) & (e2 <= g2)).sum(axis=1)
    cnt = np.where(valid, cnt, -1)
    w = int(np.argmax(cnt))  # the first maximum
    R, tt = Rh[w].copy(), th[w].copy()
    for _ in range(int(p.refine)):
        step = _gn_step(R, tt, P, obs, usable, f, cxy, fb, g2)
        if step is None:
            break
        R, tt = step
    with np.errstate(all="ignore"):
        Y, _, e2 = _residual(R, tt, P, obs, f, cxy, fb)
        front = usable & (Y[2] > 0)
        inl = front & (e2 <= g2)
        err = np.where(front, np.sqrt(e2), np.inf).astype(np.float32)
    n_inl = int(inl.sum())
    info.update(winner=w, n_inliers=n_inl, R=R, t=tt)
    if n_inl < int(p.min_inliers):
        return ok_out, err, info
    info["abstained"] = 0
    return np.where(usable & ~inl, np.uint8(0), ok_out), err, info


def info_words(info) -> np.ndarray:
    """The device info block of a restated result, as its 32 uint32 words."""
    out = np.zeros(INFO_BYTES // 4, np.uint32)
    out[:5] = np.array([info["n_usable"], info["n_valid"], info["winner"], info["n_inliers"], info["abstained"]],
                       np.int32).view(np.uint32)
    out[8:] = np.concatenate([np.asarray(info["R"], np.float64).ravel(), np.asarray(info["t"], np.float64)]).view(np.uint32)
    return out


def parse_info(raw) -> dict:
    """The info block me_motion_gate wrote (128 bytes) as motion_gate_ref's dict."""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(INFO_BYTES)
    i = raw[:20].view(np.int32)
    d = raw[32:].view(np.float64)
    return dict(n_usable=int(i[0]), n_valid=int(i[1]), winner=int(i[2]), n_inliers=int(i[3]), abstained=int(i[4]),
                R=d[:9].reshape(3, 3).copy(), t=d[9:].copy())


# ------------------------------------------------------------------ the device call
def motion_gate_device(ctx: Context, params: MotionGate, d_prev_uv: int, d_prev_xr: int, d_cur_uv: int, d_cur_xr: int,
                       d_status: int, d_ok: int, n: int, f, cx, cy, baseline, width, height, margin, t,
                       d_ok_out: int, d_err: int = 0, d_info: int = 0):
    """One me_motion_gate queued on ctx's stream, everything in device memory."""
    pc = params.to_c()
    V = ctypes.c_void_p
    ctx.check(ctx.lib.me_motion_gate(ctx.h, V(d_prev_uv), V(d_prev_xr), V(d_cur_uv), V(d_cur_xr), V(d_status), V(d_ok),
                                     int(n), float(f), float(cx), float(cy), float(baseline), int(width), int(height),
                                     float(margin), int(t), ctypes.byref(pc), V(d_ok_out), V(d_err) if d_err else None,
                                     V(d_info) if d_info else None), "me_motion_gate")


def motion_gate(prev, cur_uv, cur_xr, status, ok, f, cx, cy, baseline, width, height, margin, t,
                params: MotionGate | None = None, ctx: Context | None = None, alias: bool = False):
    """me_motion_gate on uploaded copies: motion_gate_ref's arguments and
    results, the info dict with the block's raw words under "words".
    alias=True passes the ok buffer as ok_out."""
    ctx = ctx or default_context()
    p = params or MotionGate()
    prev = np.ascontiguousarray(prev, np.float32).reshape(-1, 3)
    n = len(prev)
    parts = [np.ascontiguousarray(prev[:, :2]), np.ascontiguousarray(prev[:, 2]),
             np.ascontiguousarray(cur_uv, np.float32).reshape(-1, 2), np.ascontiguousarray(cur_xr, np.float32).reshape(-1),
             np.asarray(status).astype(np.uint8).reshape(-1), np.asarray(ok).astype(np.uint8).reshape(-1)]
    if [len(a) for a in parts] != [n] * 6:
        raise ValueError("motion_gate: the per-feature arrays differ in length")
    m = max(n, 1)
    # prev_uv | prev_xr | cur_uv | cur_xr | err | status | ok | ok_out (filled with 0xEE), then the info block
    offs = np.cumsum([0, 8 * m, 4 * m, 8 * m, 4 * m, 4 * m, m, m, m])
    o_info = int(16 * ((offs[-1] + 15) // 16))
    host = np.full(o_info + INFO_BYTES, 0xEE, np.uint8)
    for a, o in zip(parts[:4] + [None] + parts[4:], offs):
        if a is not None:
            host[o:o + a.nbytes] = a.view(np.uint8).ravel()
    d = ctx.malloc(host.nbytes)
    try:
        ctx.h2d(d, host)
        o = [int(d + x) for x in offs]
        motion_gate_device(ctx, p, o[0], o[1], o[2], o[3], o[5], o[6], n, f, cx, cy, baseline, width, height, margin, t,
                           o[6] if alias else o[7], o[4], d + o_info)
        ctx.synchronize()
        ctx.d2h(host, d)
    finally:
        ctx.free(d)
    ok_o = offs[6] if alias else offs[7]
    info = parse_info(host[o_info:])
    info["words"] = host[o_info:].view(np.uint32).copy()
    return host[ok_o:ok_o + n].copy(), host[offs[4]:offs[4] + 4 * n].view(np.float32).copy(), info
