"""Inputs of the frame-pose tests (TEST INFRASTRUCTURE, shared by
test_frame_pose.py and test_frame_pose_gpu.py): the case table of
me_frame_pose, an independent scalar statement of its definition, and the push
loops over keyframe_cases.stream() with the switch on."""
import functools
import math
import os
from dataclasses import dataclass, field

import numpy as np

import keyframe_cases as KC
import motion_gate_cases as G
from uasl_motion_estimation_amd.frame_pose import FramePose, frame_pose_ref
from uasl_motion_estimation_amd.keyframe import KeyframeSelect

F, CX, CY, B = G.F, G.CX, G.CY, G.B
CAM = (F, CX, CY, B)
D = FramePose()
# the chunk (64), workgroup (256) and multi-workgroup boundaries of the kernels
N_LIST = (0, 1, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257, 1025, 2049)


@dataclass
class Case:
    ref: np.ndarray      # (n, 3) float32 (u, v, x_r) of the keyframe
    cur: np.ndarray      # (n, 2) float32
    alive: np.ndarray    # (n,) uint8
    params: FramePose = field(default_factory=FramePose)
    start: object = None  # an info dict, or None
    alias: bool = False   # start == info
    want_err: bool = True

    @property
    def args(self):
        return self.ref, self.cur, self.alive, F, CX, CY, B, self.params

    def with_(self, **kw):
        d = dict(ref=self.ref, cur=self.cur, alive=self.alive, params=self.params, start=self.start, alias=self.alias,
                 want_err=self.want_err)
        d.update(kw)
        return Case(**d)


def block(R, t, valid=1):
    """An info dict to start from."""
    return dict(n_usable=7, n_act=7, n_inliers=7, steps=3, valid=valid, R=np.array(R, np.float64).reshape(3, 3),
                t=np.array(t, np.float64).reshape(3))


def static(n, noise=0.3, seed=0):
    """n features of a static scene under G.CAM_MOTION, every one alive."""
    o = G.scene(n, 0.0, noise, seed=seed) if n else G.scene(1, 0.0, noise, seed=seed)
    return Case(o.prev[:n].copy(), o.cur[:n, :2].copy(), np.ones(n, np.uint8))


def general(n):
    """A tenth of the features dead, a tenth alive at positions that are not
    finite, a tenth too far (disparity below min_disp); alive bytes 1 .. 3."""
    c = static(n, seed=n)
    rng = np.random.default_rng(500 + n)
    r = rng.random(n)
    c.alive[:] = np.where(r < 0.1, 0, rng.integers(1, 4, n)).astype(np.uint8)
    bad = np.flatnonzero((r >= 0.1) & (r < 0.2))
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    c.cur[bad, bad % 2] = vals[bad % 3]
    far = (r >= 0.2) & (r < 0.3)
    c.ref[far, 2] = c.ref[far, 0] - np.float32(0.25)
    return c


def some_alive(n, idx):
    c = static(n)
    c.alive[:] = 0
    c.alive[list(idx)] = 1
    return c


def on_min_disp():
    """d0 exactly min_disp (usable) on the even features, one float below it on the odd ones."""
    c = static(66, seed=3)
    u = np.rint(c.ref[:, 0]).astype(np.float32)  # (integers: u - 0.5 is exact in float32)
    c.ref[:, 0] = u
    xr = u - np.float32(0.5)
    xr[1::2] = np.nextafter(xr[1::2], np.float32(np.inf))
    c.ref[:, 2] = xr
    d0 = u.astype(np.float64) - xr.astype(np.float64)
    assert np.all(d0[::2] == 0.5) and np.all(d0[1::2] < 0.5) and np.all(d0[1::2] > 0.4999)
    return c


def not_finite():
    c = static(130, seed=4)
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    k = np.arange(0, 130, 3)
    c.cur[k, k % 2] = vals[k % 3]
    return c


def behind():
    """A start pose that puts the near features behind the camera (Y_2 <= 0)."""
    c = static(200, seed=5)
    return c.with_(start=block(np.eye(3), [0.0, 0.0, -6.0]))


def identical(n=70):
    """Every feature the same: H has rank 2, the Cholesky stops."""
    c = static(n)
    c.ref[:] = c.ref[0]
    c.cur[:] = c.cur[0]
    return c


def outliers(n=300, share=0.3):
    c = static(n, seed=6)
    rng = np.random.default_rng(61)
    bad = rng.random(n) < share
    c.cur[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2)).astype(np.float32)
    return c


def overflow():
    """A start translation of 1e150: the Jacobian's squares pass the largest double, the sums hold inf."""
    return static(130, seed=7).with_(start=block(np.eye(3), [1e150, 0.0, 0.0]))


def warm(n=257):
    """A valid start block: the truth, a little off."""
    return static(n, seed=8).with_(start=block(G.rot([0.012, -0.018, 0.004]), G.CAM_MOTION[1] + [0.01, 0.0, -0.02]))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, the whole table."""
    out = {f"general-n{n}": general(n) for n in N_LIST}
    out["all-dead-n65"] = some_alive(65, [])
    out["all-dead-n257"] = some_alive(257, [])
    out["usable-2"] = some_alive(70, [1, 66])
    out["usable-3"] = some_alive(70, [1, 66, 69])
    out["usable-5-below-min-inliers"] = some_alive(130, [0, 63, 64, 100, 129])
    out["on-min-disp"] = on_min_disp()
    out["not-finite"] = not_finite()
    out["behind"] = behind()
    out["identical"] = identical()
    out["outliers-30"] = outliers()
    out["overflow"] = overflow()
    out["iters-0"] = static(257, seed=9).with_(params=FramePose(iters=0))
    out["iters-0-warm"] = warm().with_(params=FramePose(iters=0))
    out["iters-16"] = static(257, seed=9).with_(params=FramePose(iters=16))
    out["start-valid"] = warm()
    out["start-invalid"] = warm().with_(start=block(G.rot([0.5, 0.5, 0.5]), [3.0, -2.0, 1.0], valid=0))
    out["start-valid-word-2"] = warm().with_(start=block(G.rot([0.5, 0.5, 0.5]), [3.0, -2.0, 1.0], valid=2))
    out["start-is-info"] = warm().with_(alias=True)
    out["start-is-info-n0"] = warm(0).with_(alias=True)
    out["start-is-info-invalid"] = warm(65).with_(start=block(np.eye(3), [0.0, 0.0, 0.0], valid=0), alias=True)
    out["no-err-out"] = general(257).with_(want_err=False)
    out["loose"] = outliers(130).with_(params=FramePose(huber=0.25, gate_max=0.75, min_disp=2.0, iters=3, min_inliers=40))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """frame_pose_ref's (err, info) of a case, computed once."""
    c = cases()[name]
    err, info = frame_pose_ref(*c.args, start=c.start)
    err.setflags(write=False)
    return err, info


# ------------------------------------------------------------------ the definition again, scalar
def _div(a, b):
    """IEEE a / b on python floats (python raises where IEEE divides by zero)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan  # (also NaN for NaN: the comparison is false)


def _cholesky(A, b):
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = _sqrt(s)
        for i in range(j + 1, 6):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = _div(s, L[j][j])
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = _div(s, L[i][i])
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = _div(s, L[i][i])
    return x


def scalar_statement(c: Case):
    """include/me_hip.h A12j read top to bottom with python floats, one
    feature at a time: (err list of python floats rounded to float32, info
    dict with R, t as nested lists).  Shares no code with frame_pose_ref."""
    p = c.params
    n = len(c.ref)
    fb = F * B
    feats = []
    for k in range(n):
        u0, v0, x0 = (float(x) for x in c.ref[k])
        u1, v1 = (float(x) for x in c.cur[k])
        d0 = u0 - x0
        usable = c.alive[k] != 0 and math.isfinite(u1) and math.isfinite(v1) and d0 >= p.min_disp
        P = None
        if usable:
            Z = _div(fb, d0)
            P = (_div((u0 - CX) * Z, F), _div((v0 - CY) * Z, F), Z)
        feats.append((usable, P, u1, v1))
    if c.start is not None and int(c.start["valid"]) == 1:
        R = [[float(c.start["R"][i][j]) for j in range(3)] for i in range(3)]
        t = [float(x) for x in c.start["t"]]
    else:
        R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        t = [0.0, 0.0, 0.0]

    def residual(P, u1, v1):
        Y = [((R[i][0] * P[0] + R[i][1] * P[1]) + R[i][2] * P[2]) + t[i] for i in range(3)]
        uh = _div(F * Y[0], Y[2]) + CX
        vh = _div(F * Y[1], Y[2]) + CY
        r = (uh - u1, vh - v1)
        return Y, r, r[0] * r[0] + r[1] * r[1]

    n_usable = sum(1 for f in feats if f[0])
    steps = 0
    if n_usable >= 3:
        for _ in range(p.iters):
            parts = []
            for c0 in range(0, n, 64):
                acc = [0.0] * 27
                for k in range(c0, c0 + 64):
                    term = [0.0] * 27
                    if k < n and feats[k][0]:
                        _, P, u1, v1 = feats[k]
                        Y, r, e2 = residual(P, u1, v1)
                        if Y[2] > 0.0:
                            e = _sqrt(e2)
                            w = 1.0 if e <= p.huber else _div(p.huber, e)
                            a, q = _div(F, Y[2]), Y[2] * Y[2]
                            g = [(a, 0.0, _div(-(F * Y[0]), q)), (0.0, a, _div(-(F * Y[1]), q))]
                            J = []
                            for m in range(2):
                                gm = g[m]
                                J.append((Y[1] * gm[2] - Y[2] * gm[1], Y[2] * gm[0] - Y[0] * gm[2],
                                          Y[0] * gm[1] - Y[1] * gm[0], gm[0], gm[1], gm[2]))
                            s = 0
                            for i in range(6):
                                for j in range(i, 6):
                                    term[s] = w * (J[0][i] * J[0][j] + J[1][i] * J[1][j])
                                    s += 1
                            for i in range(6):
                                term[s] = w * (J[0][i] * r[0] + J[1][i] * r[1])
                                s += 1
                    acc = [x + y for x, y in zip(acc, term)]
                parts.append(acc)
            tot = [0.0] * 27
            for acc in parts:
                tot = [x + y for x, y in zip(tot, acc)]
            A = [[0.0] * 6 for _ in range(6)]
            s = 0
            for i in range(6):
                for j in range(i, 6):
                    A[i][j] = A[j][i] = tot[s]
                    s += 1
            d = _cholesky(A, [-tot[21 + i] for i in range(6)])
            if d is None:
                break
            cv = [0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]
            cc = (cv[0] * cv[0] + cv[1] * cv[1]) + cv[2] * cv[2]
            den, om = 1.0 + cc, 1.0 - cc
            sk = [[0.0, -cv[2], cv[1]], [cv[2], 0.0, -cv[0]], [-cv[1], cv[0], 0.0]]
            C = [[_div(om + 2.0 * (cv[i] * cv[i]), den) if i == j else _div(2.0 * (cv[i] * cv[j]) + 2.0 * sk[i][j], den)
                  for j in range(3)] for i in range(3)]
            Rn = [[(C[i][0] * R[0][j] + C[i][1] * R[1][j]) + C[i][2] * R[2][j] for j in range(3)] for i in range(3)]
            tn = [((C[i][0] * t[0] + C[i][1] * t[1]) + C[i][2] * t[2]) + d[3 + i] for i in range(3)]
            R, t = Rn, tn
            steps += 1
    g2 = p.gate_max * p.gate_max
    err, n_act, n_inl = [], 0, 0
    for usable, P, u1, v1 in feats:
        e = math.inf
        if usable:
            Y, _, e2 = residual(P, u1, v1)
            if Y[2] > 0.0:
                n_act += 1
                n_inl += 1 if e2 <= g2 else 0
                e = _sqrt(e2)
        with np.errstate(over="ignore"):  # (a double past float32's range rounds to inf, as the cast on the device does)
            err.append(np.float32(e))
    return err, dict(n_usable=n_usable, n_act=n_act, n_inliers=n_inl, steps=steps,
                     valid=int(steps == p.iters and n_inl >= p.min_inliers), R=R, t=t)


# ------------------------------------------------------------------ the loops
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_pose_default.txt")
SELECT = KeyframeSelect()


def loop_config(frame_pose=D, **kw):
    return KC.loop_config(SELECT, frame_pose=frame_pose, **kw)


_RUN = []


def oracle_push():
    """(loop, keyframe index per frame) of the push loop on the oracle backend with the switch on (cached)."""
    from pipeline_oracle import OracleBackend
    from uasl_motion_estimation_amd import pipeline as PL

    if not _RUN:
        _, K, p0, v = KC.stream()
        vo = PL.WindowedStereoVO(loop_config(), OracleBackend(), K, p0, v, log_events=True)
        _RUN.append((vo, KC.run_push(vo)))
    return _RUN[0]


def record_lines(log):
    """The golden file's lines of a loop's records (kf_log, or NativeStereoVO.frame_pose_log): per pushed
    frame after the first its number, t_ref, valid, n_inliers, steps, then R_rel and t_rel as float.hex."""
    out = []
    for r in log:
        if "t_ref" not in r:
            continue
        vals = [float(x) for x in np.asarray(r["R_rel"], np.float64).ravel()] + [float(x) for x in r["t_rel"]]
        out.append("%d %d %d %d %d %s" % (r["frame"], r["t_ref"], r["pose_valid"], r["n_inliers"], r["steps"],
                                          " ".join(x.hex() for x in vals)))
    return out


def golden_lines():
    with open(GOLDEN) as fh:
        return [ln.strip() for ln in fh if ln.strip()]


def true_motion(t_ref_frame, frame):
    """(R, t) from the camera of stream frame t_ref_frame to that of `frame`, from the stream's own poses."""
    fr = KC.stream()[0]
    Rk, tk, Ri, ti = fr[t_ref_frame].R, fr[t_ref_frame].t, fr[frame].R, fr[frame].t
    R = Ri @ Rk.T
    return R, ti - R @ tk


def build_cli(out_dir):
    """tests/cpp/frame_pose_cli.cpp compiled with the flags of tests/cpp/Makefile; returns the program's path."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = os.path.join(str(out_dir), "frame_pose_cli")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "frame_pose_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def cli_input(p=D):
    """The bytes tests/cpp/frame_pose_cli.cpp reads: keyframe_cli's input, then the frame-pose parameters."""
    return (KC.cli_input(SELECT) + np.array([p.iters, p.min_inliers], np.int32).tobytes()
            + np.array([p.huber, p.gate_max, p.min_disp], np.float64).tobytes())
