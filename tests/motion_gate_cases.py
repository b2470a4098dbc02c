"""Inputs of the rigid-motion gate tests (TEST INFRASTRUCTURE, shared by
test_motion_gate.py and test_motion_gate_gpu.py): synthetic stereo
observation sets of a static scene under one camera motion, with a share of
the tracks on a second body, and a small stereo stream with a textured
rectangle that drifts against the background."""
import functools
from dataclasses import dataclass

import numpy as np

W, H = 640, 480
F, CX, CY, B = 0.9 * W, W / 2.0, H / 2.0, 0.12
MARGIN = 24.0
CAM = (F, CX, CY, B, W, H, MARGIN)


def rot(aa):
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa)
    if th == 0:
        return np.eye(3)
    k = aa / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(X):
    return np.stack([F * X[:, 0] / X[:, 2] + CX, F * X[:, 1] / X[:, 2] + CY, F * (X[:, 0] - B) / X[:, 2] + CX], 1)


CAM_MOTION = (rot([0.01, -0.02, 0.005]), np.array([0.02, -0.01, -0.15]))
BODY_MOTION = (rot([0.0, 0.03, 0.0]), np.array([0.25, 0.0, 0.1]))


@dataclass
class Obs:
    prev: np.ndarray     # (n, 3) float32 (u, v, xr) of keyframe t - 1
    cur: np.ndarray      # (n, 3) float32 of keyframe t
    status: np.ndarray   # (n,) uint8
    ok: np.ndarray       # (n,) uint8
    mover: np.ndarray    # (n,) bool: on the second body

    @property
    def args(self):
        return self.prev, self.cur[:, :2], self.cur[:, 2], self.status, self.ok


@functools.lru_cache(maxsize=None)
def scene(n, movers=0.25, noise=0.25, seed=0, zmin=2.0, zmax=12.0):
    """n tracks with depths in [zmin, zmax], the first round(movers * n) of
    them (shuffled below) on a body with a motion of its own, observation
    noise `noise` pixels in every coordinate of both keyframes."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(zmin, zmax, n)
    u, v = rng.uniform(30, W - 30, n), rng.uniform(30, H - 30, n)
    P = np.stack([(u - CX) * Z / F, (v - CY) * Z / F, Z], 1)
    Q = P @ CAM_MOTION[0].T + CAM_MOTION[1]
    mover = np.zeros(n, bool)
    mover[rng.permutation(n)[:int(round(movers * n))]] = True
    Q[mover] = P[mover] @ BODY_MOTION[0].T + BODY_MOTION[1]
    p0 = project(P) + rng.normal(0, noise, (n, 3)) if noise else project(P)
    p1 = project(Q) + rng.normal(0, noise, (n, 3)) if noise else project(Q)
    o = Obs(p0.astype(np.float32), p1.astype(np.float32), np.ones(n, np.uint8), np.ones(n, np.uint8), mover)
    for a in (o.prev, o.cur, o.status, o.ok, o.mover):
        a.setflags(write=False)
    return o


def mixed_flags(o, seed=1):
    """The scene with a tenth of the tracks lost by the tracker, a tenth by the
    matcher (ok bytes 0 .. 2: 2 is a set byte like 1) and a few far points
    (disparity below min_disp in one keyframe or the other)."""
    rng = np.random.default_rng(seed)
    n = len(o.prev)
    st = np.where(rng.random(n) < 0.1, 0, 1).astype(np.uint8)
    ok = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 3, n)).astype(np.uint8)
    prev, cur = o.prev.copy(), o.cur.copy()
    far = rng.random(n) < 0.08
    prev[far & (np.arange(n) % 2 == 0), 2] = prev[far & (np.arange(n) % 2 == 0), 0] - np.float32(0.25)
    cur[far & (np.arange(n) % 2 == 1), 2] = cur[far & (np.arange(n) % 2 == 1), 0] - np.float32(0.25)
    return Obs(prev, cur, st, ok, o.mover)


def collinear(n=40):
    """Every track on one 3-D line in both keyframes: no triangle spans a frame."""
    s = np.linspace(-1.0, 1.0, n)
    P = np.stack([0.5 * s, 0.25 * s, 5.0 + s], 1)
    Q = P + np.array([0.05, 0.0, -0.1])
    return Obs(project(P).astype(np.float32), project(Q).astype(np.float32), np.ones(n, np.uint8), np.ones(n, np.uint8),
               np.zeros(n, bool))


def behind(n=96):
    """A large step forward (2.6 along the optical axis) through a scene with
    depths from 1.5: the points the camera passes lie behind it under the true
    motion.  Their keyframe-t observation is the tracker's own business (here:
    where they were), they stay usable, and under the winner their Y_z <= 0."""
    o = scene(n, 0.0, 0.0, seed=5, zmin=1.5, zmax=8.0)
    u, v = o.prev[:, 0].astype(np.float64), o.prev[:, 1].astype(np.float64)
    Z = F * B / (u - o.prev[:, 2].astype(np.float64))
    P = np.stack([(u - CX) * Z / F, (v - CY) * Z / F, Z], 1)
    Q = P @ rot([0.0, 0.02, 0.0]).T + np.array([0.0, 0.0, -2.6])
    passed = Q[:, 2] < 0.3
    cur = np.where(passed[:, None], o.prev.astype(np.float64), project(np.where(passed[:, None], P, Q)))
    return Obs(o.prev.copy(), cur.astype(np.float32), np.ones(n, np.uint8), np.ones(n, np.uint8), passed)


def build_cli(out_dir):
    """tests/cpp/motion_gate_cli.cpp compiled with the flags of tests/cpp/Makefile; returns the program's path."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = os.path.join(str(out_dir), "motion_gate_cli")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "motion_gate_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def cli_input(o, t, p):
    """The bytes tests/cpp/motion_gate_cli.cpp reads."""
    n = len(o.prev)
    return b"".join([np.array([n, W, H, t, p.n_hyp, p.refine, p.min_inliers], np.int32).tobytes(),
                     np.array([p.seed], np.uint32).tobytes(),
                     np.array([F, CX, CY, B, p.gate_max, p.min_disp], np.float64).tobytes(),
                     np.array([MARGIN], np.float32).tobytes(), np.ascontiguousarray(o.prev).tobytes(),
                     np.ascontiguousarray(o.cur).tobytes(), o.status.tobytes(), o.ok.tobytes()])


# ------------------------------------------------------------------ the loop switch
N_KEYFRAMES = 6
SW, SH = 160, 120
RECT = (44, 34)          # the overlay's width and height
RECT_AT = (52, 44)       # its left-image corner in keyframe 0
RECT_STEP = (3, 0)       # its drift per keyframe, pixels
RECT_DISP = (26, -3)     # its disparity in keyframe 0 and the change per keyframe: it recedes without shrinking,
#                          which no camera motion over a static scene explains (a drift alone at a constant
#                          disparity is a rigid motion this far, narrow-depth background cannot tell from its own)


@functools.lru_cache(maxsize=None)
def stream():
    """(frames, K, first pose, velocity): six 160 x 120 corridor keyframes with
    a textured rectangle pasted into both images of a keyframe at one
    disparity, drifting by RECT_STEP per keyframe whatever the camera does."""
    from klt_fb_cases import texture
    from uasl_motion_estimation_amd import synthetic as S

    _, K, frames = S.stereo_stream(S.SEED0 + 1, SW, SH, N_KEYFRAMES, scene_kind="corridor")
    lut = S.tone_map()
    tex = np.rint(255.0 * texture(77, RECT[0], RECT[1])[32:32 + RECT[1], 32:32 + RECT[0]]).astype(np.uint8)
    out = []
    for k, fr in enumerate(frames):
        x, y = RECT_AT[0] + k * RECT_STEP[0], RECT_AT[1] + k * RECT_STEP[1]
        d = RECT_DISP[0] + k * RECT_DISP[1]
        left, right = fr.left.copy(), fr.right.copy()
        left[y:y + RECT[1], x:x + RECT[0]] = tex
        right[y:y + RECT[1], x - d:x - d + RECT[0]] = lut[tex]
        left.setflags(write=False)
        right.setflags(write=False)
        out.append(S.StereoFrame(left, right, fr.R, fr.t))
    poses = [np.concatenate([fr.t, S.R_to_aa_robust(fr.R)]) for fr in frames]
    return out, K, poses[0], poses[1] - poses[0]


def on_rect(t, uv, inset=2.0):
    """Features of keyframe t that lie on the overlay, `inset` pixels inside its border."""
    x, y = RECT_AT[0] + t * RECT_STEP[0], RECT_AT[1] + t * RECT_STEP[1]
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return ((uv[:, 0] >= x + inset) & (uv[:, 0] <= x + RECT[0] - 1 - inset) & (uv[:, 1] >= y + inset)
            & (uv[:, 1] <= y + RECT[1] - 1 - inset))


def loop_gate():
    """The loop tests' gate: the defaults, with the abstention bound of a stream of a few dozen features."""
    from uasl_motion_estimation_amd.motion_gate import MotionGate

    return MotionGate(min_inliers=6)


def loop_config(**cfg_kw):
    from uasl_motion_estimation_amd import pipeline as PL

    return PL.PipelineConfig(SW, SH, 48, 4, ba_iters=2, **cfg_kw)


def run_loop(vo):
    fr = stream()[0]
    for t in range(N_KEYFRAMES):
        vo.process(t, fr[t].left, fr[t].right)
    vo.finish()
    return vo


_RUNS = {}


def oracle_loop(gate=None):
    """(loop, backend) of the sequential loop on the oracle backend (cached:
    the CPU tests and both GPU loops compare against it)."""
    from pipeline_oracle import OracleBackend
    from uasl_motion_estimation_amd import pipeline as PL

    if gate not in _RUNS:
        _, K, p0, v = stream()
        be = OracleBackend()
        _RUNS[gate] = (run_loop(PL.WindowedStereoVO(loop_config(motion_gate=gate), be, K, p0, v, log_events=True)), be)
    return _RUNS[gate]


def rect_adds(vo):
    """{t: number of "add" events of keyframe t whose feature lies on the overlay}."""
    out = {}
    for ev in vo.events:
        if ev[0] == "add" and on_rect(ev[2], ev[3][:2])[0]:
            out[ev[2]] = out.get(ev[2], 0) + 1
    return out


def events_digest(events):
    """sha256 over the loop's events, every float by its exact hex form."""
    import hashlib

    rows = []
    for e in events:
        if len(e) > 2:
            rows.append("%s %d %d %s" % (e[0], int(e[1]), int(e[2]), " ".join(float(x).hex() for x in e[3])))
        else:
            rows.append("%s %d" % (e[0], int(e[1])))
    return hashlib.sha256("\n".join(rows).encode()).hexdigest()
