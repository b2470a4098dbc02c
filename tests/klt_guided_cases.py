"""Inputs of the guided KLT tests (TEST INFRASTRUCTURE, shared by
test_klt_guided.py and test_klt_guided_gpu.py): image pairs whose content moves
further than the unguided tracker can follow, guesses up to 2 px off the true
destination, and the restatement's results on them
(uasl_motion_estimation_amd/klt_ref.py), computed once."""
import functools

import numpy as np

import klt_fb_cases as F

# name -> (w, h, win, max_level, shift): the default tracker; one pyramid level less with a small window; a
# level-0-only tracker on an image narrower than the kernel's staged 32 x 32 region
CASES = {
    "A": (160, 120, 21, 3, (27.25, -21.5)),
    "B": (96, 64, 11, 1, (19.25, -13.5)),
    "C": (30, 40, 7, 0, (5.25, -3.5)),
}
TOL = 0.25  # "correct": status 1 and within TOL px of the truth


@functools.lru_cache(maxsize=None)
def pair(w, h, shift):
    """prev: the klt_fb_cases texture cropped at offset 32.  next: the same content moved by `shift` (bilinear);
    no occluder."""
    a = F.texture(F.SEED, w, h)
    prev = np.rint(255.0 * a[32:32 + h, 32:32 + w]).astype(np.uint8)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    nxt = np.rint(255.0 * F._bilinear(a, xs - shift[0] + 32.0, ys - shift[1] + 32.0)).astype(np.uint8)
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


def points(w, h, win, shift):
    """8 x 8 grid whose true destinations pts + shift all lie inside the image, a window's inset from the border."""
    m = win // 2 + 3
    xs, ys = np.meshgrid(np.linspace(m + max(0.0, -shift[0]), w - 1 - m - max(0.0, shift[0]), 8),
                         np.linspace(m + max(0.0, -shift[1]), h - 1 - m - max(0.0, shift[1]), 8))
    return (np.stack([xs.ravel(), ys.ravel()], -1) + 0.37).astype(np.float32)


def guess_error(n):
    k = np.arange(n)
    return np.stack([((7 * k) % 9 - 4) / 2.0, ((5 * k) % 9 - 4) / 2.0], -1)


class Case:
    def __init__(self, name):
        self.name = name
        self.w, self.h, self.win, self.max_level, self.shift = CASES[name]
        self.prev, self.next = pair(self.w, self.h, self.shift)
        self.pts = points(self.w, self.h, self.win, self.shift)
        self.truth = self.pts.astype(np.float64) + np.array(self.shift)
        self.guess = (self.truth + guess_error(len(self.pts))).astype(np.float32)
        self.kw = dict(win=self.win, max_level=self.max_level)
        for a in (self.pts, self.truth, self.guess):
            a.setflags(write=False)

    def correct(self, uv, st):
        return int(((st == 1) & (np.abs(uv.astype(np.float64) - self.truth).max(1) <= TOL)).sum())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def mixed_guess(c):
    """(guess, ignored): the case's guess with every kind of unusable entry written in, and guess == pts_in;
    `ignored` marks the features that must come out as the plain tracker's."""
    g = c.guess.copy()
    p = c.pts
    w, h = np.float32(c.w), np.float32(c.h)
    bad = {1: (np.nan, g[1, 1]), 4: (g[4, 0], np.nan), 7: (np.nan, np.nan), 10: (np.inf, g[10, 1]),
           13: (g[13, 0], -np.inf), 16: (-0.5, g[16, 1]), 19: (g[19, 0], -1e-6), 22: (w, g[22, 1]),
           25: (g[25, 0], h), 28: (np.nextafter(w, np.float32(np.inf)), g[28, 1]), 31: (1e30, 1e30),
           34: (p[34, 0], p[34, 1]), 37: (p[37, 0], p[37, 1])}
    ignored = np.zeros(len(g), bool)
    for i, v in bad.items():
        g[i] = v
        ignored[i] = True
    return g, ignored


_REF = {}


def ref(name, kind, fb_max=1.0):
    """The restatement on case `name`, cached and read-only: kind "plain" / "guided" -> (uv, st);
    "fb" / "guided_fb" -> (uv, st, fb_err) at fb_max."""
    from uasl_motion_estimation_amd import klt_ref as KR

    key = (name, kind, float(fb_max) if "fb" in kind else None)
    if key not in _REF:
        c = case(name)
        g = c.guess if kind.startswith("guided") else None
        if "fb" in kind:
            r = KR.klt_guided_fb_ref(c.prev, c.next, c.pts, g, fb_max, **c.kw)
        else:
            r = KR.klt_track_ref(c.prev, c.next, c.pts, g, **c.kw)
        for a in r:
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build_cli(out_dir):
    """tests/cpp/klt_guided_cli.cpp compiled with the flags of tests/cpp/Makefile; returns the program's path."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = os.path.join(str(out_dir), "klt_guided_cli")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "klt_guided_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


# ------------------------------------------------------------------ the loop switch
_RUNS = {}


def oracle_loop(**cfg_kw):
    """klt_fb_cases.oracle_loop for configurations with klt_predict (cached: the CPU tests and both GPU loops
    compare against it)."""
    from pipeline_oracle import OracleBackend
    from uasl_motion_estimation_amd import pipeline as PL

    key = tuple(sorted(cfg_kw.items()))
    if key not in _RUNS:
        _, K, p0, v, _ = F.sequence()
        _RUNS[key] = F.run_loop(PL.WindowedStereoVO(F.loop_config(**cfg_kw), OracleBackend(), K, p0, v,
                                                    log_events=True))
    return _RUNS[key]
