"""Inputs of the forward-backward KLT tests (TEST INFRASTRUCTURE, shared by
test_klt_fb.py and test_klt_fb_gpu.py): image pairs on which the check has
something to reject, and its oracle restatement (pipeline.klt_fb_host around
oracle/klt.cpp)."""
import functools

import numpy as np

# (w, h, win, max_level): default tracker; one pyramid level less than the default with a small window;
# a level-0-only tracker on an image narrower than the kernel's staged 32 x 32 region
SHAPES = [(160, 120, 21, 3), (96, 64, 11, 1), (30, 40, 7, 0)]
SEED = 7
SHIFT = (3.25, -2.5)  # content motion prev -> next, pixels


def texture(seed, w, h):
    """(h + 64, w + 64) FP64 in [0, 1]: uniform noise smoothed twice with the 5-point cross average."""
    a = np.random.default_rng(seed).random((h + 64, w + 64))
    for _ in range(2):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    return (a - a.min()) / (a.max() - a.min())


def _bilinear(a, xs, ys):
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx, fy = xs - x0, ys - y0
    return ((1 - fy) * ((1 - fx) * a[y0, x0] + fx * a[y0, x0 + 1])
            + fy * ((1 - fx) * a[y0 + 1, x0] + fx * a[y0 + 1, x0 + 1]))


@functools.lru_cache(maxsize=None)
def image_pair(w, h, seed=SEED):
    """prev: a crop of the texture.  next: the same content moved by SHIFT,
    with the columns x >= 2w // 3 replaced by a second texture (an occluder:
    tracks that end there have nothing to return to)."""
    a, b = texture(seed, w, h), texture(seed + 1000, w, h)
    prev = np.rint(255.0 * a[32:32 + h, 32:32 + w]).astype(np.uint8)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    nxt = _bilinear(a, xs - SHIFT[0] + 32.0, ys - SHIFT[1] + 32.0)
    x_occ = 2 * w // 3
    nxt[:, x_occ:] = b[32:32 + h, 32:32 + w][:, x_occ:]
    nxt = np.rint(255.0 * nxt).astype(np.uint8)
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


def grid_points(w, h, win):
    m = win // 2 + 3
    xs, ys = np.meshgrid(np.linspace(m, w - 1 - m, 8), np.linspace(m, h - 1 - m, 8))
    return (np.stack([xs.ravel(), ys.ravel()], -1) + 0.37).astype(np.float32)


_REF = {}


def oracle_fb(w, h, win, max_level, fb_max, pts=None, key=None):
    """(pts_out, status, fb_err, sf, sb) of the two-call oracle restatement (cached per key)."""
    import oracle as O
    from uasl_motion_estimation_amd.pipeline import klt_fb_host

    k = (w, h, win, max_level, float(fb_max), key)
    if pts is not None and key is None:
        k = None
    if k is not None and k in _REF:
        return _REF[k]
    prev, nxt = image_pair(w, h)
    if pts is None:
        pts = grid_points(w, h, win)
    kw = dict(win=win, max_level=max_level)
    seen = []

    def klt(a, b, p):
        out = O.klt(a, b, p, **kw)
        seen.append(out[1].copy())
        return out

    q, st, err = klt_fb_host(klt, prev, nxt, pts, fb_max)
    res = (q, st, err, seen[0], seen[1])
    for a in res:
        a.setflags(write=False)
    if k is not None:
        _REF[k] = res
    return res


def classes(st, err, sf, sb):
    """(#accepted, #both passes ok but rejected by distance, #forward ok and backward lost)."""
    both = (sf == 1) & (sb == 1)
    return int((st == 1).sum()), int((both & (st == 0)).sum()), int(((sf == 1) & (sb == 0)).sum())


def assert_classes_populated(st, err, sf, sb):
    """An input that stops exercising the gate fails the test instead of hiding."""
    acc, far, lost = classes(st, err, sf, sb)
    assert acc >= 8 and far >= 8 and lost >= 1, (acc, far, lost)


def identity_case():
    """prev = next (the 160 x 120 texture), features at integer positions (14 + 12 i, 14 + 12 j)."""
    prev, _ = image_pair(160, 120)
    xs, ys = np.meshgrid(np.arange(14, 160 - 14, 12), np.arange(14, 120 - 14, 12))
    return prev, np.stack([xs.ravel(), ys.ravel()], -1).astype(np.float32)


def build_cli(out_dir):
    """tests/cpp/klt_fb_cli.cpp compiled with the flags of tests/cpp/Makefile; returns the program's path."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = os.path.join(str(out_dir), "klt_fb_cli")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra","-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "klt_fb_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


# ------------------------------------------------------------------ the loop switch
N_KEYFRAMES = 6


@functools.lru_cache(maxsize=None)
def sequence():
    from uasl_motion_estimation_amd import pipeline as PL

    return PL.synthetic_sequence(1, N_KEYFRAMES)


def loop_config(**cfg_kw):
    """Config 1 (640 x 480, 200 features), window 4, 2 BA iterations."""
    from uasl_motion_estimation_amd import pipeline as PL

    cfg = PL.PipelineConfig.from_config(1, ba_iters=2, **cfg_kw)
    cfg.window = 4
    return cfg


def run_loop(vo):
    fr = sequence()[0]
    for t in range(N_KEYFRAMES):
        vo.process(t, fr[t].left, fr[t].right)
    vo.finish()
    return vo


_RUNS = {}


def oracle_loop(frames=None, **cfg_kw):
    """The sequential loop on the oracle backend (cached: the CPU tests and both GPU loops compare against it)."""
    from pipeline_oracle import OracleBackend
    from uasl_motion_estimation_amd import pipeline as PL

    key = tuple(sorted(cfg_kw.items()))
    if key not in _RUNS:
        _, K, p0, v, _ = sequence()
        _RUNS[key] = run_loop(PL.WindowedStereoVO(loop_config(**cfg_kw), OracleBackend(), K, p0, v, log_events=True))
    return _RUNS[key]
