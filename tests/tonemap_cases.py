"""Inputs of the 16-bit ingest tests (TEST INFRASTRUCTURE, shared by
test_tonemap.py and test_tonemap_gpu.py): a restatement by sorting, the images
of the radix-select and division cases, the 16-bit stream of the loop tests
and the oracle-backend loops on it."""
import functools

import numpy as np

import klt_fb_cases as KC
from uasl_motion_estimation_amd.tonemap import ToneMap, tonemap_ref

EXACT = ToneMap(0, 0, 1, 256)  # no clipping, no widening, no memory: the window is the frame's min .. max


def window_by_sorting(img16, params):
    """Step 1 of the definition without a histogram: sort, then index.  c[v] > k
    first holds at the value of sorted pixel k; c[v] >= m at that of pixel m - 1."""
    s = np.sort(np.asarray(img16).ravel())
    n = s.size
    k_lo, k_hi = params.lo_ppm * n // 10 ** 6, params.hi_ppm * n // 10 ** 6
    return int(s[k_lo]), int(s[n - k_hi - 1])


def brute_force(img16, params, state=None):
    """The whole definition, pixel by pixel in Python integers (small images only)."""
    lo, hi = window_by_sorting(img16, params)
    s = hi - lo
    if s < params.min_span:
        lo = max(lo - (params.min_span - s) // 2, 0)
        hi = lo + params.min_span
        if hi > 65535:
            hi, lo = 65535, 65535 - params.min_span
    if state is None or state[2] == 0:
        lo_q8, hi_q8, frames = lo * 256, hi * 256, 0
    else:
        lo_q8, hi_q8, frames = state
        lo_q8 += (((lo * 256) - lo_q8) * params.alpha_q8) // 256
        hi_q8 += (((hi * 256) - hi_q8) * params.alpha_q8) // 256
    lo_u, hi_u = lo_q8 // 256, (hi_q8 + 255) // 256
    span = max(1, hi_u - lo_u)
    a = np.asarray(img16)
    out = np.zeros(a.shape, np.uint8)
    for idx, v in np.ndenumerate(a):
        v = int(v)
        out[idx] = 0 if v < lo_u else min(255, ((min(v, hi_u) - lo_u) * 255 + span // 2) // span)
    return out, (lo_q8, hi_q8, min(frames + 1, 2 ** 31 - 1))


# ------------------------------------------------------------------ images
SIZES = [(1, 1), (7, 3), (9, 5), (61, 7), (64, 48)]  # (w, h): ragged and unaligned access


@functools.lru_cache(maxsize=None)
def noise14(w, h, seed=3):
    a = np.random.default_rng(seed).integers(0, 1 << 14, (h, w), dtype=np.uint16)
    a.setflags(write=False)
    return a


def _ro(a):
    a = np.ascontiguousarray(a, np.uint16)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def select_case(name):
    """(image, params) of a radix-select case, 97 x 53 unless the name says otherwise."""
    w, h = 97, 53
    n = w * h
    rng = np.random.default_rng(11)
    if name == "same_high_byte":  # a 200-count scene inside high byte 0x1b
        return _ro(0x1b10 + rng.integers(0, 200, (h, w))), ToneMap(1000, 1000, 16, 256)
    if name == "adjacent_high_bytes":
        return _ro(0x1bc0 + rng.integers(0, 200, (h, w))), ToneMap(1000, 1000, 16, 256)
    if name == "far_high_bytes":
        return _ro(rng.integers(300, 60000, (h, w))), ToneMap(20000, 30000, 16, 256)
    if name in ("rank_on_first_pixel_of_a_bin", "rank_on_last_pixel_of_a_bin"):
        # sorted: 1000 pixels of 0x1000, then the rest in 0x2000 + (0 .. 99); k_lo = 1000 is the first pixel of
        # the bin after 0x1000 (lo = 0x2000), k_lo = 999 the last of it (lo = 0x1000); the same from the top
        a = np.empty(n, np.int64)
        a[:1000] = 0x1000
        a[1000:n - 1000] = 0x2000 + rng.integers(0, 100, n - 2000)
        a[n - 1000:] = 0x3005
        rng.shuffle(a)
        k = 1000 if name.startswith("rank_on_first") else 999
        ppm = -(-k * 10 ** 6 // n)  # the smallest ppm with floor(ppm n / 10^6) = k
        assert ppm * n // 10 ** 6 == k
        return _ro(a.reshape(h, w)), ToneMap(ppm, ppm, 16, 256)
    if name == "ppm_0_0":
        return _ro(rng.integers(5000, 9000, (h, w))), ToneMap(0, 0, 16, 256)
    if name == "ppm_499999":
        return _ro(rng.integers(5000, 9000, (h, w))), ToneMap(499999, 499999, 16, 256)
    if name == "low_entropy_300x200":  # 16 levels, several workgroups
        tex = np.rint(255.0 * KC.texture(11, 300, 200)[32:232, 32:332]).astype(np.int64)
        return _ro(100 * 64 + tex // 16), ToneMap(1000, 1000, 4, 256)
    raise KeyError(name)


SELECT_CASES = ["same_high_byte", "adjacent_high_bytes", "far_high_bytes", "rank_on_first_pixel_of_a_bin",
                "rank_on_last_pixel_of_a_bin", "ppm_0_0", "ppm_499999", "low_entropy_300x200"]

SPANS = [1, 2, 3, 255, 256, 257, 510, 32767, 32768, 65534, 65535] + \
    [int(s) for s in np.random.default_rng(17).integers(1, 65536, 32)]


def division_image(span, lo=None):
    """256 x 257 of lo + (i mod (span + 1)): with EXACT the window is lo .. lo + span
    and (for span + 1 <= 65 792 pixels: always) every numerator of that span occurs."""
    lo = (65535 - span) // 2 if lo is None else lo
    i = np.arange(256 * 257, dtype=np.int64)
    return (lo + i % (span + 1)).astype(np.uint16).reshape(257, 256)


# ------------------------------------------------------------------ the loops
def wide_frame(img8, t):
    """The 16-bit twin of an 8-bit frame at keyframe t: 7000 + 40 t + 2 v."""
    return (7000 + 40 * t + 2 * np.asarray(img8).astype(np.int64)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def wide_sequence():
    """The config-1 sequence of klt_fb_cases as a 16-bit stream."""
    fr = KC.sequence()[0]
    out = []
    for t in range(KC.N_KEYFRAMES):
        pair = (wide_frame(fr[t].left, t), wide_frame(fr[t].right, t))
        for a in pair:
            a.setflags(write=False)
        out.append(pair)
    return out


@functools.lru_cache(maxsize=None)
def high_byte_sequence():
    """What reaches the loop today: the high byte of every pixel (imread_gray's rule)."""
    return [((L >> 8).astype(np.uint8), (R >> 8).astype(np.uint8)) for L, R in wide_sequence()]


@functools.lru_cache(maxsize=None)
def mapped_sequence(params=ToneMap()):
    """wide_sequence tone-mapped outside the loop with tonemap_ref, a state per camera."""
    out, sl, sr = [], None, None
    for L, R in wide_sequence():
        l8, sl = tonemap_ref(L, params, sl)
        r8, sr = tonemap_ref(R, params, sr)
        out.append((l8, r8))
    return out


def run_frames(vo, frames):
    for t, (L, R) in enumerate(frames):
        vo.process(t, L, R)
    vo.finish()
    return vo


_RUNS = {}


def oracle_loop(frames_id, **cfg_kw):
    """The sequential loop on the oracle backend over the 16-bit stream ("wide"),
    its high bytes ("high"), the stream mapped outside ("outside") or the 8-bit
    stream it was made from ("plain"), cached per (input, switches)."""
    from pipeline_oracle import OracleBackend
    from uasl_motion_estimation_amd import pipeline as PL

    key = (frames_id, tuple(sorted(cfg_kw.items(), key=lambda kv: kv[0])))
    if key not in _RUNS:
        fr, K, p0, v, _ = KC.sequence()
        frames = {"wide": wide_sequence, "high": high_byte_sequence, "outside": mapped_sequence,
                  "plain": lambda: [(fr[t].left, fr[t].right) for t in range(KC.N_KEYFRAMES)]}[frames_id]()
        vo = PL.WindowedStereoVO(KC.loop_config(**cfg_kw), OracleBackend(), K, p0, v, log_events=True)
        _RUNS[key] = run_frames(vo, frames)
    return _RUNS[key]


def build_cli(out_dir):
    """tests/cpp/tonemap_cli.cpp compiled as equalise_cases.build_cli compiles its caller; returns the program's path."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "uasl_motion_estimation_amd")
    exe = os.path.join(str(out_dir), "tonemap_cli")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "tonemap_cli.cpp"), "-L" + libdir, "-l:libme_hip.so",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe
