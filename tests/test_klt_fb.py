"""Forward-backward KLT check (include/me_hip.h A12c), the parts that need no
GPU: the numpy restatement pipeline.klt_fb_host around the oracle tracker
(oracle/klt.cpp), the loop switch PipelineConfig.klt_fb_max on the oracle
backend, the configuration checks and the C++ overload.  The device side is
tests/test_klt_fb_gpu.py.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import klt_fb_cases as C
from uasl_motion_estimation_amd import _lib
from uasl_motion_estimation_amd import pipeline as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, WIN, LEVELS = C.SHAPES[0]


def test_host_restatement_on_the_occluded_pair(oracle):
    prev, nxt = C.image_pair(W, H)
    pts = C.grid_points(W, H, WIN)
    q, st, err, sf, sb = C.oracle_fb(W, H, WIN, LEVELS, 0.5)
    C.assert_classes_populated(st, err, sf, sb)
    assert C.classes(st, err, sf, sb) == (43, 18, 3)  # the oracle's own counts on this input
    fwd, fst = oracle.klt(prev, nxt, pts, win=WIN, max_level=LEVELS)
    assert np.array_equal(q.view(np.uint32), fwd.view(np.uint32)) and np.array_equal(sf, fst)
    both = (sf == 1) & (sb == 1)
    assert np.array_equal(np.isinf(err), ~both) and np.all(err[~both] > 0)
    assert np.all(np.isfinite(err[both])) and np.all(err[both] >= 0)
    # status is the distance test on the tracked features, in FP64 on the unrounded distance
    back, _ = oracle.klt(nxt, prev, q, win=WIN, max_level=LEVELS)
    d = back.astype(np.float64) - pts.astype(np.float64)
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    assert np.array_equal(st == 1, both & (d2 <= 0.25))
    assert np.array_equal(err[both], np.sqrt(d2[both]).astype(np.float32))
    _, st1, err1, _, _ = C.oracle_fb(W, H, WIN, LEVELS, 1.0)
    assert np.all(st1[st == 1] == 1) and st1.sum() > st.sum()  # a superset, and a proper one here
    assert np.array_equal(err1.view(np.uint32), err.view(np.uint32))  # the distance does not depend on the bound
    _, sti, _, _, _ = C.oracle_fb(W, H, WIN, LEVELS, math.inf)
    assert np.array_equal(sti, both.astype(np.uint8))


@pytest.mark.parametrize("shape", C.SHAPES[1:])
def test_small_pairs_exercise_every_class(oracle, shape):
    for fb_max in (0.5, 1.0):
        C.assert_classes_populated(*C.oracle_fb(*shape, fb_max)[1:])


def test_host_restatement_identity(oracle):
    img, pts = C.identity_case()
    q, st, err = PL.klt_fb_host(oracle.klt, img, img, pts, 0.5)
    assert len(pts) == 88 and np.all(st == 1) and np.all(err == 0.0)
    assert np.array_equal(q.view(np.uint32), pts.view(np.uint32))


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan])
def test_host_restatement_rejects_a_bound_that_is_not_positive(bad):
    with pytest.raises(ValueError):
        PL.klt_fb_host(lambda a, b, p: (p, np.ones(len(p), np.uint8)), None, None, np.zeros((1, 2), np.float32), bad)


# ------------------------------------------------------------------ the loop switch
N_KEYFRAMES = C.N_KEYFRAMES
oracle_loop = C.oracle_loop


@pytest.fixture(scope="module")
def seq1():
    return C.sequence()


def test_loop_switch_off_is_the_default_loop(oracle, seq1):
    a, b = oracle_loop(seq1), oracle_loop(seq1, klt_fb_max=0.0)
    assert PL.PipelineConfig.from_config(1).klt_fb_max == 0.0 and PL.Backend.klt_fb_max == 0.0
    assert a.events == b.events and np.array_equal(a.ids, b.ids) and np.array_equal(a.X, b.X)
    assert sorted(a.poses) == sorted(b.poses) and all(np.array_equal(a.poses[t], b.poses[t]) for t in a.poses)


def test_loop_switch_on_drops_tracks_that_do_not_return(oracle, seq1):
    off, on = oracle_loop(seq1), oracle_loop(seq1, klt_fb_max=0.5)
    assert on.be.klt_fb_max == 0.5
    n_off, n_on = [r.n_tracked for r in off.results], [r.n_tracked for r in on.results]
    print("n_tracked off", n_off, "on", n_on)
    assert len(n_on) == len(n_off) == N_KEYFRAMES
    assert all(a <= b for a, b in zip(n_on, n_off)), (n_on, n_off)
    assert 0 < n_on[1] < n_off[1], (n_on, n_off)
    assert all(np.all(np.isfinite(p)) for p in on.poses.values())


# ------------------------------------------------------------------ configuration
@pytest.mark.parametrize("bad", [-1, -1e-9, math.nan])
def test_pipeline_config_rejects_a_negative_or_nan_bound(bad):
    with pytest.raises(ValueError):
        PL.PipelineConfig(640, 480, 200, 4, klt_fb_max=bad)
    with pytest.raises(ValueError):
        PL.PipelineConfig.from_config(1, klt_fb_max=bad)


def test_native_default_config_leaves_the_check_off():
    lib = _lib.load_library()
    c = _lib.VOLoopConfigC()
    c.klt_fb_max = 123.0
    lib.me_vo_loop_default_config(ctypes.byref(c))
    assert c.klt_fb_max == 0.0
    assert _lib.VOLoopConfigC._fields_[-1][0] == "klt_fb_max"  # appended last


def test_loop_config_mirror_matches_the_header(tmp_path):
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "me_hip.h"\n'
                   'int main() { std::printf("%zu %zu\\n", sizeof(me_vo_loop_config), '
                   'offsetof(me_vo_loop_config, klt_fb_max)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    size, off = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(_lib.VOLoopConfigC)
    assert off == _lib.VOLoopConfigC.klt_fb_max.offset


def test_symbol_is_declared_exported_and_bound():
    lib = _lib.load_library()
    assert "me_klt_track_fb" in _lib.EXPORTS and hasattr(lib, "me_klt_track_fb")
    assert lib.me_klt_track_fb.argtypes is not None and len(lib.me_klt_track_fb.argtypes) == 14
    with open(os.path.join(ROOT, "include", "me_hip.h")) as fh:
        assert "int me_klt_track_fb(" in fh.read()


def test_cpp_overload_compiles(tmp_path):
    exe = C.build_cli(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)  # no input file: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr
