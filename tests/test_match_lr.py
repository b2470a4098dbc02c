"""Left-right consistency check of the epipolar MI matcher (include/me_hip.h
A2b), the parts that need no GPU: the numpy restatement pipeline.match_lr_host
around the oracle MI (oracle/mi.cpp), the loop switch
PipelineConfig.match_lr_max on the oracle backend, the configuration checks,
the declarations and the C++ setter.  The device side is
tests/test_match_lr_gpu.py.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import klt_fb_cases as KC
import match_lr_cases as C
from uasl_motion_estimation_amd import _lib
from uasl_motion_estimation_amd import pipeline as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d-p%d" % s)
def test_host_restatement_on_the_occluded_striped_pair(oracle, shape):
    ref = C.oracle_lr(*shape)
    xr, ok, err, ok_f, ok_b = ref
    C.assert_classes_populated(ref)
    assert C.classes(*ref) == C.COUNTS[shape]  # the oracle's own counts on this input
    assert len(xr) == 80 and np.all(ok <= ok_f) and np.all(ok_b <= ok_f)
    both = ok_f & ok_b
    assert np.array_equal(np.isinf(err), ~both) and np.all(err[~both] > 0)
    assert np.all(err[both] >= 0) and np.array_equal(ok, both & (err.astype(np.float64) <= C.LR_MAX))
    assert not np.any(np.abs(err[both] - 1.0) < 1e-6)  # (no distance whose float rounding could cross the bound)
    # the bound only gates: same distances, a superset under a wider bound, everything both passes matched under inf
    wide = C.oracle_lr(*shape, lr_max=2.0)
    assert np.array_equal(bits(wide[2]), bits(err)) and np.all(ok <= wide[1])
    inf = C.oracle_lr(*shape, lr_max=math.inf)
    assert np.array_equal(inf[1], both) and np.array_equal(bits(inf[0]), bits(xr))


@pytest.mark.parametrize("shape", C.SHAPES[:2], ids=lambda s: "%dx%d" % s[:2])
def test_forward_half_is_match_host(oracle, shape):
    for kw in (dict(), dict(d_max=14), dict(lo=2, nd=31, unique=True)):
        xr, ok, err, ok_f, ok_b = C.oracle_lr(*shape, **kw)
        pxr, pok = C.oracle_plain(*shape, **kw)
        assert np.array_equal(bits(xr), bits(pxr)) and np.array_equal(ok_f, pok), kw


def test_a_small_d_max_cuts_both_passes(oracle):
    ref = C.oracle_lr(160, 120, 11, d_max=14)
    assert C.classes(*ref)[1:3] == (59, 10)
    C.assert_classes_populated(C.oracle_lr(160, 120, 11))


@pytest.mark.parametrize("shape,accepted", [(C.SHAPES[0], 43), (C.SHAPES[1], 31)])
def test_uniqueness_leaves_the_check_nothing_to_reject(oracle, shape, accepted):
    ref = C.oracle_lr(*shape, lo=2, nd=31, unique=True)
    assert C.classes(*ref) == (accepted, accepted, 0, 0)


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan])
def test_host_restatement_rejects_a_bound_that_is_not_positive(bad):
    with pytest.raises(ValueError):
        PL.match_lr_host(None, None, np.zeros((1, 2), np.float32), np.zeros(1, np.int64), 13, None, False, 128, bad)


def test_host_restatement_without_features():
    out = PL.match_lr_host(None, None, np.zeros((0, 2), np.float32), np.zeros(0, np.int64), 13, None, False, 128, 1.0)
    assert len(out) == 5 and all(len(a) == 0 for a in out)


# ------------------------------------------------------------------ the loop switch
def test_loop_switch_off_is_the_default_loop(oracle):
    a, b = KC.oracle_loop(), KC.oracle_loop(match_lr_max=0.0)
    assert PL.PipelineConfig.from_config(1).match_lr_max == 0.0 and PL.Backend.match_lr_max == 0.0
    assert a.events == b.events and np.array_equal(a.ids, b.ids) and np.array_equal(a.X, b.X)
    assert sorted(a.poses) == sorted(b.poses) and all(np.array_equal(a.poses[t], b.poses[t]) for t in a.poses)


def test_loop_switch_on_drops_matches_that_do_not_return(oracle):
    off, on = KC.oracle_loop(), KC.oracle_loop(match_lr_max=1.0)
    assert on.be.match_lr_max == 1.0
    n_off, n_on = [r.n_tracked for r in off.results], [r.n_tracked for r in on.results]
    print("n_tracked off", n_off, "on", n_on)
    assert len(n_on) == len(n_off) == KC.N_KEYFRAMES
    assert 0 < n_on[1] < n_off[1], (n_on, n_off)
    assert all(np.all(np.isfinite(p)) for p in on.poses.values())


# ------------------------------------------------------------------ configuration
@pytest.mark.parametrize("bad", [-1, -1e-9, math.nan])
def test_pipeline_config_rejects_a_negative_or_nan_bound(bad):
    with pytest.raises(ValueError):
        PL.PipelineConfig(640, 480, 200, 4, match_lr_max=bad)
    with pytest.raises(ValueError):
        PL.PipelineConfig.from_config(1, match_lr_max=bad)


def test_pipeline_config_field_follows_klt_fb_max():
    import dataclasses

    names = [f.name for f in dataclasses.fields(PL.PipelineConfig)]
    assert names.index("match_lr_max") == names.index("klt_fb_max") + 1
    assert PL.PipelineConfig(640, 480, 200, 4).match_lr_max == 0.0


def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load_library()
    with open(os.path.join(ROOT, "include", "me_hip.h")) as fh:
        header = fh.read()
    for name, nargs in (("me_mi_epipolar_match_lr", 21), ("me_mi_epipolar_match_lr_count", 20),
                        ("me_vo_loop_set_match_lr", 2)):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
        assert "int %s(" % name in header, name
    assert "A2b" in header


def test_native_loop_config_is_unchanged():
    assert _lib.VOLoopConfigC._fields_[-1][0] == "klt_fb_max"  # the switch is a setter, not a field
    assert not any("match_lr" in f[0] for f in _lib.VOLoopConfigC._fields_)
    assert _lib.load_library().me_abi_version() == 4


def test_cpp_setter_compiles(tmp_path):
    """A translation unit that calls WindowedStereoVO::setMatchLrMax, with the flags of tests/cpp/Makefile."""
    src = tmp_path / "set_lr.cpp"
    src.write_text('#include "MotionEstimationAMD/motion_estimation_amd.hpp"\n'
                   "void switch_on(me::WindowedStereoVO& vo, double lr_max) { vo.setMatchLrMax(lr_max); }\n")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                    "-c", str(src), "-o", str(tmp_path / "set_lr.o")], check=True)
