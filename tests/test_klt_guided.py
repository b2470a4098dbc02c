"""Guided KLT (include/me_hip.h A12f), the parts that need no GPU: the numpy
restatement of the whole tracker (uasl_motion_estimation_amd/klt_ref.py)
anchored to oracle/klt.cpp, what the guess buys on fast motion, the rule for
unusable guesses, the pixel prediction pipeline.predict_uv, the loop switch
PipelineConfig.klt_predict on the oracle backend and the C++ overloads.  The
device side is tests/test_klt_guided_gpu.py.
"""
import os
import subprocess

import numpy as np
import pytest

import klt_fb_cases as F
import klt_guided_cases as G
from uasl_motion_estimation_amd import _lib
from uasl_motion_estimation_amd import klt_ref as KR
from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = G.bits


# ------------------------------------------------------------------ the restatement is the oracle's tracker
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_restatement_without_a_guess_is_the_oracle_on_the_occluded_pairs(oracle, shape):
    w, h, win, lv = shape
    prev, nxt = F.image_pair(w, h)
    # the grid, and features whose window leaves the image or that lie outside it
    pts = np.concatenate([F.grid_points(w, h, win),
                          np.array([[2, 2], [w - 1, h - 1], [-5, 3], [w + 10, 5]], np.float32)])
    want, wst = oracle.klt(prev, nxt, pts, win=win, max_level=lv)
    got, gst = KR.klt_track_ref(prev, nxt, pts, win=win, max_level=lv)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(gst, wst)
    assert 0 < int(wst.sum()) < len(pts)
    # and in the other direction (the backward pass's roles)
    want, wst = oracle.klt(nxt, prev, got, win=win, max_level=lv)
    back, bst = KR.klt_track_ref(nxt, prev, got, win=win, max_level=lv)
    assert np.array_equal(bits(back), bits(want)) and np.array_equal(bst, wst)


@pytest.mark.parametrize("name", list(G.CASES))
def test_restatement_without_a_guess_is_the_oracle_on_the_fast_pairs(oracle, name):
    c = G.case(name)
    want, wst = oracle.klt(c.prev, c.next, c.pts, **c.kw)
    got, gst = G.ref(name, "plain")
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(gst, wst)


def test_restatement_fb_without_a_guess_is_klt_fb_host(oracle):
    w, h, win, lv = F.SHAPES[0]
    prev, nxt = F.image_pair(w, h)
    q, st, err = KR.klt_guided_fb_ref(prev, nxt, F.grid_points(w, h, win), None, 0.5, win=win, max_level=lv)
    ref = F.oracle_fb(w, h, win, lv, 0.5)
    assert np.array_equal(bits(q), bits(ref[0])) and np.array_equal(st, ref[1])
    assert np.array_equal(bits(err), bits(ref[2]))


def test_restatement_no_features():
    c = G.case("C")
    uv, st = KR.klt_track_ref(c.prev, c.next, c.pts[:0], c.guess[:0], **c.kw)
    assert uv.shape == (0, 2) and uv.dtype == np.float32 and st.shape == (0,)
    q, st, err = KR.klt_guided_fb_ref(c.prev, c.next, c.pts[:0], c.guess[:0], 1.0, **c.kw)
    assert q.shape == (0, 2) and st.shape == (0,) and err.shape == (0,)
    with pytest.raises(ValueError):
        KR.klt_guided_fb_ref(c.prev, c.next, c.pts, c.guess, 0.0, **c.kw)
    with pytest.raises(ValueError):
        KR.klt_track_ref(c.prev, c.next, c.pts, c.guess[:3], **c.kw)


# ------------------------------------------------------------------ what the guess buys
@pytest.mark.parametrize("name", list(G.CASES))
def test_guess_recovers_motion_the_plain_tracker_loses(name):
    c = G.case(name)
    assert len(c.pts) == 64
    lo, hi = c.truth.min(0), c.truth.max(0)
    assert lo[0] >= 0 and lo[1] >= 0 and hi[0] < c.w and hi[1] < c.h  # every true destination inside the image
    assert np.abs(c.guess.astype(np.float64) - c.truth).max() <= 2.0 + 1e-4
    unguided = c.correct(*G.ref(name, "plain"))
    guided = c.correct(*G.ref(name, "guided"))
    q, st, err = G.ref(name, "guided_fb", 1.0)
    print(name, "correct: unguided", unguided, "guided", guided, "guided fb accepts", int(st.sum()))
    assert guided == 64
    assert int(st.sum()) == 64 and np.all(err <= 1.0)
    assert np.array_equal(bits(q), bits(G.ref(name, "guided")[0]))  # the forward pass is the guided call's
    assert unguided <= (32 if name == "C" else 4)  # the input stays hard for the plain tracker


@pytest.mark.parametrize("name", list(G.CASES))
def test_unusable_guesses_fall_back_to_the_plain_tracker(oracle, name):
    c = G.case(name)
    g, ignored = G.mixed_guess(c)
    assert ignored.sum() == 13 and np.array_equal(g[34], c.pts[34])
    use = KR.usable(g, c.w, c.h)
    assert not use[ignored][:11].any() and use[ignored][11:].all() and use[~ignored].all()
    uv, st = KR.klt_track_ref(c.prev, c.next, c.pts, g, **c.kw)
    want, wst = oracle.klt(c.prev, c.next, c.pts, **c.kw)
    assert np.array_equal(bits(uv)[ignored], bits(want)[ignored]) and np.array_equal(st[ignored], wst[ignored])
    guv, gst = G.ref(name, "guided")
    assert np.array_equal(bits(uv)[~ignored], bits(guv)[~ignored]) and np.array_equal(st[~ignored], gst[~ignored])
    # the check: those features are me_klt_track_fb's, the others the guided check's
    q, fst, err = KR.klt_guided_fb_ref(c.prev, c.next, c.pts, g, 1.0, **c.kw)
    pq, pst, perr = G.ref(name, "fb", 1.0)
    gq, gfst, gerr = G.ref(name, "guided_fb", 1.0)
    for a, p, gd in ((bits(q), bits(pq), bits(gq)), (fst, pst, gfst), (bits(err), bits(perr), bits(gerr))):
        assert np.array_equal(a[ignored], p[ignored]) and np.array_equal(a[~ignored], gd[~ignored])


def test_all_unusable_guess_is_the_plain_check(oracle):
    c = G.case("A")
    g = np.full_like(c.guess, np.nan)
    for got, want in zip(KR.klt_guided_fb_ref(c.prev, c.next, c.pts, g, 1.0, **c.kw), G.ref("A", "fb", 1.0)):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    for got, want in zip(KR.klt_guided_fb_ref(c.prev, c.next, c.pts, c.pts, 1.0, **c.kw), G.ref("A", "fb", 1.0)):
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


# ------------------------------------------------------------------ the prediction
def test_predict_uv_against_the_synthetic_projection():
    rng = np.random.default_rng(5)
    K = S.intrinsics(640, 480)
    pose = np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.2, 3)])
    X = np.concatenate([rng.uniform(-3, 3, (300, 2)), rng.uniform(2, 20, (300, 1))], 1)
    X[::25, 2] = -X[::25, 2]  # behind the camera
    R = PL.aa_to_R(pose[3:])
    got = PL.predict_uv(X, pose, K[0, 0], K[0, 2], K[1, 2])
    assert got.shape == (300, 2) and got.dtype == np.float32
    Z = X @ R[2] + pose[2]
    assert (Z <= 0).sum() >= 10 and (Z > 0).sum() >= 250
    assert np.all(np.isnan(got[Z <= 0])) and np.all(np.isfinite(got[Z > 0]))
    want = np.array([S.project(K, 0.5, R, pose[:3], x)[0][:2] for x in X])
    d = np.abs(got.astype(np.float64) - want)[Z > 0]
    print("predict_uv vs synthetic.project: max |d| = %.3g px" % d.max())
    assert np.abs(want[Z > 0]).max() < 8192  # (float32 rounding below 2.5e-4 px at these sizes)
    assert d.max() <= 1e-3
    assert PL.predict_uv(np.zeros((0, 3)), pose, 1.0, 0.0, 0.0).shape == (0, 2)


# ------------------------------------------------------------------ the loop switch
def test_switch_is_off_by_default():
    assert PL.PipelineConfig.from_config(1).klt_predict is False and PL.Backend.klt_predict is False
    off = F.oracle_loop()
    assert off.cfg.klt_predict is False and off.be.klt_predict is False


def _spy_loop(**cfg_kw):
    """The oracle-backend loop with a backend that records every klt_submit's
    guess and, at step 4 of the same keyframe (after the pops and step 3's
    prediction), predict_uv of the loop's state."""
    from pipeline_oracle import OracleBackend

    class Spy(OracleBackend):
        vo = None

        def __init__(self):
            self.seen, self.at_step3, self.n_pts = [], [], []

        def klt_submit(self, prev, cur, pts, guess=None):
            self.seen.append(None if guess is None else np.array(guess, np.float32))
            self.n_pts.append(len(pts))
            return OracleBackend.klt_submit(self, prev, cur, pts, guess=guess)

        def klt_match_new(self, h, imgs, lo, nd, dvalid, t, *a):
            vo = self.vo
            act = np.flatnonzero(vo.active)
            self.at_step3.append(PL.predict_uv(vo.X[act], vo.poses[t], vo.f, vo.cx, vo.cy))
            return OracleBackend.klt_match_new(self, h, imgs, lo, nd, dvalid, t, *a)

    _, K, p0, v, _ = F.sequence()
    be = Spy()
    vo = PL.WindowedStereoVO(F.loop_config(**cfg_kw), be, K, p0, v, log_events=True)
    be.vo = vo
    return F.run_loop(vo)


def test_loop_guess_is_predict_uv_of_the_state_at_step_3(oracle):
    vo = _spy_loop(klt_predict=True)
    be = vo.be
    assert be.klt_predict is True
    assert len(be.seen) == len(be.at_step3) == F.N_KEYFRAMES - 1
    assert any(ev[0] == "pop" for ev in vo.events)  # pops did run between steps 1 and 3
    for g, want, n in zip(be.seen, be.at_step3, be.n_pts):
        assert g is not None and g.shape == (n, 2) and g.dtype == np.float32 and n > 0
        assert np.array_equal(bits(g), bits(want))  # (bit patterns: NaN rows compare too)
        assert np.isfinite(g).all(1).sum() >= n // 2
    assert len(vo.results) == F.N_KEYFRAMES


def test_loop_switch_off_passes_no_guess(oracle):
    vo = _spy_loop()
    assert all(g is None for g in vo.be.seen) and len(vo.be.seen) == F.N_KEYFRAMES - 1
    assert vo.events == F.oracle_loop().events


def test_loop_with_the_guess_ignored_is_the_switch_off_loop(oracle, monkeypatch):
    from pipeline_oracle import OracleBackend

    real, calls = KR.klt_track_ref, []

    def no_guess(prev, nxt, pts, guess=None, **kw):
        calls.append(guess is not None)
        return real(prev, nxt, pts, None, **kw)

    monkeypatch.setattr(KR, "klt_track_ref", no_guess)
    _, K, p0, v, _ = F.sequence()
    on = F.run_loop(PL.WindowedStereoVO(F.loop_config(klt_predict=True), OracleBackend(), K, p0, v, log_events=True))
    off = F.oracle_loop()
    assert calls == [True] * (F.N_KEYFRAMES - 1)
    assert on.events == off.events and np.array_equal(on.ids, off.ids) and np.array_equal(on.X, off.X)
    assert sorted(on.poses) == sorted(off.poses) and all(np.array_equal(on.poses[t], off.poses[t]) for t in on.poses)


@pytest.mark.parametrize("fb_max", [0.0, 0.5])
def test_loop_switch_on_completes(oracle, fb_max):
    on = G.oracle_loop(klt_predict=True, klt_fb_max=fb_max)
    assert on.be.klt_predict is True and on.be.klt_fb_max == fb_max
    n_on = [r.n_tracked for r in on.results]
    print("n_tracked with the guess, klt_fb_max", fb_max, ":", n_on, "without:",
          [r.n_tracked for r in F.oracle_loop(klt_fb_max=fb_max).results])
    assert len(n_on) == F.N_KEYFRAMES and all(n > 0 for n in n_on[1:])
    assert all(np.all(np.isfinite(p)) for p in on.poses.values())


# ------------------------------------------------------------------ the ABI and the mirrors
def test_symbols_are_declared_exported_and_bound():
    lib = _lib.load_library()
    with open(os.path.join(ROOT, "include", "me_hip.h")) as fh:
        hdr = fh.read()
    for name, nargs in (("me_klt_track_guided", 13), ("me_klt_track_guided_fb", 15), ("me_vo_loop_set_klt_predict", 2)):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
        assert "int %s(" % name in hdr
    assert lib.me_abi_version() == 4  # setters and entry points only: the ABI version stays


def test_setter_rejects_a_null_loop():
    assert _lib.load_library().me_vo_loop_set_klt_predict(None, 1) == -1


def test_cpp_overloads_compile(tmp_path):
    exe = G.build_cli(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)  # no input file: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr
