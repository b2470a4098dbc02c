"""Inputs of the left-right stereo check tests (TEST INFRASTRUCTURE, shared by
test_match_lr.py and test_match_lr_gpu.py): stereo pairs with an occluded band
and a striped region, on which the check has something to reject, and its
oracle restatement (pipeline.match_lr_host around oracle/mi.cpp)."""
import functools

import numpy as np

from klt_fb_cases import _bilinear, texture

# (w, h, patch): the 11 x 11 kernels on two sizes, the generic scorer (patch 7) on the small one
SHAPES = [(160, 120, 11), (96, 64, 11), (96, 64, 7)]
DISPARITY = 9.5
LO, ND, MARGIN, LR_MAX, D_MAX = 4, 13, 24, 1.0, 128
# (forward ok, accepted, far, back lost) of the restatement at LO / ND / unique = 0 / LR_MAX / D_MAX
COUNTS = {(160, 120, 11): (66, 59, 5, 2), (96, 64, 11): (62, 45, 15, 2), (96, 64, 7): (60, 35, 24, 1)}


@functools.lru_cache(maxsize=None)
def image_pair(w, h):
    """L: a crop of the texture.  R: the same content 9.5 px to the left; the
    columns [w // 3, w // 3 + w // 5) of R show a second texture (an occluder:
    left points that land there have no way back), and the rows >= 2 h // 3 of
    both carry period-7 stripes, 9 px apart (repeated structure)."""
    a, b = texture(11, w + 40, h), texture(1011, w + 40, h)
    L = 255.0 * a[32:32 + h, 52:52 + w]
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    R = 255.0 * _bilinear(a, xs + DISPARITY + 52.0, ys + 32.0)
    c0, c1 = w // 3, w // 3 + w // 5
    R[:, c0:c1] = 255.0 * b[32:32 + h, 52:52 + w][:, c0:c1]
    s = 127.0 + 100.0 * np.sin(2.0 * np.pi * np.arange(w + 9, dtype=np.float64) / 7.0)
    r0 = 2 * h // 3
    L[r0:] = 0.25 * L[r0:] + 0.75 * s[None, :w]
    R[r0:] = 0.25 * R[r0:] + 0.75 * s[None, 9:9 + w]
    L, R = np.rint(L).astype(np.uint8), np.rint(R).astype(np.uint8)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


def features(w, h):
    """80 features: a 9 x 8 grid, and 8 more near the right border whose backward candidates run past it."""
    xs, ys = np.meshgrid(np.linspace(24, w - 25, 9), np.linspace(24, h - 25, 8))
    grid = np.stack([xs.ravel(), ys.ravel()], -1) + 0.37
    edge = np.stack([np.full(8, w - 12.63), np.linspace(24, h - 25, 8) + 0.37], -1)
    return np.concatenate([grid, edge]).astype(np.float32)


def backend(patch):
    """The oracle backend scoring patch x patch pairs (pipeline_oracle.OracleBackend scores 11 x 11)."""
    import oracle as O
    from pipeline_oracle import OracleBackend

    class PatchBackend(OracleBackend):
        def mi_scores(self, imgs, xyL, xyR):
            return O.mi_scores(imgs[3], imgs[4], np.ascontiguousarray(xyL, np.int32),
                               np.ascontiguousarray(xyR, np.int32), patch, patch)

    return PatchBackend()


_REF = {}


def oracle_lr(w, h, patch, lo=LO, nd=ND, unique=False, d_max=D_MAX, lr_max=LR_MAX, dvalid=None, uv=None, key=None):
    """(xr, ok, lr_err, ok_f, ok_b) of the restatement on the pair, cached
    (`key` names a per-feature lo, a dvalid or other features)."""
    from uasl_motion_estimation_amd.pipeline import match_lr_host

    k = (w, h, patch, lo if np.isscalar(lo) else None, nd, bool(unique), d_max, float(lr_max), key)
    assert key is not None or (np.isscalar(lo) and dvalid is None and uv is None)
    if k not in _REF:
        L, R = image_pair(w, h)
        be = backend(patch)
        imgs = be.frame_images(0, L, R)
        if uv is None:
            uv = features(w, h)
        lo_a = np.full(len(uv), lo, np.int64) if np.isscalar(lo) else np.asarray(lo, np.int64)
        res = match_lr_host(be, imgs, uv, lo_a, nd, dvalid, unique, d_max, lr_max, patch=patch)
        for a in res:
            a.setflags(write=False)
        _REF[k] = res
    return _REF[k]


def oracle_plain(w, h, patch, lo=LO, nd=ND, unique=False, d_max=D_MAX):
    """match_host on the same input (11 x 11 only: match_host has no patch argument)."""
    from uasl_motion_estimation_amd.pipeline import match_host

    L, R = image_pair(w, h)
    be = backend(patch)
    uv = features(w, h)
    return match_host(be, be.frame_images(0, L, R), uv, np.full(len(uv), lo, np.int64), nd, None, unique, d_max)


def classes(xr, ok, lr_err, ok_f, ok_b):
    """(#forward ok, #accepted, #both passes ok but rejected by distance, #forward ok and no way back)."""
    return int(ok_f.sum()), int(ok.sum()), int((ok_f & ok_b & ~ok).sum()), int((ok_f & ~ok_b).sum())


def assert_classes_populated(ref):
    """An input that stops exercising the gate fails the test instead of hiding."""
    _, acc, far, lost = classes(*ref)
    assert acc >= 8 and far >= 4 and lost >= 1, (acc, far, lost)
