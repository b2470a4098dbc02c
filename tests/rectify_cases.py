"""Inputs of the rectification tests (TEST INFRASTRUCTURE, shared by
test_rectify.py and test_rectify_gpu.py): camera models, Q5 maps that reach
every tap case of the remap, images, and the raw sequences of the loop tests."""
import functools
import math

import numpy as np

from uasl_motion_estimation_amd.rectify import SENTINEL, CameraModel, RectifiedModel, StereoRectifier

PAD = (8, 5)      # columns, rows added on every side of a frame by the padded-crop model
PAD_VALUE = 77
STRONG = (-0.3, 0.1, 1e-3, -5e-4, 0.01)   # k1, k2, p1, p2, k3
RECT_SIZES = [(1, 1), (3, 2), (5, 7), (97, 61), (200, 130)]  # (width, height)


def rot(axis, deg):
    """Row-major rotation by `deg` degrees about x (0), y (1) or z (2)."""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return tuple(R.ravel())


def rect_model(w, h):
    return RectifiedModel(w, h, 0.9 * max(w, 2), 0.9 * max(w, 2), w / 2.0, h / 2.0)


def same_camera(rect, **kw):
    """A raw camera with the rectified model's size and pinhole parameters."""
    return CameraModel(rect.width, rect.height, rect.fx, rect.fy, rect.cx, rect.cy, **kw)


def padded_camera(rect, pad=PAD):
    """The camera of a frame padded by `pad` on every side: the rectified image is the crop."""
    return CameraModel(rect.width + 2 * pad[0], rect.height + 2 * pad[1], rect.fx, rect.fy, rect.cx + pad[0],
                       rect.cy + pad[1])


def models(w, h):
    """name -> (camera, rectified) for a rectified size: the cases of the map tests."""
    r = rect_model(w, h)
    out = {
        "identity": (same_camera(r), r),
        "padcrop": (padded_camera(r), r),
        # a raw camera of another size and focal length (80 x 64 against 97 x 61)
        "other": (CameraModel(80, 64, 75.0, 74.0, 41.5, 30.25), r),
        "rot_x": (same_camera(r, R=rot(0, 2.0)), r),
        "rot_y": (same_camera(r, R=rot(1, 2.0)), r),
        "rot_z": (same_camera(r, R=rot(2, 2.0)), r),
        "strong": (same_camera(r, dist=STRONG, R=rot(1, 1.0)), r),
        # W <= 0 on a part of the image: rays that point behind the raw camera
        "behind": (same_camera(r, R=rot(1, 100.0)), r),
        # far pixels land beyond 2^24
        "overflow": (same_camera(r, dist=(1e9, 0.0, 0.0, 0.0, 0.0)), r),
    }
    return out


MODEL_NAMES = ["identity", "padcrop", "other", "rot_x", "rot_y", "rot_z", "strong", "behind", "overflow"]


def realistic(w, h):
    """The model of the driver's timings: k1 -0.3, k2 0.1, small p1 / p2, rotations of a degree or two."""
    r = RectifiedModel(w, h, 0.9 * w, 0.9 * w, w / 2.0, h / 2.0)
    R = np.array(rot(0, 1.0)).reshape(3, 3) @ np.array(rot(1, -1.5)).reshape(3, 3) @ np.array(rot(2, 0.7)).reshape(3, 3)
    cam = CameraModel(w, h, 0.92 * w, 0.91 * w, w / 2.0 + 3.5, h / 2.0 - 2.25, (-0.3, 0.1, 5e-4, -3e-4, 0.0),
                      tuple(R.ravel()))
    return cam, r


# ------------------------------------------------------------------ images
@functools.lru_cache(maxsize=None)
def noise(w, h, seed=3):
    a = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    a = (((x + y) & 1) * 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def padded_buffer(img, extra=3, fill=PAD_VALUE):
    """(view, buffer): the image as a view of a buffer whose rows are `extra` bytes longer, padding = fill."""
    h, w = img.shape
    buf = np.full((h, w + extra), fill, np.uint8)
    buf[:, :w] = img
    return buf[:, :w], buf


# ------------------------------------------------------------------ maps
def as_map(iu, iv):
    m = np.empty(np.broadcast(iu, iv).shape + (2,), np.int32)
    m[..., 0], m[..., 1] = iu, iv
    return m


def grid_q5(dw, dh):
    v, u = np.mgrid[0:dh, 0:dw]
    return 32 * u.astype(np.int64), 32 * v.astype(np.int64)


def identity_map(dw, dh):
    return as_map(*grid_q5(dw, dh))


def shift_map(dw, dh, dx, dy, q=0):
    """dst(x, y) <- src(x + dx + q / 32, y + dy): an integer shift, plus q / 32 pixel in x."""
    iu, iv = grid_q5(dw, dh)
    return as_map(iu + 32 * dx + q, iv + 32 * dy)


def fraction_map(bx, by):
    """32 x 32: pixel (i, j) (column i, row j) reads the 2 x 2 block at (bx, by) with fractions (i, j)."""
    j, i = np.mgrid[0:32, 0:32]
    return as_map(32 * bx + i, 32 * by + j)


def random_map(dw, dh, sw, sh, seed, outside=0.0):
    """Uniformly random entries with every tap inside the source; a share
    `outside` of them instead far outside, half of those the sentinel."""
    rng = np.random.default_rng(seed)
    iu = rng.integers(0, max(32 * (sw - 1), 1), (dh, dw))
    iv = rng.integers(0, max(32 * (sh - 1), 1), (dh, dw))
    if outside > 0.0:
        k = rng.random((dh, dw))
        far = rng.integers(-2 ** 30, 2 ** 30, (2, dh, dw))
        far = np.where(np.abs(far) < 32 * (sw + sh + 4), far + 2 ** 20, far)
        iu = np.where(k < outside, far[0], iu)
        iv = np.where(k < outside, far[1], iv)
        iu = np.where(k < outside / 2, SENTINEL, iu)
        iv = np.where(k < outside / 2, SENTINEL, iv)
    return as_map(iu, iv)


def outside_map(dw, dh, sw, sh):
    """Every entry at least two pixels off the source, on all sides in turn."""
    v, u = np.mgrid[0:dh, 0:dw]
    side = (u + v) % 4
    iu = np.choose(side, [-64 - u, 32 * (sw + 1) + u, 32 * (u % sw), 32 * (u % sw)])
    iv = np.choose(side, [32 * (v % sh), 32 * (v % sh), -64 - v, 32 * (sh + 1) + v])
    return as_map(iu, iv)


def edge_map(dw, dh, sw, sh):
    """Taps that straddle each of the four sides (sx = -1, sx = sw - 1, sy = -1, sy = sh - 1), and the
    corners, with fractions that run through 0 .. 31."""
    v, u = np.mgrid[0:dh, 0:dw]
    side = (u // 2 + v) % 4
    fx, fy = (3 * u + v) % 32, (5 * v + u) % 32
    xin, yin = 32 * (u % sw) + fx, 32 * (v % sh) + fy
    iu = np.choose(side, [-32 + fx, 32 * (sw - 1) + fx, xin, np.where(u % 2 == 0, -32 + fx, 32 * (sw - 1) + fx)])
    iv = np.choose(side, [yin, yin, np.where(u % 2 == 0, -32 + fy, 32 * (sh - 1) + fy),
                          np.where(v % 2 == 0, -32 + fy, 32 * (sh - 1) + fy)])
    return as_map(iu, iv)


def transpose_map(dw, dh):
    """dst(x, y) <- src(y, x)."""
    iu, iv = grid_q5(dw, dh)
    return as_map(iv, iu)


def decimation_map(dw, dh, k=4):
    iu, iv = grid_q5(dw, dh)
    return as_map(k * iu + 16, k * iv + 16)


def user_maps(dw, dh, sw, sh):
    """name -> map of dw x dh over a source of sw x sh: the hand-made maps of the remap tests."""
    return {
        "identity": identity_map(dw, dh),
        "shift_left": shift_map(dw, dh, 3, 0),
        "shift_right": shift_map(dw, dh, -3, 0),
        "shift_up": shift_map(dw, dh, 0, 2),
        "shift_down": shift_map(dw, dh, 0, -2),
        "random": random_map(dw, dh, sw, sh, 11),
        "random_tenth_out": random_map(dw, dh, sw, sh, 12, 0.1),
        "outside": outside_map(dw, dh, sw, sh),
        "edges": edge_map(dw, dh, sw, sh),
        "transpose": transpose_map(dw, dh),
        "decimate4": decimation_map(dw, dh),
    }


def tile_paths_ref(m, sw, sh, tw, th, cap):
    """The path of every tile of me_remap_q5 (0 staged, 1 global), from the
    rule me_hip.h states beside me_remap_tile_dims: (tiles_y, tiles_x) uint8."""
    dh, dw = m.shape[:2]
    sx, sy = m[..., 0].astype(np.int64) >> 5, m[..., 1].astype(np.int64) >> 5
    touch = (sx >= -1) & (sx <= sw - 1) & (sy >= -1) & (sy <= sh - 1)
    out = np.zeros(((dh + th - 1) // th, (dw + tw - 1) // tw), np.uint8)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            sl = (slice(ty * th, (ty + 1) * th), slice(tx * tw, (tx + 1) * tw))
            t = touch[sl]
            if not t.any():
                continue
            xs, ys = sx[sl][t], sy[sl][t]
            x0, x1, y0, y1 = int(xs.min()), int(xs.max()) + 1, int(ys.min()), int(ys.max()) + 1
            words, rows = (x1 >> 2) - (x0 >> 2) + 1, y1 - y0 + 1
            out[ty, tx] = rows * ((words + 1) | 1) > cap
    return out


def box_map(dw, dh, x0, y0, x1, y1):
    """A map whose first tile's taps span exactly columns x0 .. x1 and rows
    y0 .. y1 of the source: the pixels of the first row step through the
    columns, those of the first column through the rows, entry (0, 0) at
    (x0, y0), and the last of each at x1 - 1 / y1 - 1 (a tap pair ends one
    further); every other entry repeats (x0, y0)."""
    iu = np.full((dh, dw), 32 * x0, np.int64)
    iv = np.full((dh, dw), 32 * y0, np.int64)
    iu[0, :min(dw, 8)] = 32 * np.linspace(x0, x1 - 1, min(dw, 8)).astype(np.int64) + 7
    iv[:min(dh, 8), 0] = 32 * np.linspace(y0, y1 - 1, min(dh, 8)).astype(np.int64) + 9
    return as_map(iu, iv)


# ------------------------------------------------------------------ the loops
def padded_rectifier(cfg_w, cfg_h, K):
    """The rectifier of frames padded by PAD with PAD_VALUE: it crops them back."""
    r = RectifiedModel.from_K(cfg_w, cfg_h, K)
    cam = padded_camera(r)
    return StereoRectifier(cam, cam, r, border=0)


def pad_frame(img):
    return np.pad(np.asarray(img), ((PAD[1], PAD[1]), (PAD[0], PAD[0])), constant_values=PAD_VALUE)


@functools.lru_cache(maxsize=None)
def padded_sequence():
    import klt_fb_cases as KC

    fr = KC.sequence()[0]
    return [(pad_frame(fr[t].left), pad_frame(fr[t].right)) for t in range(KC.N_KEYFRAMES)]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def same_loop(a, b):
    """Two loops took the same decisions and hold the same numbers, bit for bit: events, track table, poses, results."""
    assert a.events == b.events
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.active, b.active)
    assert np.array_equal(_bits(a.X), _bits(b.X))
    pa, pb = a.poses, b.poses
    assert sorted(pa) == sorted(pb)
    for t in pa:
        assert np.array_equal(_bits(pa[t]), _bits(pb[t])), t
    ra_, rb_ = a.results, b.results
    assert len(ra_) == len(rb_)
    for ra, rb in zip(ra_, rb_):
        assert (ra.t, ra.n_tracked, ra.n_new, ra.n_active, ra.n_window_pts, ra.n_window_obs, ra.scale_stop,
                ra.scale_iters, ra.ba_iters) == \
            (rb.t, rb.n_tracked, rb.n_new, rb.n_active, rb.n_window_pts, rb.n_window_obs, rb.scale_stop,
             rb.scale_iters, rb.ba_iters), (ra, rb)
        assert np.array_equal(_bits([ra.scale, ra.ba_cost]), _bits([rb.scale, rb.ba_cost])), (ra, rb)
        assert np.array_equal(_bits(ra.pose), _bits(rb.pose)), (ra, rb)


def run_raw(vo, frames):
    for t, (L, R) in enumerate(frames):
        vo.process(t, L, R)
    vo.finish()
    return vo


# Two cameras of different sizes in front of the config-1 sequence, k1 of
# opposite signs: the left camera is smaller than the rectified image and has
# a shorter focal length, the right one larger with a longer one.
def two_camera_rig(cfg_w, cfg_h, K):
    r = RectifiedModel.from_K(cfg_w, cfg_h, K)
    left = CameraModel(600, 452, 0.93 * r.fx, 0.93 * r.fy, 300.5, 225.75, (0.02, 0.0, 1e-4, -1e-4, 0.0), rot(0, 0.2))
    right = CameraModel(704, 520, 1.08 * r.fx, 1.08 * r.fy, 351.25, 260.5, (-0.02, 0.0, -1e-4, 1e-4, 0.0), rot(1, -0.2))
    return StereoRectifier(left, right, r, border=0)


def inverse_warp(img, cam, rect):
    """A raw image for `cam` made from a rectified one (test input only, plain float arithmetic): raw pixel
    (x, y) is undistorted by fixed-point iteration, rotated into the rectified frame and takes the rectified
    image's bilinear value there, 0 outside."""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    R = np.array(cam.R).reshape(3, 3)
    k1, k2, p1, p2, k3 = cam.dist
    y, x = np.mgrid[0:cam.height, 0:cam.width].astype(np.float64)
    xd, yd = (x - cam.cx) / cam.fx, (y - cam.cy) / cam.fy
    a, b = xd.copy(), yd.copy()
    for _ in range(8):
        r2 = a * a + b * b
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        a = (xd - (2.0 * p1 * a * b + p2 * (r2 + 2.0 * a * a))) / rad
        b = (yd - (p1 * (r2 + 2.0 * b * b) + 2.0 * p2 * a * b)) / rad
    ray = np.stack([a, b, np.ones_like(a)], -1) @ R.T
    u = rect.fx * ray[..., 0] / ray[..., 2] + rect.cx
    v = rect.fy * ray[..., 1] / ray[..., 2] + rect.cy
    ok = (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    u0 = np.clip(np.floor(u).astype(np.int64), 0, w - 2)
    v0 = np.clip(np.floor(v).astype(np.int64), 0, h - 2)
    fu, fv = np.clip(u - u0, 0.0, 1.0), np.clip(v - v0, 0.0, 1.0)
    val = ((1 - fv) * ((1 - fu) * img[v0, u0] + fu * img[v0, u0 + 1])
           + fv * ((1 - fu) * img[v0 + 1, u0] + fu * img[v0 + 1, u0 + 1]))
    return np.where(ok, np.rint(val), 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rig_sequence():
    """(rectifier, raw frames) of the two-camera rig over the config-1 sequence."""
    import klt_fb_cases as KC

    fr, K = KC.sequence()[:2]
    cfg = KC.loop_config()
    rig = two_camera_rig(cfg.width, cfg.height, K)
    frames = [(inverse_warp(fr[t].left, rig.left, rig.out), inverse_warp(fr[t].right, rig.right, rig.out))
              for t in range(KC.N_KEYFRAMES)]
    return rig, frames
