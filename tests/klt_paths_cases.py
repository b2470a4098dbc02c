"""Inputs of the KLT path tests (TEST INFRASTRUCTURE, shared by
test_klt_paths.py and test_klt_paths_gpu.py): image pairs, feature lists and
parameters that drive klt_kernel (csrc/klt.hip) through the arithmetic its
bit-exactness rests on and that the smooth textures of the other KLT tests
never reach.  Each case is named for the path it pins; test_klt_paths.py proves
from the trace of the numpy restatement (klt_ref.klt_track_ref(trace=...)) that
the case reaches it.

  S  saturating contrast: window sums past 2^31 (the FP64 stages of the wave sums)
  W  bilinear fractions whose fourth rounded weight is -1
  E  minimum-eigenvalue / determinant rejects, at level 0 and above
  V  every odd window from 3 to 21, windows touching each border
  P  max_iters 0 / 1 / 2, eps 0 and 10, min_eig 0 and 1e3
  D  pyramids that shrink to one pixel; the smallest staged level
  N  positions that are NaN, infinite, past the int range or on the image's edge
  n  0, 1, 2, 3 and 5 features (the partly filled last workgroup)

Everything is deterministic from fixed seeds; images are at most 160 x 120 and
a case has at most 64 features.
"""
import functools

import numpy as np

import klt_fb_cases as F

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_positions(got, want):
    """Bit patterns where the expected value is a number; NaN by isnan (its payload is not specified)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def assert_same(got, want):
    """(pts_out, status[, fb_err]) of two trackers: no tolerance anywhere."""
    assert len(got) == len(want)
    assert same_positions(got[0], want[0]), np.flatnonzero((bits(got[0]) != bits(want[0])).any(1))
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1])
    if len(want) > 2:
        assert np.array_equal(bits(got[2]), bits(want[2]))  # (fb_err: a distance or +inf, never NaN)


# ------------------------------------------------------------------ images
@functools.lru_cache(maxsize=None)
def _binary_field(seed, w, h):
    """(h + 48, w + 64) image of 2 x 2 blocks, each 0 or 255."""
    rng = np.random.default_rng(seed)
    f = np.kron(rng.integers(0, 2, ((h + 48) // 2, (w + 64) // 2)), np.ones((2, 2), np.int64)) * 255
    return f.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def binary_pair(seed, variant, w=96, h=80):
    """prev: the field cropped at (8, 8).  next: the content moved by (+1, -1) ("shift1"), by (+2, -2)
    ("shift2"), or 255 - prev ("inverted")."""
    f = _binary_field(seed, w, h)
    prev = f[8:8 + h, 8:8 + w].copy()
    if variant == "inverted":
        nxt = 255 - prev
    else:
        s = {"shift1": 1, "shift2": 2}[variant]
        nxt = f[8 + s:8 + s + h, 8 - s:8 - s + w].copy()  # next(x, y) = prev(x - s, y + s)
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


@functools.lru_cache(maxsize=None)
def flat_pair(w=96, h=80):
    a = np.full((h, w), 128, np.uint8)
    a.setflags(write=False)
    return a, a


@functools.lru_cache(maxsize=None)
def half_flat_pair(w=96, h=80):
    """binary_pair(1, "shift1") with the columns x < w // 2 of both images set to 128."""
    prev, nxt = (a.copy() for a in binary_pair(1, "shift1", w, h))
    prev[:, :w // 2] = 128
    nxt[:, :w // 2] = 128
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


@functools.lru_cache(maxsize=None)
def stripes_pair(w=96, h=80):
    """Vertical stripes of period 4 (0, 0, 255, 255); next: the same moved by one column.  No row differs from
    its neighbours: every y derivative is 0."""
    x = np.arange(w + 1)
    row = np.where(x % 4 >= 2, 255, 0).astype(np.uint8)
    prev = np.ascontiguousarray(np.broadcast_to(row[:w], (h, w)))
    nxt = np.ascontiguousarray(np.broadcast_to(row[1:], (h, w)))
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


# ------------------------------------------------------------------ feature lists
def border_points(w, h, win):
    """Six features whose template window touches a border exactly: origin ix0 = 0 (inside), ix0 + win = w - 1
    (the last origin inside), ix0 + win = w (the first outside), and the same in y."""
    half = (win - 1) // 2
    cx, cy = w / 2 + 0.37, h / 2 + 0.37
    xs = [half + 0.37, w - 1 - win + half + 0.37, w - win + half + 0.37]
    ys = [half + 0.37, h - 1 - win + half + 0.37, h - win + half + 0.37]
    return np.array([(x, cy) for x in xs] + [(cx, y) for y in ys], F32)


def grid_and_borders(w, h, win):
    """58 points of the 8 x 8 grid and the six border points."""
    grid = np.delete(F.grid_points(w, h, win), [5, 15, 25, 35, 45, 55], 0)
    return np.concatenate([grid, border_points(w, h, win)]).astype(F32)


W_KS = tuple(range(17, 29))


def weight_points(scale=1):
    """Fractions k 2^-19 at 16 + k 2^-19 (k = 17 on both axes rounds to the weights 16383, 1, 1, -1), k from 17
    to 28 on either axis, times `scale` (a power of two: exact); 41 grid points of the 160 x 120 image around
    them."""
    u = lambda k: 16.0 + k * 2.0 ** -19  # noqa: E731
    sp = [(u(17), u(17))] + [(u(k), u(17)) for k in W_KS[1:]] + [(u(17), u(k)) for k in W_KS[1:]]
    sp = np.array(sp, np.float64) * scale
    assert np.array_equal(sp.astype(F32).astype(np.float64), sp)  # exactly representable
    return np.concatenate([F.grid_points(160, 120, 21)[:41], sp.astype(F32)])


N_BAD_SLOTS = (1, 6, 11, 12, 17, 22, 27, 28, 33, 38, 43, 44, 49, 54)  # every position of a workgroup of four


def bad_points(w, h, win):
    """(pts (64, 2), bad (64,) bool): grid points with, at N_BAD_SLOTS, the positions the contract of
    me_hip.h A12 names; every workgroup of four that holds a bad row also holds valid ones."""
    grid = F.grid_points(w, h, win)
    x, y = grid[27]
    inf, nan = F32(np.inf), F32(np.nan)
    rows = [(nan, y), (x, nan), (nan, nan), (inf, y), (x, -inf), (2.0 ** 31, y), (3e9, 3e9), (1e30, 1e30),
            (-1e30, y), (-0.0, -0.0), (w - 1, h - 1), (np.nextafter(F32(w), inf), y), (-inf, inf),
            (-(2.0 ** 31), -(2.0 ** 31) - 256.0)]
    assert len(rows) == len(N_BAD_SLOTS)
    pts, bad = np.zeros((64, 2), F32), np.zeros(64, bool)
    src = iter(grid)
    for i in range(64):
        if i in N_BAD_SLOTS:
            pts[i] = rows[N_BAD_SLOTS.index(i)]
            bad[i] = True
        else:
            pts[i] = next(src)
    return pts, bad


# ------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, pair, pts, bad=None, **kw):
        self.name, self.kw = name, kw
        self.prev, self.next = pair
        self.h, self.w = self.prev.shape
        self.pts = np.ascontiguousarray(pts, F32)
        self.pts.setflags(write=False)
        self.bad = bad  # case N: the rows the contract gives status 0

    def __repr__(self):
        return self.name


def _cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))  # noqa: E731
    # S
    for seed in (1, 2):
        for variant in ("shift1", "shift2", "inverted"):
            for lv in (0, 1):
                add("S-seed%d-%s-L%d" % (seed, variant, lv), binary_pair(seed, variant), F.grid_points(96, 80, 21),
                    win=21, max_level=lv)
    # W (a 160 x 120 pair of S's kind: its level 2 holds the window at 16 + k 2^-19)
    big = binary_pair(1, "shift1", 160, 120)
    add("W-L0", big, weight_points(), win=21, max_level=0)
    add("W-x4-L2", big, weight_points(4), win=21, max_level=2)
    # E
    add("E-flat", flat_pair(), F.grid_points(96, 80, 11), win=11, max_level=2)
    add("E-halfflat", half_flat_pair(), F.grid_points(96, 80, 11), win=11, max_level=2)
    add("E-stripes", stripes_pair(), F.grid_points(96, 80, 21), win=21, max_level=1)
    # V
    for win in range(3, 22, 2):
        add("V-smooth-win%d" % win, F.image_pair(97, 81), grid_and_borders(97, 81, win), win=win, max_level=2)
        add("V-binary-win%d" % win, binary_pair(1, "shift1"), grid_and_borders(96, 80, win), win=win, max_level=2)
    # P
    base = dict(win=9, max_level=2)
    for it in (0, 1, 2):
        add("P-iters%d" % it, F.image_pair(97, 81), grid_and_borders(97, 81, 9), max_iters=it, **base)
    for eps in (0.0, 10.0):
        add("P-eps%g" % eps, F.image_pair(97, 81), grid_and_borders(97, 81, 9), eps=eps, **base)
    for me in (0.0, 1e3):
        add("P-mineig%g" % me, F.image_pair(97, 81), grid_and_borders(97, 81, 9), min_eig=me, **base)
    # D
    for w, h in ((40, 30), (33, 17)):
        add("D-%dx%d-L7" % (w, h), F.image_pair(w, h), F.grid_points(w, h, 7), win=7, max_level=7)
    for w, h in ((32, 32), (33, 32)):
        add("D-%dx%d-win21" % (w, h), F.image_pair(w, h), F.grid_points(w, h, 21), win=21, max_level=0)
    # N
    for win, lv in ((21, 0), (9, 0), (21, 3), (9, 3)):
        pts, bad = bad_points(97, 81, win)
        add("N-win%d-L%d" % (win, lv), F.image_pair(97, 81), pts, bad=bad, win=win, max_level=lv)
    return {c.name: c for c in out}


CASES = _cases()
NAMES = list(CASES)
FB_NAMES = [n for n in NAMES if n[0] in "SWN"]  # these also go through me_klt_track_fb
FB_MAX = 1.0
SMALL_N = (0, 1, 2, 3, 5)
SMALL_N_CASE = "P-iters2"


def kind(name):
    return name[0]


# ------------------------------------------------------------------ references, computed once
_REF, _REF_FB, _TRACE = {}, {}, {}


def _frozen(res):
    for a in res:
        a.setflags(write=False)
    return res


def oracle_ref(name):
    """oracle/klt.cpp on the case: (pts_out, status)."""
    import oracle as O

    if name not in _REF:
        c = CASES[name]
        _REF[name] = _frozen(O.klt(c.prev, c.next, c.pts, **c.kw))
    return _REF[name]


def oracle_valid_only(name):
    """Case N without its bad rows: what the valid rows must come out as."""
    import oracle as O

    key = (name, "valid")
    if key not in _REF:
        c = CASES[name]
        _REF[key] = _frozen(O.klt(c.prev, c.next, c.pts[~c.bad], **c.kw))
    return _REF[key]


def oracle_fb_ref(name):
    """The two-call restatement of me_klt_track_fb around oracle/klt.cpp (pipeline.klt_fb_host, as
    klt_fb_cases.oracle_fb): (pts_out, status, fb_err)."""
    import oracle as O
    from uasl_motion_estimation_amd.pipeline import klt_fb_host

    if name not in _REF_FB:
        c = CASES[name]
        _REF_FB[name] = _frozen(klt_fb_host(lambda a, b, p: O.klt(a, b, p, **c.kw), c.prev, c.next, c.pts, FB_MAX))
    return _REF_FB[name]


def restatement(name):
    """klt_ref.klt_track_ref on the case with a trace: ((pts_out, status), trace)."""
    from uasl_motion_estimation_amd import klt_ref as KR

    if name not in _TRACE:
        c = CASES[name]
        tr = {}
        _TRACE[name] = (_frozen(KR.klt_track_ref(c.prev, c.next, c.pts, trace=tr, **c.kw)), tr)
    return _TRACE[name]
