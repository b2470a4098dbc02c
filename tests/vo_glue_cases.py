"""Restatements and inputs of the VO loop's device-side glue tests (TEST
INFRASTRUCTURE, shared by test_vo_glue.py and test_vo_glue_gpu.py): numpy
restatements of me_vo_new_cells, me_ba_window_indices and me_vo_ba_chain as
include/me_hip.h defines them, built from the arithmetic pipeline.py states
(new_cells, in_margin, rot_series, move_landmarks), and the named inputs both
files use.  Imports without a GPU."""
import functools
from dataclasses import dataclass, field

import numpy as np

from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd import synthetic as S

MARGIN = PL.MARGIN


# ------------------------------------------------------------------ restatements
def good_mask(uv, status, ok, width, height):
    """me_vo_new_cells' gate: status == 1, ok != 0 and inside the margin, the
    margin compared in float32 as the kernel does (pipeline.in_margin on a
    float32 array compares in float32 too; the two are asserted equal)."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    m = np.float32(MARGIN)
    hi_u, hi_v = np.float32(width) - m, np.float32(height) - m
    with np.errstate(invalid="ignore"):
        inside = (uv[:, 0] >= m) & (uv[:, 0] < hi_u) & (uv[:, 1] >= m) & (uv[:, 1] < hi_v)
        assert np.array_equal(inside, PL.in_margin(uv, width, height))
    return (np.asarray(status).reshape(-1) == 1) & (np.asarray(ok).reshape(-1) != 0) & inside


def cells_host(t, uv, status, ok, width, height, grid, d_min=0):
    """me_vo_new_cells: the gate, then pipeline.new_cells over the good
    features.  Returns (new uv (k, 2) float32, lo (k,) int32 = d_min)."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    good = good_mask(uv, status, ok, width, height)
    out = PL.new_cells(t, uv[good], grid)
    assert out.dtype == np.float32
    return out, np.full(len(out), d_min, np.int32)


def window_indices_host(frame, ids, first_frame, win_ids):
    """me_ba_window_indices: cam_idx = frame - first_frame, pt_idx = the ID's
    index in the ascending win_ids, -1 for an ID the window does not hold."""
    frame, ids = np.asarray(frame, np.int64), np.asarray(ids, np.int64)
    win_ids = np.asarray(win_ids, np.int64)
    cam_idx = (frame - first_frame).astype(np.int32)
    j = np.searchsorted(win_ids, ids)
    hit = j < len(win_ids)
    hit[hit] = win_ids[j[hit]] == ids[hit]
    return cam_idx, np.where(hit, j, -1).astype(np.int32)


@dataclass
class ChainArgs:
    """me_vo_chain_args."""
    pose: np.ndarray
    R: np.ndarray
    vel: np.ndarray = field(default_factory=lambda: np.zeros(6))
    k1: int = 0
    k0: int = 0
    mode: int = 1

    def to_c(self):
        from uasl_motion_estimation_amd._lib import VOChainArgsC

        a = VOChainArgsC()
        a.pose[:] = [float(x) for x in self.pose]
        a.R[:] = [float(x) for x in np.asarray(self.R, np.float64).ravel()]
        a.vel[:] = [float(x) for x in self.vel]
        a.k1, a.k0, a.mode = int(self.k1), int(self.k0), int(self.mode)
        return a


def chain_pose2(prev_cams, prev_ok, cams, cam_src, args):
    """pose(t) of me_vo_ba_chain and the cam(k) it is formed from."""
    cams = np.asarray(cams, np.float64)

    def cam(k):
        s = int(cam_src[k])
        return np.asarray(prev_cams, np.float64)[s] if prev_ok and s >= 0 else cams[k]

    if args.mode == 1:
        c1 = cam(args.k1)
        pose2 = c1 + (c1 - cam(args.k0))
    elif args.mode == 0:
        pose2 = cam(args.k1) + np.asarray(args.vel, np.float64)
    else:
        pose2 = cams[-1].copy()
    return pose2, cam


def chain_host(prev_cams, prev_pts, prev_ok, cams, pts, cam_src, win_ids, prev_ids, new_from, args):
    """me_vo_ba_chain as include/me_hip.h defines it: (cams, pts) after the
    call.  prev_cams / prev_pts / prev_ok are the chained-from solve's result
    and termination != FAILURE; cams / pts the host values the call is given."""
    cams = np.array(cams, np.float64).reshape(-1, 6)
    pts = np.array(pts, np.float64).reshape(-1, 3)
    win_ids, prev_ids = np.asarray(win_ids, np.int64), np.asarray(prev_ids, np.int64)
    nc = len(cams)
    pose2, cam = chain_pose2(prev_cams, prev_ok, cams, cam_src, args)
    out_c = np.stack([cam(k) for k in range(nc - 1)] + [pose2])
    moved = bool(np.any(pose2 != np.asarray(args.pose, np.float64)))
    out_p = pts.copy()
    old = win_ids < new_from
    if prev_ok and old.any() and len(prev_ids):
        j = np.searchsorted(prev_ids, win_ids)
        found = old & (j < len(prev_ids))
        found[found] = prev_ids[j[found]] == win_ids[found]
        out_p[found] = np.asarray(prev_pts, np.float64)[j[found]]
    new = ~old
    if moved and new.any():
        out_p[new] = PL.move_landmarks(pts[new], np.asarray(args.R, np.float64).reshape(3, 3),
                                       np.asarray(args.pose, np.float64), pose2, PL.rot_series(pose2[3:]))
    return out_c, out_p


# ------------------------------------------------------------------ me_vo_new_cells inputs
# (nx, ny, width, height): each grid named for the path of vo_cells_kernel it takes (1024 threads, one
# contiguous chunk of ceil(ncell / 1024) cells each, occupancy in 32-bit words)
GRIDS = {
    "1x1-single-cell": (1, 1, 640, 480),
    "33x31-last-thread-idle-31-bit-tail-word": (33, 31, 640, 480),
    "32x32-chunk-1-exactly": (32, 32, 640, 480),
    "1025x1-chunk-2-most-threads-empty": (1025, 1, 1280, 720),
    "37x28-chunk-2-tail-word": (37, 28, 640, 480),
    "256x256-max-cells-chunk-64": (256, 256, 1280, 720),
}
CELL_N = (0, 700, 2500)  # none; one trip of the 1024-thread feature loop; three trips, the last partial
CELL_T = (0, 7, 100000, 2 ** 31 - 1)  # the last two wrap the hash's 32-bit products


def cell_grid(name, n_feats=0):
    """pipeline's grid tuple (nx, ny, cw, ch, n_feats) and (width, height)."""
    nx, ny, width, height = GRIDS[name]
    return (nx, ny, (width - 2 * MARGIN) / nx, (height - 2 * MARGIN) / ny, n_feats), (width, height)


@functools.lru_cache(maxsize=None)
def cell_features(name, n):
    """n tracked features (uv float32, status, ok) over the grid's image.  The
    first 16 are fixed: the margin's four edge values in u and in v, a NaN
    coordinate, status 2 and 0, ok 0, and three features in one cell; the rest
    are random, about one in twelve outside the margin, about one in ten
    rejected by status or by ok."""
    _, (width, height) = cell_grid(name)
    rng = np.random.default_rng(1000 + n)
    uv = np.stack([rng.uniform(MARGIN - 6.0, width - MARGIN + 6.0, n),
                   rng.uniform(MARGIN - 4.0, height - MARGIN + 4.0, n)], -1).astype(np.float32)
    status = np.where(rng.random(n) < 0.05, 2, 1).astype(np.uint8)
    ok = (rng.random(n) >= 0.05).astype(np.uint8)
    m, one = np.float32(MARGIN), np.float32(1)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))  # noqa: E731
    mu, mv = np.float32(width / 2 + 0.25), np.float32(height / 2 + 0.25)
    hu, hv = np.float32(width) - m, np.float32(height) - m
    fixed = [(m, mv, 1, 1), (below(m), mv, 1, 1), (hu, mv, 1, 1), (below(hu), mv, 1, 1),
             (mu, m, 1, 1), (mu, below(m), 1, 1), (mu, hv, 1, 1), (mu, below(hv), 1, 1),
             (np.float32(np.nan), mv, 1, 1), (mu, np.float32(np.nan), 1, 1),
             (mu + one, mv, 2, 1), (mu + one, mv, 0, 1), (mu + one, mv, 1, 0),
             (m + one, m + one, 1, 1), (m + one, m + one, 1, 1), (m + one + one / 8, m + one + one / 8, 1, 1)]
    for k, (u, v, s, o) in enumerate(fixed[:n]):
        uv[k], status[k], ok[k] = (u, v), s, o
    for a in (uv, status, ok):
        a.setflags(write=False)
    return uv, status, ok


def cell_gate_counts(name, n):
    """Features the gate rejects by one term alone: (status, ok, u, v), and the good ones."""
    uv, status, ok = cell_features(name, n)
    _, (width, height) = cell_grid(name)
    one = np.ones(n, np.uint8)
    all_in = good_mask(uv, one, one, width, height)
    mid = np.broadcast_to(np.float32([width / 2, height / 2]), uv.shape)
    u_in = good_mask(np.stack([uv[:, 0], mid[:, 1]], -1), one, one, width, height)
    v_in = good_mask(np.stack([mid[:, 0], uv[:, 1]], -1), one, one, width, height)
    st, k = status == 1, ok != 0
    return (int((~st & k & all_in).sum()), int((st & ~k & all_in).sum()), int((st & k & ~u_in & v_in).sum()),
            int((st & k & u_in & ~v_in).sum()), int(good_mask(uv, status, ok, width, height).sum()))


def cell_occupancy(name, n):
    """(good, empty): good features and the cells they leave empty."""
    uv, status, ok = cell_features(name, n)
    grid, (width, height) = cell_grid(name)
    good = int(good_mask(uv, status, ok, width, height).sum())
    everything = len(cells_host(0, uv, status, ok, width, height, grid[:4] + (good + grid[0] * grid[1],))[0])
    return good, everything


def cell_n_feats(name, n):
    """n_feats values by regime: {"none": want == 0, "some": 0 < want < empty
    (where two cells are empty), "all": want > empty}."""
    good, empty = cell_occupancy(name, n)
    out = {"none": good, "all": good + empty + 3}
    if empty >= 2:
        out["some"] = good + (empty + 1) // 2
    return out


# ------------------------------------------------------------------ me_ba_window_indices inputs
INDEX_N_OBS = (0, 1, 255, 256, 257, 1000)  # the kernel's 256-thread blocks: below, at, above one; several
INDEX_N_PTS = (0, 1, 2, 300)
FIRST_FRAME = 37


def gapped_ids(rng, n, last=None, first=1000):
    """n ascending IDs with gaps of 1..4 (every ID has a free neighbour below
    it); ending at `last` when given, else starting at `first`."""
    ids = np.cumsum(rng.integers(2, 6, n)).astype(np.int64)
    ids += (last - ids[-1]) if (last is not None and n) else first
    return ids


@functools.lru_cache(maxsize=None)
def index_case(n_obs, n_pts, high=False):
    """(frame, ids, first_frame, win_ids) int32: about half the observation
    IDs are the window's, the rest fall below its first ID, above its last and
    into its gaps.  high: the window's IDs end at 2^31 - 3 and the IDs above
    it reach 2^31 - 1."""
    rng = np.random.default_rng(7 * n_obs + n_pts + (1 if high else 0))
    win = gapped_ids(rng, n_pts, last=2 ** 31 - 3 if high else None)
    lo, hi = (int(win[0]), int(win[-1])) if n_pts else (1000, 1000)
    kind = rng.integers(0, 6, n_obs)
    ids = np.empty(n_obs, np.int64)
    for i, k in enumerate(kind):
        if k < 3 and n_pts:
            ids[i] = win[rng.integers(0, n_pts)]
        elif k == 3 or not n_pts:
            ids[i] = lo - int(rng.integers(1, 50))
        elif k == 4:
            ids[i] = hi + int(rng.integers(1, 3))
        else:
            ids[i] = win[rng.integers(0, n_pts)] - 1  # (gaps are at least 2: never a window ID)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() <= 2 ** 31 - 1)
    frame = FIRST_FRAME + rng.integers(0, 8, n_obs)
    out = (frame.astype(np.int32), ids.astype(np.int32), FIRST_FRAME, win.astype(np.int32))
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ me_vo_ba_chain inputs
SRC_CAMS = 8


@functools.lru_cache(maxsize=None)
def chain_source():
    """The chained-from window: a small BA problem and its tracks' ascending gapped IDs."""
    bp = S.ba_problem(21, 300, SRC_CAMS, 640, 480)
    ids = gapped_ids(np.random.default_rng(5), len(bp.pts)).astype(np.int32)
    ids.setflags(write=False)
    return bp, ids


@dataclass
class ChainCase:
    cams: np.ndarray       # (n_cams, 6) host values
    pts: np.ndarray        # (n_pts, 3) host values
    cam_src: np.ndarray    # (n_cams,) int32, inside the source's cameras or -1
    win_ids: np.ndarray    # (n_pts,) int32 ascending
    new_from: int
    args: ChainArgs
    pose_from_reference: bool = False  # args.pose := the reference's pose(t), so nothing moves

    def classes(self, prev_ids):
        """Landmarks (found in prev_ids, below new_from but absent, new)."""
        ids = self.win_ids.astype(np.int64)
        old = ids < self.new_from
        inp = np.isin(ids, prev_ids)
        return int((old & inp).sum()), int((old & ~inp).sum()), int((~old).sum())


def _host_cams(rng, n):
    c = np.zeros((n, 6))
    c[:, :3] = rng.normal(0.0, 0.3, (n, 3)) + np.arange(n)[:, None] * np.array([0.01, 0.0, -0.5])
    c[:, 3:] = rng.normal(0.0, 0.02, (n, 3))
    return c


def _chain_landmarks(rng, n_pts, prev_ids):
    """win_ids (ascending) and new_from for n_pts landmarks.  From 255 up a
    mix: IDs of the previous window below new_from (found), IDs of its gaps
    below new_from (kept), IDs at or above new_from (new), one of which the
    previous window holds too."""
    prev = prev_ids.astype(np.int64)
    new_from = int(prev[-40])
    if n_pts == 0:
        return np.zeros(0, np.int32), new_from
    if n_pts == 1:
        return prev[3:4].astype(np.int32), new_from
    below = prev[prev < new_from]
    found = rng.choice(below, min(n_pts // 2, 3 * len(below) // 4), replace=False)
    kept = rng.choice(below[1:] - 1, min(max(n_pts // 10, 1), len(below) - 1), replace=False)  # (gaps: no window ID)
    n_new = n_pts - len(found) - len(kept)
    new = np.concatenate([prev[-5:-4], int(prev[-1]) + 1 + 2 * np.arange(n_new - 1)])
    ids = np.sort(np.concatenate([found, kept, new]))
    assert len(np.unique(ids)) == n_pts
    return ids.astype(np.int32), new_from


def _slid(n_cams):
    return np.array(list(range(1, n_cams)) + [-1], np.int32)


# name -> (n_cams, n_pts, cam_src, mode, k1, k0, vel, pose_from_reference)
_CHAIN = {
    "mode1-slid-by-one-8cams-700pts": (8, 700, _slid(8), 1, 6, 5, False, False),
    "mode1-unmoved-pose-equals-prediction-255pts": (8, 255, _slid(8), 1, 6, 5, False, True),
    "mode0-velocity-hole-in-the-middle-257pts": (8, 257, [0, 1, -1, 3, 4, 5, 6, -1], 0, 6, -1, True, False),
    "mode-1-kept-permuted-sources-256pts": (8, 256, [3, 0, 2, 1, 7, 6, 5, 4], -1, -1, -1, False, False),
    "mode1-k1-from-the-host-value-256pts": (8, 256, [1, 2, 3, 4, 5, 6, -1, -1], 1, 6, 5, False, False),
    "mode1-k0-from-the-host-value-1pt": (8, 1, [1, 2, 3, 4, 5, -1, 7, -1], 1, 6, 5, False, False),
    "mode0-2cams-1pt": (2, 1, [3, -1], 0, 0, -1, True, False),
    "mode1-2cams-k0-equals-k1-257pts": (2, 257, [7, -1], 1, 0, 0, False, False),
    "mode1-50cams-700pts": (50, 700, [(3 * k) % 8 if k % 7 else -1 for k in range(49)] + [-1], 1, 48, 47, False, False),
    "mode1-no-landmarks-8cams": (8, 0, _slid(8), 1, 6, 5, False, False),
    "mode0-no-landmarks-50cams": (50, 0, [k % 8 for k in range(49)] + [-1], 0, 48, -1, True, False),
    "mode1-nothing-new-new_from-int32-max-100pts": (8, 100, _slid(8), 1, 6, 5, False, False),
}
CHAIN_NAMES = tuple(_CHAIN)
NOTHING_NEW = "mode1-nothing-new-new_from-int32-max-100pts"  # the loop's new_from on a keyframe without new tracks


@functools.lru_cache(maxsize=None)
def chain_case(name):
    n_cams, n_pts, cam_src, mode, k1, k0, vel, from_ref = _CHAIN[name]
    _, prev_ids = chain_source()
    rng = np.random.default_rng(sum(map(ord, name)))
    cams = _host_cams(rng, n_cams)
    win_ids, new_from = _chain_landmarks(rng, n_pts, prev_ids)
    if name == NOTHING_NEW:  # the new IDs stay, the largest of them the previous window's last: all found or kept
        new_from = 2 ** 31 - 1
    pts = rng.normal(0.0, 3.0, (n_pts, 3)) + np.array([0.0, 0.0, 20.0])
    pose = cams[-1] + rng.normal(0.0, 0.01, 6)  # the first prediction the new landmarks were triangulated at
    args = ChainArgs(pose, PL.aa_to_R(pose[3:]), rng.normal(0.0, 0.05, 6) if vel else np.zeros(6), k1, k0, mode)
    return ChainCase(cams, pts, np.asarray(cam_src, np.int32), win_ids, new_from, args, from_ref)


def chain_reference(case, prev_cams, prev_pts, prev_ok):
    """(cams, pts) chain_host gives for the case, and the args to call the
    device with (args.pose replaced by the reference's pose(t) where the case
    asks for it)."""
    _, prev_ids = chain_source()
    args = case.args
    if case.pose_from_reference:
        pose2, _ = chain_pose2(prev_cams, prev_ok, case.cams, case.cam_src, args)
        args = ChainArgs(pose2.copy(), PL.aa_to_R(pose2[3:]), args.vel, args.k1, args.k0, args.mode)
    return chain_host(prev_cams, prev_pts, prev_ok, case.cams, case.pts, case.cam_src, case.win_ids, prev_ids,
                      case.new_from, args), args


# ------------------------------------------------------------------ me_vo_window_submit inputs
@dataclass
class Window:
    first_frame: int
    cams: np.ndarray      # (nc, 6) the loop's values before any solve
    win_ids: np.ndarray   # (np,) int32 ascending
    pts: np.ndarray       # (np, 3)
    lo: int               # the window's observations: rows [lo, hi) of the store
    hi: int


@dataclass
class WindowPair:
    """Two consecutive windows over one observation store kept frame by frame
    (obs (n, 4), frame, ids): window 2 drops window 1's oldest camera and adds
    one, keeps the tracks still seen and adds new ones with larger IDs."""
    obs: np.ndarray
    frame: np.ndarray
    ids: np.ndarray
    K: np.ndarray
    baseline: float
    feat_var: float
    w1: Window
    w2: Window
    cam_src: np.ndarray
    new_from: int
    args: ChainArgs

    def problem(self, w, cams=None, pts=None):
        """The window as a host BAProblem (window_indices_host indices)."""
        sl = slice(w.lo, w.hi)
        ci, pi = window_indices_host(self.frame[sl], self.ids[sl], w.first_frame, w.win_ids)
        assert pi.min() >= 0 and ci.min() >= 0 and ci.max() < len(w.cams)
        return S.BAProblem(np.array(w.cams if cams is None else cams), np.array(w.pts if pts is None else pts),
                           self.obs[sl], ci, pi, self.K.copy(), self.K.copy(), self.baseline, self.feat_var, 2)


@functools.lru_cache(maxsize=None)
def window_pair(first_frame=11, n_cams=6, n_pts=150):
    bp = S.ba_problem(33, n_pts, n_cams + 1, 640, 480)
    ci, pi = bp.cam_idx.astype(np.int64), bp.pt_idx.astype(np.int64)
    npt = len(bp.pts)
    start = np.full(npt, n_cams + 1)
    end = np.full(npt, -1)
    np.minimum.at(start, pi, ci)
    np.maximum.at(end, pi, ci)
    new = start == n_cams - 1       # seen in the last two keyframes only: made new in the last one
    gone = end == 1                 # seen in the first two only: made to leave with the first
    keep = ~((new[pi] & (ci == n_cams - 1)) | (gone[pi] & (ci == 1)))
    ci, pi, obs = ci[keep], pi[keep], bp.obs[keep]
    # track IDs ascending with gaps, the new tracks last (the loop numbers tracks in creation order)
    order = np.argsort(new, kind="stable")
    tid = np.empty(npt, np.int64)
    tid[order] = gapped_ids(np.random.default_rng(9), npt, first=500)
    o = np.lexsort((tid[pi], ci))   # the store: frame by frame, ascending IDs inside a frame
    ci, pi, obs = ci[o], pi[o], np.ascontiguousarray(obs[o])
    frame = (first_frame + ci).astype(np.int32)
    ids = tid[pi].astype(np.int32)

    def window(c0):
        lo, hi = int(np.searchsorted(ci, c0)), int(np.searchsorted(ci, c0 + n_cams))
        pw = np.unique(pi[lo:hi])
        pw = pw[np.argsort(tid[pw])]
        return Window(first_frame + c0, bp.cams[c0:c0 + n_cams].copy(), tid[pw].astype(np.int32), bp.pts[pw].copy(),
                      lo, hi)

    w1, w2 = window(0), window(1)
    new_from = int(tid[new].min())
    assert new.sum() >= 5 and gone.sum() >= 1 and not np.isin(tid[new], w1.win_ids).any()
    assert np.isin(tid[new], w2.win_ids).all() and not np.isin(tid[gone], w2.win_ids).any()
    pose = w2.cams[-1].copy()
    args = ChainArgs(pose, PL.aa_to_R(pose[3:]), np.zeros(6), n_cams - 2, n_cams - 3, 1)
    return WindowPair(obs, frame, ids, bp.K0.copy(), float(bp.baseline), float(bp.feat_var), w1, w2, _slid(n_cams),
                      new_from, args)
