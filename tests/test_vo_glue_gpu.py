"""The VO loop's device-side glue against its numpy restatements
(vo_glue_cases.py), bit for bit, at shapes that take milliseconds:
me_vo_new_cells (vo_cells_kernel, csrc/vo.hip), me_ba_window_indices
(window_indices_kernel), me_vo_ba_chain (vo_chain_kernel) and
me_vo_window_submit / me_ba_wait_out / me_ba_reserve (csrc/ba.hip).  The loop
tests reach these only at config 5 and only along the paths that loop takes;
here each kernel sees the grids, counts, modes and sources its code branches
on.  Floats are compared as integer views; every output buffer is pre-filled
with a sentinel byte that must survive past the defined outputs."""
import ctypes

import numpy as np
import pytest

import vo_glue_cases as C
from uasl_motion_estimation_amd._lib import ME_DEVICE, BAProblemC, BASummaryC, Context, VOWindowC
from uasl_motion_estimation_amd.optimisation import DeviceBAProblem, SolverOptions, _summary, ba_struct

pytestmark = pytest.mark.gpu
V = ctypes.c_void_p
SENTINEL = 0x7f
ME_ERR_INVALID, ME_ERR_STATE = -1, -5
FAILURE = 2  # me_ba_summary.termination


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Bufs:
    """Device buffers freed together."""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.ctx.malloc(max(a.nbytes, 16))
        self.all.append(p)
        if a.nbytes:
            self.ctx.h2d(p, a)
        return p

    def sentinel(self, nbytes):
        return self.up(np.full(nbytes, SENTINEL, np.uint8))

    def read(self, p, dtype, count):
        out = np.empty(count, dtype)
        if count:
            self.ctx.d2h(out, p)
        return out

    def close(self):
        self.ctx.synchronize()
        for p in self.all:
            self.ctx.free(p)
        self.all = []


@pytest.fixture
def bufs(ctx):
    b = Bufs(ctx)
    yield b
    b.close()


def last_error(ctx):
    return ctx.lib.me_last_error(ctx.h) or b""


# ------------------------------------------------------------------ a. me_vo_new_cells
def new_cells_device(ctx, bufs, d_in, n, width, height, grid, t, d_min, d_out, cap):
    """One call on uploaded inputs; returns (uv (cap, 2), lo (cap,), count (4,)) as raw arrays."""
    nx, ny, cw, ch, n_feats = grid
    d_uv, d_lo, d_cnt = d_out
    fill = np.full(8 * cap, SENTINEL, np.uint8)
    ctx.h2d(d_uv, fill)
    ctx.h2d(d_lo, fill[:4 * cap])
    ctx.h2d(d_cnt, fill[:16])
    ctx.check(ctx.lib.me_vo_new_cells(ctx.h, V(d_in[0]), V(d_in[1]), V(d_in[2]), n, width, height, float(C.MARGIN), nx,
                                      ny, cw, ch, n_feats, t, d_min, V(d_uv), V(d_lo), V(d_cnt)), "me_vo_new_cells")
    ctx.synchronize()
    return (bufs.read(d_uv, np.float32, 2 * cap).reshape(cap, 2), bufs.read(d_lo, np.int32, cap),
            bufs.read(d_cnt, np.int32, 4))


@pytest.mark.parametrize("name", list(C.GRIDS))
def test_new_cells_equal_the_host_restatement(ctx, bufs, name):
    """Every grid (named for the path of vo_cells_kernel it takes) x feature
    count (none: NULL inputs; one trip and three trips of the feature loop) x
    regime of want (0, below the empty count, above it: out_count clipped) x
    keyframe (the last two wrap the hash's 32-bit products): the new
    features, lo = d_min and the count, bit for bit; nothing past them
    written.  Each input rejects features by every gate term."""
    (nx, ny, cw, ch, _), (width, height) = C.cell_grid(name)
    cap = nx * ny + 8
    d_out = (bufs.sentinel(8 * cap), bufs.sentinel(4 * cap), bufs.sentinel(16))
    word = np.frombuffer(bytes([SENTINEL] * 4), np.uint32)[0]
    regimes_seen = set()
    for n in C.CELL_N:
        uv, status, ok = C.cell_features(name, n)
        good, empty = C.cell_occupancy(name, n)
        if n:
            assert min(C.cell_gate_counts(name, n)) >= 1 and good > 0
        d_in = (bufs.up(uv), bufs.up(status), bufs.up(ok)) if n else (None, None, None)
        for regime, n_feats in C.cell_n_feats(name, n).items():
            want = max(0, n_feats - good)
            assert {"none": want == 0, "some": 0 < want < empty, "all": want > empty}[regime]
            regimes_seen.add(regime)
            grid = (nx, ny, cw, ch, n_feats)
            for t in C.CELL_T:
                d_min = 3 + (t & 3)
                ref_uv, ref_lo = C.cells_host(t, uv, status, ok, width, height, grid, d_min)
                k = len(ref_uv)
                assert k == min(want, empty)
                got_uv, got_lo, got_cnt = new_cells_device(ctx, bufs, d_in, n, width, height, grid, t, d_min, d_out,
                                                           cap)
                where = (name, n, regime, t)
                assert got_cnt[0] == k and np.all(bits(got_cnt[1:]) == word), where
                assert np.array_equal(bits(got_uv[:k]), bits(ref_uv)), where
                assert np.array_equal(got_lo[:k], ref_lo), where
                assert np.all(bits(got_uv[k:]) == word) and np.all(bits(got_lo[k:]) == word), where
    assert regimes_seen == ({"none", "all"} if nx * ny == 1 else {"none", "some", "all"})


def test_new_cells_argument_errors_leave_the_context_usable(ctx, bufs):
    name = "37x28-chunk-2-tail-word"
    (nx, ny, cw, ch, _), (width, height) = C.cell_grid(name)
    n = 700
    uv, status, ok = C.cell_features(name, n)
    d_in = (bufs.up(uv), bufs.up(status), bufs.up(ok))
    cap = nx * ny + 8
    d_out = (bufs.sentinel(8 * cap), bufs.sentinel(4 * cap), bufs.sentinel(16))
    grid = (nx, ny, cw, ch, C.cell_n_feats(name, n)["some"])
    ref_uv, _ = C.cells_host(7, uv, status, ok, width, height, grid)

    def call(n=n, nx=nx, ny=ny, cw=cw):
        return ctx.lib.me_vo_new_cells(ctx.h, V(d_in[0]), V(d_in[1]), V(d_in[2]), n, width, height, float(C.MARGIN),
                                       nx, ny, cw, ch, grid[4], 7, 0, V(d_out[0]), V(d_out[1]), V(d_out[2]))

    for bad in (dict(nx=65537, ny=1), dict(nx=0), dict(cw=0.0), dict(n=-1)):
        assert call(**bad) == ME_ERR_INVALID, bad
        assert b"me_vo_new_cells" in last_error(ctx)
        got_uv, _, got_cnt = new_cells_device(ctx, bufs, d_in, n, width, height, grid, 7, 0, d_out, cap)
        assert got_cnt[0] == len(ref_uv) and np.array_equal(bits(got_uv[:len(ref_uv)]), bits(ref_uv))


# ------------------------------------------------------------------ b. me_ba_window_indices
def window_indices_device(ctx, bufs, frame, ids, first_frame, win_ids):
    n_obs, pad = len(ids), 8
    d_ci, d_pi = bufs.sentinel(4 * (n_obs + pad)), bufs.sentinel(4 * (n_obs + pad))
    d_f, d_i, d_w = (bufs.up(a) if len(a) else None for a in (frame, ids, win_ids))
    ctx.check(ctx.lib.me_ba_window_indices(ctx.h, V(d_f), V(d_i), n_obs, first_frame, V(d_w), len(win_ids), V(d_ci),
                                           V(d_pi)), "me_ba_window_indices")
    ctx.synchronize()
    return bufs.read(d_ci, np.int32, n_obs + pad), bufs.read(d_pi, np.int32, n_obs + pad)


@pytest.mark.parametrize("n_pts", C.INDEX_N_PTS)
@pytest.mark.parametrize("n_obs", C.INDEX_N_OBS)
def test_window_indices_equal_the_host_restatement(ctx, bufs, n_obs, n_pts):
    check_window_indices(ctx, bufs, C.index_case(n_obs, n_pts))


def test_window_indices_with_ids_near_int32_max(ctx, bufs):
    case = C.index_case(1000, 300, high=True)
    assert case[3][-1] == 2 ** 31 - 3 and case[1].max() == 2 ** 31 - 1
    check_window_indices(ctx, bufs, case)


def check_window_indices(ctx, bufs, case):
    frame, ids, first_frame, win_ids = case
    n_obs, n_pts = len(ids), len(win_ids)
    assert first_frame != 0 and (n_pts < 2 or np.diff(win_ids.astype(np.int64)).min() >= 2)
    ref_ci, ref_pi = C.window_indices_host(frame, ids, first_frame, win_ids)
    if n_obs >= 255:
        assert (ref_pi == -1).sum() >= 10
        assert (ref_pi >= 0).sum() >= (10 if n_pts else 0)
        if n_pts:  # below the first ID, above the last, inside a gap
            i64 = ids.astype(np.int64)
            assert (i64 < win_ids[0]).any() and (i64 > win_ids[-1]).any()
            assert n_pts < 2 or ((i64 > win_ids[0]) & (i64 < win_ids[-1]) & (ref_pi == -1)).any()
    if n_pts == 0:
        assert np.all(ref_pi == -1)
    got_ci, got_pi = window_indices_device(ctx, bufs, frame, ids, first_frame, win_ids)
    assert np.array_equal(got_ci[:n_obs], ref_ci) and np.array_equal(got_pi[:n_obs], ref_pi)
    word = np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]
    assert np.all(got_ci[n_obs:] == word) and np.all(got_pi[n_obs:] == word)


# ------------------------------------------------------------------ c. me_vo_ba_chain
SRC_ITERS = 3


@pytest.fixture
def source(ctx):
    """The chained-from window, device-resident; closed after the test has read the chain's output."""
    bp, _ = C.chain_source()
    dp = DeviceBAProblem(bp, ctx)
    yield dp
    ctx.synchronize()
    dp.close()


def chain_upload(bufs, case, prev_ids):
    """The case's host values and index arrays on the device (uploads wait for
    the stream: done before the source solve is queued)."""
    pad = np.full(16, SENTINEL, np.uint8)
    return dict(c=bufs.up(np.concatenate([case.cams.ravel().view(np.uint8), pad])),
                p=bufs.up(np.concatenate([case.pts.ravel().view(np.uint8), pad])),
                s=bufs.up(case.cam_src), w=bufs.up(case.win_ids), i=bufs.up(prev_ids), n_prev=len(prev_ids))


def chain_call(ctx, d, case, args, cams=True):
    a = args.to_c()
    return ctx.lib.me_vo_ba_chain(ctx.h, V(d["c"]) if cams else None, len(case.cams), V(d["p"]), len(case.pts),
                                  V(d["s"]), V(d["w"]), V(d["i"]), d["n_prev"], case.new_from, ctypes.byref(a))


def chain_read(bufs, d, case):
    """(cams, pts) on the device; their sentinel tails intact."""
    nc, npts = len(case.cams), len(case.pts)
    c = bufs.read(d["c"], np.uint8, 48 * nc + 16)
    p = bufs.read(d["p"], np.uint8, 24 * npts + 16)
    assert np.all(c[48 * nc:] == SENTINEL) and np.all(p[24 * npts:] == SENTINEL)
    return c[:48 * nc].view(np.float64).reshape(nc, 6), p[:24 * npts].view(np.float64).reshape(npts, 3)


def check_chain(case, got, prev, prev_ok):
    """The device's (cams, pts) against chain_host on the downloaded previous
    result; the case's landmark classes are populated."""
    _, prev_ids = C.chain_source()
    (ref_c, ref_p), args = C.chain_reference(case, prev[0], prev[1], prev_ok)
    found, kept, new = case.classes(prev_ids)
    if len(case.pts) >= 255:
        assert found >= 20 and kept >= 5 and new >= 20
        ids = case.win_ids.astype(np.int64)
        assert np.isin(ids[ids >= case.new_from], prev_ids).sum() == 1
    if case.new_from == 2 ** 31 - 1:  # (a keyframe without new tracks)
        assert found >= 20 and kept >= 20 and new == 0
    moved = bool(np.any(ref_c[-1] != args.pose))
    assert moved != case.pose_from_reference
    assert np.array_equal(bits(got[0]), bits(ref_c))
    assert np.array_equal(bits(got[1]), bits(ref_p))
    return ref_c, ref_p


def run_chain(ctx, bufs, source, name, iters=SRC_ITERS, after_wait=False):
    """Queue the source solve, call the chain while it is queued (or after the
    wait: the retained last solve), then wait and download the previous result."""
    case = C.chain_case(name)
    _, prev_ids = C.chain_source()
    d = chain_upload(bufs, case, prev_ids)
    source.reset()
    source.solve_async(SolverOptions.fixed_iterations(iters))
    summ = None
    if after_wait:
        summ = source.wait()
    try:
        # (the reference needs the previous result, which the call must not wait for: the case's own
        # args, except where args.pose is the reference's pose(t) -- that case chains after the wait)
        if case.pose_from_reference:
            assert after_wait
            _, args = C.chain_reference(case, *source.download(), summ["termination"] != FAILURE)
        else:
            args = case.args
        rc = chain_call(ctx, d, case, args)
    finally:
        if summ is None:
            summ = source.wait()
    ctx.check(rc, "me_vo_ba_chain")
    prev = source.download()
    got = chain_read(bufs, d, case)
    return case, got, prev, summ


@pytest.mark.parametrize("name", [n for n in C.CHAIN_NAMES if not C.chain_case(n).pose_from_reference])
def test_chain_behind_a_queued_solve_equals_the_host_restatement(ctx, bufs, source, name):
    case, got, prev, summ = run_chain(ctx, bufs, source, name)
    assert summ["termination"] != FAILURE and summ["iterations"] == SRC_ITERS
    ref_c, _ = check_chain(case, got, prev, True)
    assert not np.array_equal(prev[0], source.bp.cams)  # (the solve moved the cameras: sourced != host values)
    if len(case.pts) == 0:  # the cameras are written all the same
        assert not np.array_equal(bits(ref_c), bits(case.cams))


@pytest.mark.parametrize("name", ["mode1-unmoved-pose-equals-prediction-255pts", "mode1-slid-by-one-8cams-700pts"])
def test_chain_from_the_retained_last_solve(ctx, bufs, source, name):
    """After the wait the newest waited solve stays the chain source.  The
    unmoved case runs here: its args.pose is the reference's pose(t), known
    once the previous result is."""
    case, got, prev, summ = run_chain(ctx, bufs, source, name, after_wait=True)
    assert summ["termination"] != FAILURE
    check_chain(case, got, prev, True)


@pytest.mark.parametrize("name", ["mode1-slid-by-one-8cams-700pts", "mode0-velocity-hole-in-the-middle-257pts",
                                  "mode1-k1-from-the-host-value-256pts"])
def test_chain_after_a_failed_solve_keeps_the_host_values(ctx, bufs, source, name):
    """Test hook 1024: every camera solve of the source fails and it ends with
    termination FAILURE.  Sourced cameras and found landmarks keep the host
    values, pose(t) is predicted from host values, new landmarks still move."""
    hook = ctx.lib.me_debug_solve_flags
    hook.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert hook(ctx.h, 1024) == 0
    try:
        case, got, prev, summ = run_chain(ctx, bufs, source, name, iters=8)
    finally:
        hook(ctx.h, 0)
    assert summ["termination"] == FAILURE and summ["status"] == 3, summ
    ref_c, ref_p = check_chain(case, got, prev, False)
    assert np.array_equal(bits(ref_c[:-1]), bits(case.cams[:-1]))
    ids = case.win_ids.astype(np.int64)
    old = ids < case.new_from
    assert np.array_equal(bits(ref_p[old]), bits(case.pts[old]))
    assert not np.array_equal(ref_p[~old], case.pts[~old])
    # the success case differs: a reference that ignored the failure would not pass
    (ok_c, ok_p), _ = C.chain_reference(case, prev[0] + 1e-3, prev[1] + 1e-3, True)
    assert not np.array_equal(ok_c, ref_c) and not np.array_equal(ok_p, ref_p)


def test_chain_state_and_argument_errors(ctx, bufs, source):
    name = "mode1-slid-by-one-8cams-700pts"
    case = C.chain_case(name)
    bp, prev_ids = C.chain_source()
    nc = len(case.cams)

    def valid():
        c, got, prev, summ = run_chain(ctx, bufs, source, name)
        check_chain(c, got, prev, summ["termination"] != FAILURE)

    # no solve on the context yet
    d = chain_upload(bufs, case, prev_ids)
    with Context(ctx.device) as fresh:
        assert chain_call(fresh, d, case, case.args) == ME_ERR_STATE and b"no BA solve" in last_error(fresh)
    valid()
    # the newest solve works on host memory
    keep = []
    p, _, _ = ba_struct(bp, keep)
    o = SolverOptions.fixed_iterations(SRC_ITERS).to_c()
    ctx.check(ctx.lib.me_ba_solve_async(ctx.h, ctypes.byref(p), ctypes.byref(o)), "me_ba_solve_async")
    try:
        rc = chain_call(ctx, d, case, case.args)
        assert rc == ME_ERR_STATE and b"not device-resident" in last_error(ctx)
    finally:
        ctx.check(ctx.lib.me_ba_wait(ctx.h, None), "me_ba_wait")
    valid()
    # prediction cameras outside the window's first n_cams - 1
    for k1, k0, mode in ((nc - 1, 0, 1), (-1, 0, 1), (nc - 1, 0, 0), (0, nc - 1, 1), (0, -1, 1)):
        a = C.ChainArgs(case.args.pose, case.args.R, case.args.vel, k1, k0, mode)
        assert chain_call(ctx, d, case, a) == ME_ERR_INVALID, (k1, k0, mode)
        msg = last_error(ctx)
        assert b"prediction cameras %d, %d" % (k1, k0) in msg and b"first %d" % (nc - 1) in msg
        valid()
    assert chain_call(ctx, d, case, case.args, cams=False) == ME_ERR_INVALID
    valid()
    got = chain_read(bufs, d, case)  # the refused calls wrote nothing
    assert np.array_equal(bits(got[0]), bits(case.cams)) and np.array_equal(bits(got[1]), bits(case.pts))


# ------------------------------------------------------------------ d. me_vo_window_submit / me_ba_wait_out / reserve
WIN_ITERS = 3


def _solve_sync(ctx, bp):
    dp = DeviceBAProblem(bp, ctx)
    try:
        summ = dp.solve(SolverOptions.fixed_iterations(WIN_ITERS))
        return dp.download() + (summ,)
    finally:
        dp.close()


@pytest.fixture(scope="module")
def pair_reference(ctx):
    """Window 1 solved synchronously on the host restatement's indices, then
    chain_host on its result and window 2 solved synchronously."""
    wp = C.window_pair()
    c1, p1, s1 = _solve_sync(ctx, wp.problem(wp.w1))
    start_c, start_p = C.chain_host(c1, p1, s1["termination"] != FAILURE, wp.w2.cams, wp.w2.pts, wp.cam_src,
                                    wp.w2.win_ids, wp.w1.win_ids, wp.new_from, wp.args)
    # the chain does something to every class: sourced cameras, a re-predicted pose, found and moved landmarks
    assert not np.array_equal(start_c[:-1], wp.w2.cams[:-1]) and not np.array_equal(start_c[-1], wp.args.pose)
    new = wp.w2.win_ids >= wp.new_from
    assert new.sum() >= 5 and (~new).sum() >= 20
    assert not np.array_equal(start_p[new], wp.w2.pts[new]) and not np.array_equal(start_p[~new], wp.w2.pts[~new])
    c2, p2, s2 = _solve_sync(ctx, wp.problem(wp.w2, start_c, start_p))
    assert s1["iterations"] == WIN_ITERS and s2["iterations"] == WIN_ITERS
    return (c1, p1, s1), (c2, p2, s2)


class SubmittedPair:
    """The pair queued through me_vo_window_submit: window 2 chained behind
    window 1 before window 1 is waited."""

    def __init__(self, ctx, bufs, staged=True):
        self.ctx, self.bufs, self.wp = ctx, bufs, C.window_pair()
        wp = self.wp
        self.d_obs, self.d_frame, self.d_ids = bufs.up(wp.obs), bufs.up(wp.frame), bufs.up(wp.ids)
        self.stages, self.sets, self.keep = [], [], []
        self.opt = SolverOptions.fixed_iterations(WIN_ITERS).to_c()
        self.queued = 0
        try:
            # every upload first (a blocking copy waits for the stream), then the two submits back to back
            for w, chain in ((wp.w1, False), (wp.w2, True)):
                self._prepare(w, chain, staged)
            for win, p in self.keep:
                ctx.check(ctx.lib.me_vo_window_submit(ctx.h, ctypes.byref(win), ctypes.byref(p),
                                                      ctypes.byref(self.opt)), "me_vo_window_submit")
                self.queued += 1
        except Exception:
            self.close()
            raise

    def _prepare(self, w, chain, staged):
        ctx, wp = self.ctx, self.wp
        nc, npts, n_obs = len(w.cams), len(w.pts), w.hi - w.lo
        o_ids = 48 * nc + 24 * npts
        o_cs = o_ids + 4 * npts
        nb = o_cs + 4 * nc
        block = np.concatenate([w.cams.ravel().view(np.uint8), w.pts.ravel().view(np.uint8), w.win_ids.view(np.uint8),
                                wp.cam_src.view(np.uint8)])
        assert block.nbytes == nb
        d = self.bufs.sentinel(nb + 16)
        d_idx = self.bufs.sentinel(8 * n_obs + 16)
        win = VOWindowC()
        if staged:  # cams | pts | win_ids (| cam_src) from page-locked memory, inside the call
            hp = ctx.host_alloc(nb)
            self.stages.append(hp)
            ctypes.memmove(hp, block.ctypes.data, nb)
            win.stage, win.dev, win.stage_bytes = hp, d, nb if chain else o_cs
        else:
            ctx.h2d(d, block)
            win.stage, win.dev, win.stage_bytes = None, None, 0
        if chain:
            prev = self.sets[-1]
            win.chain, win.cam_src, win.prev_ids, win.n_prev = 1, d + o_cs, prev["d"] + prev["o_ids"], prev["npts"]
            win.new_from, win.args = wp.new_from, wp.args.to_c()
        win.win_ids, win.first_frame = d + o_ids, w.first_frame
        win.frame, win.ids = self.d_frame + 4 * w.lo, self.d_ids + 4 * w.lo
        p = BAProblemC()
        p.n_cams, p.n_pts, p.n_obs = nc, npts, n_obs
        p.cams = ctypes.cast(d, ctypes.POINTER(ctypes.c_double))
        p.pts = ctypes.cast(d + 48 * nc, ctypes.POINTER(ctypes.c_double))
        p.obs = ctypes.cast(self.d_obs + 32 * w.lo, ctypes.POINTER(ctypes.c_double))
        p.cam_idx = ctypes.cast(d_idx, ctypes.POINTER(ctypes.c_int32))
        p.pt_idx = ctypes.cast(d_idx + 4 * n_obs, ctypes.POINTER(ctypes.c_int32))
        p.K0[:] = [float(x) for x in wp.K.ravel()]
        p.K1[:] = [float(x) for x in wp.K.ravel()]
        p.baseline, p.feat_var, p.fixed_frames, p.mem, p.obs_dim = wp.baseline, wp.feat_var, 2, ME_DEVICE, 4
        self.keep.append((win, p))
        self.sets.append(dict(d=d, o_ids=o_ids, npts=npts, nc=nc, n_obs=n_obs, d_idx=d_idx, w=w, nb=nb))

    def wait_out(self, k, cams=True, pts=True):
        """me_ba_wait_out of window k (the oldest queued): (cams, pts, summary), None for a NULL array."""
        st, pad = self.sets[k], 4
        c = np.full(6 * st["nc"] + pad, np.nan)
        p = np.full(3 * st["npts"] + pad, np.nan)
        c.view(np.uint8)[:] = SENTINEL
        p.view(np.uint8)[:] = SENTINEL
        s = BASummaryC()
        self.ctx.check(self.ctx.lib.me_ba_wait_out(self.ctx.h, ctypes.byref(s), V(c.ctypes.data) if cams else None,
                                                   V(p.ctypes.data) if pts else None), "me_ba_wait_out")
        self.queued -= 1
        for a, n, given in ((c, 6 * st["nc"], cams), (p, 3 * st["npts"], pts)):
            assert np.all(a.view(np.uint8)[8 * (n if given else 0):] == SENTINEL)
        return (c[:6 * st["nc"]].reshape(-1, 6) if cams else None, p[:3 * st["npts"]].reshape(-1, 3) if pts else None,
                _summary(s))

    def check_indices(self):
        """The cam_idx / pt_idx the calls filled equal the host restatement's; nothing past them written."""
        for st in self.sets:
            w, n = st["w"], st["n_obs"]
            raw = self.bufs.read(st["d_idx"], np.uint8, 8 * n + 16)
            ci, pi = C.window_indices_host(self.wp.frame[w.lo:w.hi], self.wp.ids[w.lo:w.hi], w.first_frame, w.win_ids)
            assert np.array_equal(raw[:4 * n].view(np.int32), ci)
            assert np.array_equal(raw[4 * n:8 * n].view(np.int32), pi)
            assert np.all(raw[8 * n:] == SENTINEL)
            tail = self.bufs.read(st["d"] + st["nb"], np.uint8, 16)
            assert np.all(tail == SENTINEL)

    def close(self):
        try:
            while self.queued > 0:  # (nothing may stay queued on the shared context)
                self.queued -= 1
                self.ctx.lib.me_ba_wait(self.ctx.h, None)
            self.ctx.synchronize()
        finally:
            for hp in self.stages:
                self.ctx.host_free(hp)
            self.stages = []


def same_result(got, ref, cams=True, pts=True):
    assert got[2] == ref[2], (got[2], ref[2])
    if cams:
        assert np.array_equal(bits(got[0]), bits(ref[0]))
    if pts:
        assert np.array_equal(bits(got[1]), bits(ref[1]))


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "stage_bytes-0"])
def test_window_pair_equals_synchronous_solves_around_chain_host(ctx, bufs, pair_reference, staged):
    """Window 1 unchained, window 2 chained behind it before it is waited:
    each me_ba_wait_out result equals the synchronous solve of the same
    arrays (window 2's from chain_host on window 1's result), bit for bit,
    summaries included; the indices the calls filled are the host's."""
    sp = SubmittedPair(ctx, bufs, staged)
    try:
        r1 = sp.wait_out(0)
        r2 = sp.wait_out(1)
        sp.check_indices()
    finally:
        sp.close()
    same_result(r1, pair_reference[0])
    same_result(r2, pair_reference[1])
    assert not np.array_equal(r2[0][:5], r1[0][1:])  # (window 2 was solved, not just chained)


def test_wait_out_with_null_arrays_and_with_nothing_queued(ctx, bufs, pair_reference):
    sp = SubmittedPair(ctx, bufs)
    try:
        r1 = sp.wait_out(0, cams=False)
        r2 = sp.wait_out(1, pts=False)
    finally:
        sp.close()
    same_result(r1, pair_reference[0], cams=False)
    same_result(r2, pair_reference[1], pts=False)
    s = BASummaryC()
    c = np.zeros(6 * 6)
    assert ctx.lib.me_ba_wait_out(ctx.h, ctypes.byref(s), V(c.ctypes.data), None) == ME_ERR_STATE
    assert b"no asynchronous BA solve" in last_error(ctx)
    assert not c.any()


def test_reserve_leaves_every_result_bit_unchanged(ctx, bufs, pair_reference):
    """me_ba_reserve with larger sizes ahead of the pair: the same bits;
    ME_ERR_STATE while a solve is queued, and the queued solves unharmed."""
    wp = C.window_pair()
    n_obs = len(wp.obs)
    ctx.check(ctx.lib.me_ba_reserve(ctx.h, 12, 4 * len(wp.w2.pts), 4 * n_obs, 4, 2), "me_ba_reserve")
    sp = SubmittedPair(ctx, bufs)
    try:
        assert ctx.lib.me_ba_reserve(ctx.h, 16, 8 * len(wp.w2.pts), 8 * n_obs, 4, 2) == ME_ERR_STATE
        assert b"me_ba_reserve" in last_error(ctx)
        r1 = sp.wait_out(0)
        assert ctx.lib.me_ba_reserve(ctx.h, 16, 8 * len(wp.w2.pts), 8 * n_obs, 4, 2) == ME_ERR_STATE
        r2 = sp.wait_out(1)
        sp.check_indices()
    finally:
        sp.close()
    same_result(r1, pair_reference[0])
    same_result(r2, pair_reference[1])
    # and the synchronous path afterwards
    c1, p1, s1 = _solve_sync(ctx, wp.problem(wp.w1))
    same_result((c1, p1, s1), pair_reference[0])
