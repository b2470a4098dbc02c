"""The native VO loop's host logic on the CPU (csrc/vo_tracks.hpp, csrc/vo_math.hpp).

tests/cpp/vo_host_cli (no HIP, no libme_hip.so) runs the loop's track table through a script of keyframes and
the loop's arithmetic through seeded inputs; values cross as raw bits.  The table's events are replayed through
feature_types.WBA_Point exactly as test_pipeline._replay does for the Python loop; the arithmetic is compared
with pipeline.py / synthetic.py, bit for bit where both sides use only + - * /, rounding and comparisons.
"""
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from uasl_motion_estimation_amd import pipeline as PL
from uasl_motion_estimation_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "tests", "cpp", "vo_host_cli")


def _cli(mode, src, dst):
    assert os.path.exists(CLI), "build() compiles tests/cpp/vo_host_cli"
    p = subprocess.run([CLI, mode, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)


# ------------------------------------------------------------------------------------------------ track table
WINDOW, N_FRAMES = 3, 12
# Per keyframe: which of the active tracks (= the previous keyframe's features, ascending ID) continue, and how
# many new features are accepted.  IDs in the comments; pop(t - 3) runs at the start of keyframe t.
_PLAN = [
    ([], 6),                        # 0: 0..5
    ([1] * 6, 2),                   # 1: every track continues; 6, 7
    ([0, 1, 1, 0, 1, 1, 1, 1], 0),  # 2: 0 and 3 lost; no new feature
    ([1] * 6, 2),                   # 3: 8, 9; pop(0) deletes nothing
    ([1] * 6 + [0, 0], 0),          # 4: 8, 9 lost; frame 0 popped, the tracks live on (first bumped)
    ([1] * 6, 0),                   # 5: pop(2) deletes 0 (first row) and 3 (a middle row)
    ([1] * 6, 0),                   # 6
    ([0] * 6, 3),                   # 7: pop(4) deletes 8, 9 (the last rows); all tracks lost; 10, 11, 12
    ([1, 1, 0], 1),                 # 8: 12 lost; 13
    ([1] * 3, 0),                   # 9
    ([1] * 3, 0),                   # 10: pop(7) deletes 1, 2, 4, 5, 6, 7 (the first rows)
    ([1] * 3, 1),                   # 11: pop(8) deletes 12 (a middle row); 14
]


def _script(path, seed=20240917):
    """The script file of `vo_host_cli tracks` (its layout is described there)."""
    rng = np.random.default_rng(seed)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<ii", WINDOW, N_FRAMES))
        for t, (mask, n_new) in enumerate(_PLAN):
            m = np.zeros(8, np.uint8)
            m[:len(mask)] = mask
            sub = np.zeros(8, np.uint8)
            sub[:len(mask)] = rng.integers(0, 2, len(mask))
            if len(mask) > 1:
                sub[0], sub[1] = 1, 0  # a proper, non-empty part of the active tracks
            fh.write(m.tobytes() + sub.tobytes())
            fh.write(rng.uniform(30.0, 600.0, 24).astype(np.float32).tobytes())
            # candidates: the accepted ones among some rejected ones (none at all in keyframe 9)
            ok = [1] * n_new + [0] * (0 if t == 9 else 2)
            rng.shuffle(ok)
            assert sum(mask) + n_new <= 8
            fh.write(struct.pack("<i", len(ok)))
            for o in ok:
                fh.write(rng.uniform(30.0, 600.0, 3).astype(np.float32).tobytes() + bytes([o]))


def _f32(h):
    return float(np.array([int(h, 16)], np.uint32).view(np.float32)[0])


def _f64(h):
    return float(np.array([int(h, 16)], np.uint64).view(np.float64)[0])


def _parse_tracks(path):
    """Per frame: dict of the records `vo_host_cli tracks` printed for it."""
    frames = []
    ended = False
    for line in open(path):
        w = line.split()
        k, a = w[0], w[1:]
        if k == "F":
            frames.append(dict(t=int(a[0]), U=[], P=None, T0=None, T1=None, R=[], B=None, W=None, S=None, O={}, E=[]))
            continue
        if k == "END":
            ended = a[0] == "1"
            continue
        fr = frames[-1]
        if k == "U":
            n = int(a[2])
            rows = [(int(a[3 + 4 * i]), _f32(a[4 + 4 * i]), _f32(a[5 + 4 * i]), _f32(a[6 + 4 * i])) for i in range(n)]
            fr["U"].append(dict(kind=int(a[0]), same=int(a[1]), rows=rows))
        elif k == "P":
            npop = int(a[3])
            popped = [int(x) for x in a[4:4 + npop]]
            ndel = int(a[4 + npop])
            fr["P"] = dict(new_first=int(a[0]), g0=int(a[1]), g1=int(a[2]), popped=popped,
                           deleted=[int(x) for x in a[5 + npop:5 + npop + ndel]])
        elif k in ("T0", "T1"):
            n = int(a[1])
            rows = [dict(id=int(a[2 + 7 * i]), first=int(a[3 + 7 * i]), last=int(a[4 + 7 * i]), active=int(a[5 + 7 * i]),
                         X=tuple(_f64(x) for x in a[6 + 7 * i:9 + 7 * i])) for i in range(n)]
            fr[k] = dict(gen=int(a[0]), rows=rows)
        elif k == "R":
            m = int(a[4])
            fr["R"].append(dict(when=int(a[0]), t=int(a[1]), gen=int(a[2]), cur=int(a[3]),
                                pts=[(int(a[5 + 3 * i]), int(a[6 + 3 * i]), int(a[7 + 3 * i])) for i in range(m)]))
        elif k == "B":
            n = int(a[1])
            fid = [int(x) for x in a[2:2 + n]]
            nn = int(a[2 + n])
            fr["B"] = dict(fid=fid, new_ids=[int(x) for x in a[3 + n:3 + n + nn]])
        elif k == "W":
            m = int(a[3])
            fr["W"] = dict(f0=int(a[0]), fits=int(a[1]), gen=int(a[2]),
                           rows=[(int(a[4 + 4 * i]), int(a[5 + 4 * i]), int(a[6 + 4 * i]), _f64(a[7 + 4 * i]))
                                 for i in range(m)])
        elif k == "S":
            n = int(a[0])
            fr["S"] = [tuple(_f32(x) for x in a[1 + 3 * i:4 + 3 * i]) for i in range(n)]
        elif k == "O":
            n = int(a[1])
            fr["O"][int(a[0])] = [(int(a[2 + 5 * i]), tuple(_f32(x) for x in a[3 + 5 * i:7 + 5 * i])) for i in range(n)]
        elif k == "E":
            kind, t, tid = int(a[0]), int(a[1]), int(a[2])
            f = tuple(_f32(x) for x in a[3:7])
            fr["E"].append((("new", "add")[kind], tid, t, f) if kind < 2 else (("pop", "del")[kind - 2], tid))
        else:
            raise AssertionError(line)
    assert ended
    return frames


def _check_resolve(r, rows, seen):
    """One resolve record against the table it was taken on; counts the branch and its cases."""
    ids = [x["id"] for x in rows]
    for wid, j, live in r["pts"]:
        assert 0 <= j < max(len(ids), 1)
        assert (ids[j] == wid) if live else (wid not in ids)
    d = r["cur"] - r["gen"]
    if d == 0:
        seen["resolve_same_gen"] += 1
        assert all(live for _, _, live in r["pts"])
    elif d == 1:
        seen["resolve_next_gen"] += 1
        seen["resolve_next_gen_deleted"] += any(not live for _, _, live in r["pts"])
    else:
        for wid, _, live in r["pts"]:
            if not ids:
                seen["resolve_by_id_empty_table"] += 1
            elif live:
                seen["resolve_by_id_present"] += 1
            elif wid > ids[-1]:
                seen["resolve_by_id_beyond_last"] += 1
            else:
                seen["resolve_by_id_deleted"] += 1


def test_track_table_matches_wba_point(tmp_path):
    """The C++ loop's track table through 12 scripted keyframes of a W = 3 window (at most 8 features each): its
    events replayed through WBA_Point give the table and the observation store after every keyframe; the tracker
    upload, the pops, the BA window's rows and the resolve of earlier windows are checked on the way, and every
    situation the script is there for is counted."""
    from test_pipeline import _replay

    _script(tmp_path / "script.bin")
    _cli("tracks", tmp_path / "script.bin", tmp_path / "out.txt")
    frames = _parse_tracks(tmp_path / "out.txt")
    assert [f["t"] for f in frames] == list(range(N_FRAMES + 1))  # (the last one drains the table)
    seen = dict.fromkeys(["all_continue", "some_lost", "all_lost", "no_new", "pop_deletes_nothing", "pop_first_row",
                          "pop_middle_row", "pop_last_row", "first_bumped", "upload_fast", "upload_search",
                          "resolve_same_gen", "resolve_next_gen", "resolve_next_gen_deleted", "resolve_by_id_present",
                          "resolve_by_id_deleted", "resolve_by_id_beyond_last", "resolve_by_id_empty_table"], 0)
    events, prev = [], None
    for fr in frames:
        t, drain = fr["t"], fr["t"] == N_FRAMES
        # ---- the tracker upload: the rows' features of keyframe t - 1, by ID
        for u in fr["U"]:
            if not u["rows"]:
                continue
            po = dict(prev["O"][t - 1])
            assert [(i, po[i][0], po[i][1], po[i][2]) for i, _, _, _ in u["rows"]] == u["rows"]
            same = [i for i, _, _, _ in u["rows"]] == [i for i, _ in prev["O"][t - 1]]
            assert u["same"] == same and same == (u["kind"] == 0)
            seen["upload_fast" if same else "upload_search"] += 1
        # ---- the pop
        if fr["P"] is not None:
            p, before = fr["P"], prev["T1"]
            bid = [x["id"] for x in before["rows"]]
            assert p["new_first"] == (N_FRAMES + WINDOW if drain else t - WINDOW)
            assert p["popped"] == [f for f in sorted(prev["O"]) if f < p["new_first"]]
            assert p["deleted"] == [x["id"] for x in before["rows"] if x["last"] < p["new_first"]]
            assert p["g0"] == before["gen"] and p["g1"] == p["g0"] + bool(p["deleted"]) == fr["T0"]["gen"]
            kept = [x for x in before["rows"] if x["id"] not in p["deleted"]]
            assert [(x["id"], x["last"], x["X"]) for x in fr["T0"]["rows"]] == [(x["id"], x["last"], x["X"]) for x in kept]
            if not drain:
                seen["pop_deletes_nothing"] += not p["deleted"]
                for i in p["deleted"]:
                    k = bid.index(i)
                    seen["pop_first_row" if k == 0 else "pop_last_row" if k == len(bid) - 1 else "pop_middle_row"] += 1
                seen["first_bumped"] += any(a["first"] in p["popped"] and b["first"] == a["first"] + 1
                                            for a in kept for b in fr["T0"]["rows"] if a["id"] == b["id"])
        # ---- this keyframe booked
        if not drain:
            mask, n_new = _PLAN[t]
            b, rows = fr["B"], fr["T1"]["rows"]
            act = [i for i, _ in prev["O"][t - 1]] if prev else []
            assert len(act) == len(mask)
            kept = [i for i, m in zip(act, mask) if m]
            seen["all_continue"] += bool(act) and len(kept) == len(act)
            seen["some_lost"] += 0 < len(kept) < len(act)
            seen["all_lost"] += bool(act) and not kept
            seen["no_new"] += n_new == 0
            assert b["fid"] == sorted(b["fid"]) == sorted(kept + b["new_ids"]) and len(b["new_ids"]) == n_new
            assert [i for i, _ in fr["O"][t]] == b["fid"]
            assert [x["id"] for x in rows] == sorted(x["id"] for x in rows)
            assert all(x["X"] == (x["id"], x["id"] + 0.25, x["id"] + 0.5) for x in rows)
            assert [x["id"] for x in rows if x["active"]] == b["fid"]
            assert fr["S"] == [(f[0], f[1], f[2]) for _, f in fr["O"][t]]
            # the BA window's rows: the tracks last seen in it, in table order
            w = fr["W"]
            assert w["f0"] == max(0, t - WINDOW + 1) and w["fits"] == 1 and w["gen"] == fr["T1"]["gen"]
            assert w["rows"] == [(k, x["id"], x["id"], float(x["id"])) for k, x in enumerate(rows) if x["last"] >= w["f0"]]
        for r in fr["R"]:
            _check_resolve(r, fr["T0" if r["when"] == 0 else "T1"]["rows"], seen)
        # ---- WBA_Point: the events so far replayed give exactly the table and the store
        events += fr["E"]
        live = _replay(SimpleNamespace(events=events))
        tab = fr["T0"] if drain else fr["T1"]
        assert list(live) == sorted(live) and sorted(live) == [x["id"] for x in tab["rows"]]
        per_track = {x["id"]: [] for x in tab["rows"]}
        for f in sorted(fr["O"]):
            for i, fe in fr["O"][f]:
                per_track[i].append((f, fe))
        for x in tab["rows"]:
            p, got = live[x["id"]], per_track[x["id"]]
            assert [g[0] for g in got] == p.indices
            assert [g[1] for g in got] == [(a[0], a[1], c[0], c[1]) for a, c in p.features]
            assert (x["first"], x["last"]) == (p.indices[0], p.indices[-1])
        prev = fr
    assert not frames[-1]["T0"]["rows"] and not frames[-1]["O"]
    missing = [k for k, v in seen.items() if v == 0]
    assert not missing, (missing, seen)


# ------------------------------------------------------------------------------------------------ arithmetic
def _i64(*v):
    return np.array(v, np.int64).tobytes()


def _f8(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def _f4(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


class _Out:
    def __init__(self, path):
        self.buf, self.pos = open(path, "rb").read(), 0

    def take(self, dtype, n):
        a = np.frombuffer(self.buf, dtype, n, self.pos)
        self.pos += a.nbytes
        return a


def _rel(a, b):
    """Largest difference of a from b relative to b's largest magnitude (a matrix or a vector as one quantity)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _vo(cfg, K, first_pose=None, velocity=None):
    """A WindowedStereoVO for its host helpers only (no backend call is made)."""
    return PL.WindowedStereoVO(cfg, PL.Backend(), K, first_pose, velocity)


@pytest.fixture(scope="module")
def maths(tmp_path_factory):
    """Seeded inputs with the edge values the code branches on, through `vo_host_cli math` once."""
    d = tmp_path_factory.mktemp("vo_math")
    rng = np.random.default_rng(7)
    m = SimpleNamespace()
    ax = rng.normal(size=(40, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.concatenate([[0.0, 1e-13, 1e-3, np.pi - 1e-9, np.pi, 3.0], rng.uniform(0.0, np.pi, 34)])
    m.aa = ax * ang[:, None]
    m.aa[0] = 0.0
    m.X = rng.uniform(-20.0, 20.0, (40, 3)) + np.array([0.0, 0.0, 25.0])
    m.poses = np.concatenate([rng.uniform(-2.0, 2.0, (40, 3)), m.aa * 0.05], 1)
    m.poses2 = m.poses + rng.normal(scale=1e-3, size=(40, 6))
    m.cells = [(t, c) for t in (0, 1, 7, 1000) for c in (0, 1, 2, 63, 1999, 123456)]
    m.grids = [(640, 480, 500), (1280, 720, 2000), (320, 240, 7), (96, 96, 1), (200, 120, 37), (400, 300, 50)]
    m.cam = (576.0, 319.5, 241.25, 0.5)
    m.w, m.h = 640, 480
    # new cells: more good features than n_feats, fewer, none; on a grid where n_feats is no multiple of nx
    m.nc_cases = []
    for t, (w, h, nf), ng in [(0, (200, 120, 37), 0), (3, (200, 120, 37), 12), (5, (200, 120, 37), 60),
                              (9, (640, 480, 500), 300)]:
        uv = np.stack([rng.uniform(0.0, w, ng), rng.uniform(0.0, h, ng)], -1).astype(np.float32)
        m.nc_cases.append((t, w, h, nf, uv))
    e = float(PL.MARGIN)
    m.uv_margin = np.array([[e, e], [np.nextafter(np.float32(e), np.float32(0)), e], [m.w - e, 100], [m.w - e - 0.5, 100],
                            [100, m.h - e], [100, np.nextafter(np.float32(m.h - e), np.float32(0))], [np.nan, 100],
                            [300.25, 200.5]], np.float32)
    # pose prediction: t = 0 and 1 with and without a velocity, constant velocity, a missing t - 2 pose
    p = {k: m.poses[k] for k in range(8)}
    m.pp_cases = [(0, False, {}), (0, True, {}), (1, False, {0: p[0]}), (1, True, {0: p[0]}),
                  (2, False, {0: p[0], 1: p[1]}), (2, True, {0: p[0], 1: p[1]}), (5, False, {3: p[3], 4: p[4]}),
                  (5, True, {4: p[4]}), (5, False, {4: p[4]}), (7, True, {2: p[2], 6: p[6]})]
    m.first, m.vel = m.poses[10], m.poses[11] * 0.1
    m.d_pred = np.concatenate([[np.nan, np.inf, -np.inf, 1e9, 1.0000001e9, 1e12, 0.0, -3.0, 0.49, 0.5, 1.5, 2.5,
                                7.999, 8.0, 130.0, 134.5, 1e-300], rng.uniform(0.0, 140.0, 30)])
    m.d_min, m.d_max = 2, 128
    # landmarks seen from pose 3, the first four behind the camera (Z <= 0), one of them only just
    m.pose = m.poses[3]
    R = S.aa_to_R(m.pose[3:])
    m.Xw = m.X.copy()
    m.Xw[:4] = (np.array([[1.0, 2.0, -5.0], [0.0, 0.0, -0.1], [3.0, -1.0, -40.0], [0.5, 0.5, -1e-6]]) - m.pose[:3]) @ R
    m.feats = np.stack([rng.uniform(30, 600, 40), rng.uniform(30, 440, 40), np.zeros(40)], -1).astype(np.float32)
    m.feats[:, 2] = m.feats[:, 0] - rng.uniform(2.0, 128.0, 40).astype(np.float32)
    with open(d / "in.bin", "wb") as fh:
        fh.write(_i64(1, len(m.aa)) + _f8(m.aa))
        fh.write(_i64(2, 40))
        for k in range(40):
            fh.write(_f8(m.X[k]) + _f8(S.aa_to_R(m.poses[k, 3:])) + _f8(m.poses[k]) + _f8(m.poses2[k])
                     + _f8(PL.rot_series(m.poses2[k, 3:])))
        fh.write(_i64(3, len(m.cells)) + b"".join(_i64(t, c) for t, c in m.cells))
        fh.write(_i64(4, len(m.grids)) + b"".join(_i64(*g) for g in m.grids))
        for t, w, h, nf, uv in m.nc_cases:
            fh.write(_i64(5, t, w, h, nf, len(uv)) + _f4(uv))
        fh.write(_i64(6, m.w, m.h, len(m.uv_margin)) + _f4(m.uv_margin))
        for t, hv, ps in m.pp_cases:
            fh.write(_i64(7, t, int(hv), len(ps)) + _f8(m.first) + _f8(m.vel)
                     + b"".join(_i64(k) + _f8(v) for k, v in ps.items()))
        fh.write(_i64(8, m.d_min, m.d_max, len(m.d_pred)) + _f8(m.d_pred))
        fh.write(_i64(9) + _f8(m.cam) + _f8(m.pose) + _i64(len(m.feats)) + _f4(m.feats))
        fh.write(_i64(10) + _f8(m.cam) + _f8(m.pose) + _i64(len(m.Xw)) + _f8(m.Xw))
    _cli("math", d / "in.bin", d / "out.bin")
    o = _Out(d / "out.bin")
    rr = o.take(np.float64, 18 * len(m.aa)).reshape(-1, 2, 9)
    m.rot_series, m.aa_to_R = rr[:, 0], rr[:, 1]
    m.moved = o.take(np.float64, 3 * 40).reshape(-1, 3)
    m.jitter = o.take(np.float64, 2 * len(m.cells)).reshape(-1, 2)
    m.grid_out = [(tuple(o.take(np.int64, 2)), tuple(o.take(np.float64, 2))) for _ in m.grids]
    m.new_cells = []
    for _ in m.nc_cases:
        n = int(o.take(np.int64, 1)[0])
        m.new_cells.append(o.take(np.float32, 2 * n).reshape(-1, 2))
    m.in_margin = o.take(np.uint8, len(m.uv_margin))
    m.predicted = [o.take(np.float64, 6) for _ in m.pp_cases]
    m.lo = o.take(np.int32, len(m.d_pred))
    m.dvalid = o.take(np.uint8, len(m.d_pred))
    m.tri = o.take(np.float64, 3 * len(m.feats)).reshape(-1, 3)
    m.guess = o.take(np.float32, 2 * len(m.Xw)).reshape(-1, 2)
    m.disp = o.take(np.float64, len(m.Xw))
    assert o.pos == len(o.buf)
    return m


def test_rotation_series_and_landmark_move_bit_equal(maths):
    m = maths
    for k, aa in enumerate(m.aa):
        assert _bits_equal(m.rot_series[k], PL.rot_series(aa).ravel()), k
    for k in range(40):
        R, R2 = S.aa_to_R(m.poses[k, 3:]), PL.rot_series(m.poses2[k, 3:])
        ref = PL.move_landmarks(m.X[k:k + 1], R, m.poses[k], m.poses2[k], R2)[0]
        assert _bits_equal(m.moved[k], ref), k


def test_grid_jitter_new_cells_margin_bit_equal(maths):
    m = maths
    for k, (t, c) in enumerate(m.cells):
        assert _bits_equal(m.jitter[k], PL._cell_jitter(t, np.array([c]))[0]), (t, c)
    K = np.array([[576.0, 0, 319.5], [0, 576.0, 241.25], [0, 0, 1.0]])
    odd = 0
    for (w, h, nf), ((nx, ny), (cw, ch)) in zip(m.grids, m.grid_out):
        vo = _vo(PL.PipelineConfig(w, h, nf, 3), K)
        assert (int(nx), int(ny)) == (vo.nx, vo.ny) and _bits_equal(np.array([cw, ch]), np.array([vo.cw, vo.ch]))
        odd += nf % vo.nx != 0
    assert odd > 0  # (a grid where n_feats is no multiple of nx)
    more = 0
    for (t, w, h, nf, uv), got in zip(m.nc_cases, m.new_cells):
        vo = _vo(PL.PipelineConfig(w, h, nf, 3), K)
        ref = PL.new_cells(t, uv, (vo.nx, vo.ny, vo.cw, vo.ch, nf))
        assert _bits_equal(got, ref.reshape(-1, 2)), (t, nf, len(uv))
        more += len(uv) > nf and len(got) == 0
    assert more > 0  # (more good features than n_feats: no new cell)
    ref = PL.in_margin(m.uv_margin, m.w, m.h)
    assert _bits_equal(m.in_margin.astype(bool), ref) and ref.any() and not ref.all()


def test_pose_prediction_and_search_window_bit_equal(maths):
    m = maths
    K = np.array([[576.0, 0, 319.5], [0, 576.0, 241.25], [0, 0, 1.0]])
    cfg = PL.PipelineConfig(m.w, m.h, 100, 3, d_min=m.d_min, d_max=m.d_max)
    for (t, hv, ps), got in zip(m.pp_cases, m.predicted):
        vo = _vo(cfg, K, m.first, m.vel if hv else None)
        vo.poses = dict(ps)
        assert _bits_equal(got, vo._predict_pose(t)), (t, hv, sorted(ps))
    lo, nd, dvalid = _vo(cfg, K).search_window(m.d_pred)
    assert nd == 13 and _bits_equal(m.lo.astype(np.int64), lo) and _bits_equal(m.dvalid.astype(bool), dvalid)
    assert not np.isfinite(m.d_pred[:3]).any() and (m.d_pred[3:6] >= 1e9).all()  # (the edge values are in)
    assert lo.min() == m.d_min and lo.max() == m.d_max and not dvalid.all()


def test_library_arithmetic_within_rounding(maths):
    """aa_to_R, triangulate, the klt_predict guess and the predicted disparity go through sin / cos or a matrix
    product, from two libraries: equal to rounding.  Each bound is eight times the largest relative difference
    measured over these inputs (relative to the quantity's largest component), which leaves room for another libm;
    anything above 1e-12 would be more than rounding."""
    m = maths
    K = np.array([[m.cam[0], 0, m.cam[1]], [0, m.cam[0], m.cam[2]], [0, 0, 1.0]])
    cfg = PL.PipelineConfig(m.w, m.h, 100, 3, baseline=m.cam[3])
    vo = _vo(cfg, K)
    d = {}
    d["aa_to_R"] = max(_rel(m.aa_to_R[k], S.aa_to_R(aa).ravel()) for k, aa in enumerate(m.aa))
    ref = vo._triangulate(m.feats[:, :2], m.feats[:, 2], m.pose)
    d["triangulate"] = max(_rel(a, b) for a, b in zip(m.tri, ref))
    ref = PL.predict_uv(m.Xw, m.pose, *m.cam[:3])
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(m.guess), nan) and nan[:4].all() and not nan[4:].any()  # (Z <= 0: NaN)
    d["guess"] = max(_rel(a, b) for a, b in zip(m.guess[4:], ref[4:]))
    vo.X = m.Xw
    ref = vo._predicted_disparity(np.arange(len(m.Xw)), m.pose)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(m.disp), nan) and nan[:4].all() and not nan[4:].any()
    d["disparity"] = max(_rel(a, b) for a, b in zip(m.disp[4:], ref[4:]))
    print("largest relative differences:", {k: "%.3g" % v for k, v in d.items()})
    assert all(v <= 1e-12 for v in d.values()), d
    assert d["aa_to_R"] <= 8 * 9.07e-16      # measured 9.07e-16
    assert d["triangulate"] <= 8 * 2.07e-16  # measured 2.07e-16
    assert d["guess"] <= 8 * 0.0             # measured 0: the float32 pixels are the same bits
    assert d["disparity"] <= 8 * 3.58e-16    # measured 3.58e-16
