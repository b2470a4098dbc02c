"""bench.py's command line: the plain run (headline fields only), --dump-outputs and the option checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_options():
    """--full and --dump-outputs exist; --steps sets the timed steps, so it cannot be 0."""
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_outputs(tmp_path, oracle):
    """A plain run prints the headline fields and none of the --full measurements; its dump holds
    float arrays for the two replayed frames, and the last step's frame meets the oracle at the bench's
    parity bars (KLT bit-exact, scale 1e-9 relative, BA 1e-6 relative)."""
    import bench
    from uasl_motion_estimation_amd import synthetic as S

    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "2",
                        "--dump-outputs", d], capture_output=True, text=True, timeout=110, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["value"] > 0 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert abs(line["ms_per_step"] * line["value"] - 1e3) <= 1.0  # one frame per step on one GPU
    for k in ("roofline", "cpu_baseline", "parity", "pipeline", "sharded_ba", "multi_stream", "mi_roofline"):
        assert k not in line, k
    names = ("klt_pts", "klt_status", "scale", "ba_cams", "ba_pts")
    assert sorted(os.listdir(d)) == sorted(f"frame{k}_{n}.npy" for k in (0, 1) for n in names)
    dump = [{n: np.load(os.path.join(d, f"frame{k}_{n}.npy")) for n in names} for k in (0, 1)]
    assert all(a.dtype in (np.float32, np.float64) for g in dump for a in g.values())
    assert sum(a.nbytes for g in dump for a in g.values()) <= 64 << 20

    frames = bench.make_frames(S.CONFIGS[3], S.SEED0 + 3, 2)  # the run's inputs: a function of its arguments
    g, fd = dump[0], frames[0]  # the last timed step's frame: (3 - 1) % 2
    o = bench.cpu_frame(bench.cpu_payload(fd), 10, 10)
    got = dict(klt=g["klt_pts"], klt_status=g["klt_status"].astype(np.uint8),
               scale=dict(scale=g["scale"][0], iterations=int(g["scale"][1]), stop=int(g["scale"][2])),
               cams=g["ba_cams"], pts=g["ba_pts"],
               ba=dict(iterations=o["ba"]["iterations"], successful_steps=o["ba"]["successful_steps"]))
    c = bench.compare(got, o)
    assert c["klt_bit_exact"] and c["scale_match"] and c["ba_match"], c
