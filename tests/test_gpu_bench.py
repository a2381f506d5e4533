"""bench.py as a program: the plain run's result line and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from oracle import stgcn as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the IK path's pose tolerance (test_gpu_ik.py)


def test_bench_plain_run_dumps_last_step(tmp_path, ik_weights):
    """A plain run (no --full) times exactly --steps steps, prints one JSON line
    with the headline fields and no roofline / baseline extras, and
    --dump-outputs writes the poses of the last timed step: float32, and the
    CPU oracle's poses for the benchmark's seeded windows (the same in every
    run) within the IK tolerance."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    B, T = 5, 64
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--T", str(T), "--dump-outputs", str(tmp_path / "out")],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1, out
    r = json.loads(out[0])
    assert r["metric"] == "IK frames/sec (COCO-17->SMPLx pose)" and r["unit"] == "IK frames/s"
    assert r["higher_is_better"] is True and r["steps"] == 3 and r["warmup"] == 1
    assert r["dtype"].startswith("f32 via bf16x3")
    assert r["ms_per_step"] > 0 and abs(r["value"] - B / (r["ms_per_step"] * 1e-3)) <= 0.01 * r["value"]
    assert not {"roofline", "forward", "other_precisions", "fk", "online", "cpu_baseline"} & set(r)
    assert os.listdir(tmp_path / "out") == ["poses.npy"]
    y = np.load(tmp_path / "out" / "poses.npy")
    assert y.dtype == np.float32 and y.shape == (B, r["config"]["out_frames"], 66)
    ref = orc.pose_regressor(syn.synthetic_windows(B, T, seed=0), ik_weights)["poses"]
    assert np.abs(y - ref).max() < TOL
