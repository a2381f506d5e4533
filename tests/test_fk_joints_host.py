"""Host side of the mesh-free joints path: the selection resolver and the
bench's command line (no GPU, no library call)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden


def test_coco_selection_is_the_golden_map():
    from temporal_inverse_kinematics_amd.smplx_fk import resolve_select
    want = [int(v) for v in golden("keypoints.npz")["smplx_to_coco"]]
    assert resolve_select("coco", 144) == want
    assert resolve_select(None, 144) is None
    assert resolve_select(np.array([3, 3, 143]), 144) == [3, 3, 143]
    assert resolve_select(range(144), 144) == list(range(144))


@pytest.mark.parametrize("sel", [[-1], [144], [0, 200], list(range(144)) + list(range(113)), [], "body25"])
def test_selection_validator_rejects(sel, monkeypatch):
    from temporal_inverse_kinematics_amd import _lib, smplx_fk

    def no_library(*a, **k):
        raise AssertionError("the validator must not touch the library")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError):
        smplx_fk.resolve_select(sel, 144)
    assert len(smplx_fk.resolve_select([0] * 256, 144)) == 256


def test_bench_fk_help_lists_joints():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench_fk.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--joints" in p.stdout and "coco" in p.stdout
    src = open(os.path.join(REPO, "bench_fk.py")).read()
    head = src[:src.index("def measure_fk")]
    assert "import torch" not in head and "temporal_inverse_kinematics_amd" not in head.split('"""')[2]
