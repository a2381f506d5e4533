"""Guard zones around every device buffer while tik_fk_pose_metrics (with and without rows, target_poses and
joints_out) and a validation step with val_metrics run (tests/pose_metrics_guard_child.py, a fresh process with
TIK_GUARD=1 and a NaN fill): no guard zone may be written, no poison may reach an output."""
import json
import os
import subprocess
import sys

import pytest

import memedge as me

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_guard_zone_written_and_no_poison_read():
    import pose_metrics_guard_child as child
    me.lib()
    env = dict(os.environ)
    env.update(TIK_GUARD="1", TIK_POISON="ff")
    p = subprocess.run([sys.executable, os.path.join(HERE, "pose_metrics_guard_child.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = {d["family"]: d for d in (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))}
    assert p.returncode == 0, (p.returncode, lines, p.stderr[-3000:])
    assert sorted(lines) == sorted(child.FAMILY_NAMES)
    for name, r in lines.items():
        assert r["checks"] > 0 and r["bad"] == 0 and r["nan"] == 0, (name, r)
