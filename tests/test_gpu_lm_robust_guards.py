"""Guard zones around every device buffer while tik_fk_refine_robust (robust term and missing rule on) and an online
stream with confidences per push run (tests/lm_robust_guard_child.py, a fresh process with TIK_GUARD=1 and a NaN fill):
no guard zone may be written, no poison may reach an output."""
import json
import os
import subprocess
import sys

import pytest

import memedge as me

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_guard_zone_written_and_no_poison_read():
    import lm_robust_guard_child as child
    me.lib()
    env = dict(os.environ)
    env.update(TIK_GUARD="1", TIK_POISON="ff")
    p = subprocess.run([sys.executable, os.path.join(HERE, "lm_robust_guard_child.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = {d["family"]: d for d in (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))}
    assert p.returncode == 0, (p.returncode, lines, p.stderr[-3000:])
    assert sorted(lines) == sorted(child.FAMILY_NAMES)
    for name, r in lines.items():
        assert r["checks"] > 0 and r["bad"] == 0 and r["nan"] == 0, (name, r)
