"""Out-of-bounds stores into the library's own buffers (TIK_GUARD=1).

With TIK_GUARD=1 every dev_alloc carries 1 MiB of 0xA5 on both sides and
tik_debug_check_guards() counts the guard zones that were written. The
switch is latched on first use, so tests/guard_child.py runs in a fresh child
process, once per module: every IK path configuration at the tile-edge shapes
of tests/memedge.py plus (9,64), on handles sized exactly for each call and
on one reserved workspace; the block API, gconv, the FK configurations, the
trainer and the online stream. It reports one JSON line per family; the
cases below read that one report. A family whose guards were written fails
with the checker's description of the buffer and the byte range.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = (["ik:default", "ik:xblk0", "ik:xgw0", "ik:xtws0", "ik:xtws255", "ik:xfg0", "ik:xchunk3", "ik:fp32",
             "ik:split", "block", "gconv", "fk:sparse", "fk:dense", "fk:chunk2", "fk:fp32", "trainer",
             "stream:9:1", "stream:64:1", "stream:9:0", "stream:64:0"])


@pytest.fixture(scope="module")
def report():
    """One run of the child (a fresh process, never exec; a failed run is cached like a good one)."""
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    env = dict(os.environ)
    env.pop("TIK_POISON", None)
    env["TIK_GUARD"] = "1"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "guard_child.py")], env=env, capture_output=True,
                           text=True, timeout=600)
        rc, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        dec = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
        rc, out, err = "timeout", dec(e.stdout), dec(e.stderr)
    lines = {}
    for ln in out.splitlines():
        if ln.startswith("{"):
            d = json.loads(ln)
            lines[d["family"]] = d
    return {"rc": rc, "families": lines, "stderr": err[-3000:]}


def test_child_lists_these_families():
    import guard_child
    assert guard_child.FAMILY_NAMES == FAMILIES
    assert [n for n, _ in guard_child.families()] == FAMILIES


@pytest.mark.parametrize("family", FAMILIES)
def test_no_guard_zone_written(report, family):
    errors = {k: v["error"] for k, v in report["families"].items() if "error" in v}
    assert report["rc"] == 0, (report["rc"], errors, report["stderr"])
    assert family in report["families"], sorted(report["families"])
    r = report["families"][family]
    assert r["checks"] > 0
    assert r["bad"] == 0, r["report"]
