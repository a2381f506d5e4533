"""Child program of tests/test_gpu_guards.py (not a test module).

TIK_GUARD is latched on first use, so guard mode needs a process of its own:
started with TIK_GUARD=1, this runs the workloads of tests/memedge.py, family
by family, on buffers that carry 1 MiB guard zones, calls
tik_debug_check_guards() after each family and prints one JSON line
{"family", "bad", "report"} (bad = guard zones found written). On any error
it prints {"family", "error"} and exits non-zero at once: nothing further is
started on the GPU.
"""
import gc
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import memedge as me   # noqa: E402

GUARD_SHAPE = (9, 64)   # nine windows of the bench length: each workgroup walks a whole tile


def families():
    """(name, callable) in run order; tests/test_gpu_guards.py lists the same names."""
    out = []
    for c in me.IK_CONFIGS:
        shapes = me.ik_shapes(c) if c == "split" else me.SHAPES + [GUARD_SHAPE]
        # exactly sized first (a guard right behind the last row), then on the reserved workspace
        out.append((f"ik:{c}", lambda c=c, s=shapes: (me.ik_reference(c, s), me.ik_family(c, s))))
    out.append(("block", lambda: (me.block_family(fresh=True), me.block_family())))
    out.append(("gconv", me.gconv_family))
    for c in me.FK_CONFIGS:
        out.append((f"fk:{c}", lambda c=c: (me.fk_family(c, reserve=None), me.fk_family(c))))
    out.append(("trainer", me.trainer_family))
    for win, online in me.STREAM_CASES:
        out.append((f"stream:{win}:{online}", lambda w=win, o=online: me.stream_family(w, o)))
    return out


FAMILY_NAMES = [f"ik:{c}" for c in me.IK_CONFIGS] + ["block", "gconv"] + [f"fk:{c}" for c in me.FK_CONFIGS] + \
    ["trainer"] + [f"stream:{w}:{o}" for w, o in me.STREAM_CASES]


def main():
    if os.environ.get("TIK_GUARD") != "1":
        print(json.dumps({"family": "-", "error": "start this program with TIK_GUARD=1"}), flush=True)
        return 2
    import torch
    from temporal_inverse_kinematics_amd import _lib
    lib = me.lib()
    found = {"bad": 0, "report": "", "checks": 0}

    def check():   # memedge calls this while a handle is alive and its work is done
        n = _lib.check(lib.tik_debug_check_guards(), "tik_debug_check_guards")
        found["checks"] += 1
        if n:
            found["bad"] += n
            found["report"] += _lib.last_error()[:1000]

    me.ON_RELEASE = check
    for name, fn in families():
        t0 = time.time()
        found.update(bad=0, report="", checks=0)
        try:
            res = fn()
            torch.cuda.synchronize()
            del res
            gc.collect()
            assert found["checks"] > 0, "no guard check ran"
        except Exception:   # a HIP error included: stop here
            print(json.dumps({"family": name, "error": traceback.format_exc()[-2000:]}), flush=True)
            return 1
        print(json.dumps({"family": name, "bad": found["bad"], "report": found["report"][:4000],
                          "checks": found["checks"], "seconds": round(time.time() - t0, 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
