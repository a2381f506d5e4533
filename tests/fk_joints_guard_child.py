"""Child program of tests/test_gpu_fk_joints.py (not a test module), modelled on
tests/guard_child.py: started with TIK_GUARD=1 (latched on first use, hence a
process of its own), it runs the mesh-free joints workload of
tests/fk_joints_edges.py on buffers that carry 1 MiB guard zones, exactly
sized and on a reserved handle, calls tik_debug_check_guards() while each
handle is alive and prints one JSON line {"family", "bad", "report",
"checks"} per configuration. On any error it prints {"family", "error"} and
exits non-zero at once: nothing further is started on the GPU.
"""
import gc
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import memedge as me            # noqa: E402
import fk_joints_edges as fje   # noqa: E402

FAMILY_NAMES = [f"fk_joints:{c}" for c in fje.CONFIGS]


def main():
    if os.environ.get("TIK_GUARD") != "1":
        print(json.dumps({"family": "-", "error": "start this program with TIK_GUARD=1"}), flush=True)
        return 2
    import torch
    from temporal_inverse_kinematics_amd import _lib
    lib = me.lib()
    found = {"bad": 0, "report": "", "checks": 0}

    def check():   # memedge.release calls this while the handle is alive and its work is done
        n = _lib.check(lib.tik_debug_check_guards(), "tik_debug_check_guards")
        found["checks"] += 1
        if n:
            found["bad"] += n
            found["report"] += _lib.last_error()[:1000]

    me.ON_RELEASE = check
    for name, c in zip(FAMILY_NAMES, fje.CONFIGS):
        found.update(bad=0, report="", checks=0)
        try:
            res = (fje.joints_family(c, reserve=None), fje.joints_family(c))
            torch.cuda.synchronize()
            del res
            gc.collect()
            assert found["checks"] > 0, "no guard check ran"
        except Exception:   # a HIP error included: stop here
            print(json.dumps({"family": name, "error": traceback.format_exc()[-2000:]}), flush=True)
            return 1
        print(json.dumps({"family": name, "bad": found["bad"], "report": found["report"][:4000],
                          "checks": found["checks"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
