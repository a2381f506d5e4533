"""Child program of tests/test_gpu_fk_shape_jacobian.py (not a test module),
modelled on tests/fk_jacobian_guard_child.py: started with TIK_GUARD=1 (latched
on first use, hence a process of its own) and TIK_POISON=ff, it runs the shape
Jacobian, the summed normal equations and their solve on buffers that carry
1 MiB guard zones and a NaN fill, calls tik_debug_check_guards() while each
handle is alive and prints one JSON line {"family", "bad", "report", "checks",
"nan"} per configuration. On any error it prints {"family", "error"} and exits
non-zero at once: nothing further is started on the GPU.
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

CONFIGS = ("sparse", "dense")   # the nzw pairs / the dense WT rows (TIK_FK_SKIN)
FAMILY_NAMES = [f"fk_shape_jacobian:{c}" for c in CONFIGS]
BATCHES = (1, 37, 65)


def family(config, found):
    import torch
    import fk_jacobian_ref as R
    import fk_shape_ref as S
    with me.env(TIK_FK_SKIN=config):
        m = S.SMPLX(R.small_consts(), batch_size=9)
    nan = 0
    sel = R.COCO + [55 + 21 + 7]
    for B in BATCHES:   # ascending then descending: stale rows of the larger call behind the smaller
        for n in (B, 1):
            args = [torch.from_numpy(a[:n]).cuda() for a in me.fk_inputs(B)]
            for with_joints in (True, False):
                jac, joints = m.joints_shape_jacobian(*args, select=sel, return_joints=with_joints)
                r = (joints if with_joints else m.joints(*args, select=sel)).reshape(n, -1).contiguous()
                partial = S.lm_accumulate(jac, r)
                delta = S.lm_solve_sum(partial, mu=0.1, lam=0.5, prior=torch.ones(jac.shape[2], device="cuda"))
                torch.cuda.synchronize()
                nan += int(torch.isnan(jac).sum()) + int(torch.isnan(r).sum()) + int(torch.isnan(partial).sum())
                nan += int(torch.isnan(delta).sum())
    me.release(m)
    found["nan"] = nan


def main():
    if os.environ.get("TIK_GUARD") != "1":
        print(json.dumps({"family": "-", "error": "start this program with TIK_GUARD=1"}), flush=True)
        return 2
    import torch
    from temporal_inverse_kinematics_amd import _lib
    lib = me.lib()
    found = {"bad": 0, "report": "", "checks": 0, "nan": 0}

    def check():   # memedge.release calls this while the handle is alive and its work is done
        n = _lib.check(lib.tik_debug_check_guards(), "tik_debug_check_guards")
        found["checks"] += 1
        if n:
            found["bad"] += n
            found["report"] += _lib.last_error()[:1000]

    me.ON_RELEASE = check
    for name, c in zip(FAMILY_NAMES, CONFIGS):
        found.update(bad=0, report="", checks=0, nan=0)
        try:
            family(c, found)
            torch.cuda.synchronize()
            gc.collect()
            assert found["checks"] > 0, "no guard check ran"
        except Exception:   # a HIP error included: stop here
            print(json.dumps({"family": name, "error": traceback.format_exc()[-2000:]}), flush=True)
            return 1
        print(json.dumps({"family": name, "bad": found["bad"], "report": found["report"][:4000],
                          "checks": found["checks"], "nan": found["nan"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
