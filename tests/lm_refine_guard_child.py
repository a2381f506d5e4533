"""Child program of tests/test_gpu_lm_refine_guards.py (not a test module), in the pattern of
tests/fk_jacobian_guard_child.py: started with TIK_GUARD=1 (latched on first use, hence a process of its own)
and TIK_POISON=ff, it runs tik_fk_refine at B = 1, 3, 37 on both skinning table forms and a refining online
stream at win 9 on both paths, on buffers that carry 1 MiB guard zones and a NaN fill, calls
tik_debug_check_guards() while each handle is alive and prints one JSON line {"family", "bad", "report",
"checks", "nan"} per configuration. On any error it prints {"family", "error"} and exits non-zero at once:
nothing further is started on the GPU.
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

FAMILIES = [("lm_refine", "sparse"), ("lm_refine", "dense"), ("stream_refine", "1"), ("stream_refine", "0")]
FAMILY_NAMES = [f"{k}:{c}" for k, c in FAMILIES]
BATCHES = (1, 3, 37)


def refine_family(skin, found):
    import numpy as np
    import torch
    import lm_refine_ref as L
    with me.env(TIK_FK_SKIN=skin):
        m = L.R.SMPLX(L.consts(), batch_size=9)
    nan = 0
    rng = np.random.default_rng(7)
    for B in BATCHES:
        th = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 66)).astype(np.float32)).cuda()
        kps = torch.from_numpy(rng.normal(0, 0.3, (B, 17, 3)).astype(np.float32)).cuda()
        betas = torch.from_numpy(rng.normal(0, 1, (B, 10)).astype(np.float32)).cuda()
        w = torch.ones(B, 17, device="cuda")
        for kw in (dict(), dict(betas=betas, prior=th.clone(), prev=th.clone(), smooth=0.1, joint_weight=w, debug=True),
                   dict(iters=0)):
            out = m.refine_frames(th, kps, **{"iters": 2, **kw})
            torch.cuda.synchronize()
            nan += sum(int(torch.isnan(t).sum()) for t in out)
    me.release(m)
    found["nan"] = nan


def stream_family(online, found):
    import numpy as np
    import lm_refine_ref as L
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    seq = me.golden("run_inference.npz")["seq"][:14]
    body = L.R.SMPLX(L.consts(), batch_size=9)
    nan = 0
    with me.env(TIK_ONLINE=online):
        m = synthetic_model(win_size=9, device="cuda")
        for graph in (True, False):
            s = OnlineIK(m, use_graph=graph, refine=2, smplx_model=body, smooth_weight=0.1, betas=np.zeros(10, np.float32),
                         joint_weight=np.ones(17, np.float32))
            out = s.run(seq)                       # the first h pushes and the flush included
            nan += int(np.isnan(out).sum()) + int(np.isnan(s.raw).sum())
            me.release(s, m, body)
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
    for name, (kind, c) in zip(FAMILY_NAMES, FAMILIES):
        found.update(bad=0, report="", checks=0, nan=0)
        try:
            (refine_family if kind == "lm_refine" else stream_family)(c, found)
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
