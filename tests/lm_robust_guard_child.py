"""Child program of tests/test_gpu_lm_robust_guards.py (not a test module), in the pattern of
tests/lm_refine_guard_child.py: started with TIK_GUARD=1 (latched on first use, hence a process of its own) and
TIK_POISON=ff, it runs tik_fk_refine_robust with the robust term and the missing rule on (debug outputs included) at
B = 1, 3, 37 on both skinning table forms, and an online stream that refines with confidences per push at win 9 on both
paths, on buffers that carry 1 MiB guard zones and a NaN fill, calls tik_debug_check_guards() while each handle is alive
and prints one JSON line {"family", "bad", "report", "checks", "nan"} per configuration. On any error it prints
{"family", "error"} and exits non-zero at once: nothing further is started on the GPU.
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

FAMILIES = [("lm_robust", "sparse"), ("lm_robust", "dense"), ("stream_conf", "1"), ("stream_conf", "0")]
FAMILY_NAMES = [f"{k}:{c}" for k, c in FAMILIES]
BATCHES = (1, 3, 37)


def robust_family(skin, found):
    import numpy as np
    import torch
    import lm_robust_ref as RR
    L = RR.L
    with me.env(TIK_FK_SKIN=skin):
        m = L.R.SMPLX(L.consts(), batch_size=9)
    nan = 0
    rng = np.random.default_rng(7)
    for B in BATCHES:
        th = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 66)).astype(np.float32)).cuda()
        k = rng.normal(0, 0.3, (B, 17, 3)).astype(np.float32)
        k[0, 9] = np.nan                     # a missing keypoint in the first frame
        k[B - 1, 12, 2] = np.inf             # a missing hip in the last (the same frame at B = 1)
        kps = torch.from_numpy(k).cuda()
        betas = torch.from_numpy(rng.normal(0, 1, (B, 10)).astype(np.float32)).cuda()
        w = torch.ones(B, 17, device="cuda")
        on = dict(robust_sigma=RR.SIGMA, skip_nonfinite=True)
        for kw in (on, dict(betas=betas, prior=th.clone(), prev=th.clone(), smooth=0.1, joint_weight=w, debug=True, **on),
                   dict(iters=0, debug=True, **on)):
            out = m.refine_frames(th, kps, **{"iters": 2, **kw})
            torch.cuda.synchronize()
            # dbg_r holds the residual against the cleaned target: finite too
            nan += sum(int(torch.isnan(t).sum()) for t in out)
    me.release(m)
    found["nan"] = nan


def stream_family(online, found):
    import numpy as np
    import lm_robust_ref as RR
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    L = RR.L
    seq = np.array(me.golden("run_inference.npz")["seq"][:14], np.float32)
    conf = np.ones((14, 17), np.float32)
    seq[3:5, 9], conf[3:5, 9] = np.nan, 0
    conf[6, 11] = 0
    seq[8], conf[8] = np.nan, 0
    conf[10, 2] = 0.5
    body = L.R.SMPLX(L.consts(), batch_size=9)
    nan = 0
    with me.env(TIK_ONLINE=online):
        m = synthetic_model(win_size=9, device="cuda")
        for graph in (True, False):
            s = OnlineIK(m, use_graph=graph, refine=2, smplx_model=body, smooth_weight=0.1, betas=np.zeros(10, np.float32),
                         joint_weight=np.ones(17, np.float32), robust_sigma=RR.SIGMA)
            out = s.run(seq, conf)                 # the first h pushes and the flush included
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
            (robust_family if kind == "lm_robust" else stream_family)(c, found)
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
