"""Child program of tests/test_gpu_train_kp.py (not a test module), in the pattern of
tests/lm_refine_guard_child.py: started with TIK_GUARD=1 (latched on first use, hence a process of its own) and
TIK_POISON=ff, it runs one training step with the keypoint term at (N,T) = (5,1) and one at (2,3), each with two
body models, on buffers that carry 1 MiB guard zones and a NaN fill, calls tik_debug_check_guards() while the
handles are alive and prints one JSON line {"family", "bad", "report", "checks", "nan"} per shape: nan counts the
NaNs in the loss, its two parts and every parameter gradient. On any error it prints {"family", "error"} and exits
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

SHAPES = [(5, 1, 31, [0, 0, 1, 0, 1]), (2, 3, 33, [1, 0])]
FAMILY_NAMES = [f"kp_step:{N}x{T}" for N, T, _, _ in SHAPES]


def step_family(N, T, seed, gid, found):
    import numpy as np
    import torch
    import kp_loss_ref as K
    import trainref as tref
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    c1 = dict(K.consts())
    c1["v_template"] = np.ascontiguousarray(c1["v_template"] * np.float32(1.1))
    bodies = {"a": K.R.SMPLX(K.consts(), batch_size=9), "b": K.R.SMPLX(c1, batch_size=9)}
    x, tgt, mask = tref.batch(N, T, seed)
    Tp = tgt.shape[1]
    kps = K.coco_of(tgt.reshape(-1, 66)).astype(np.float32).reshape(N, Tp, 17, 3)
    betas = np.random.default_rng(seed + 1000).normal(0, 1, (N, Tp, 10)).astype(np.float32)
    cu = lambda a: torch.from_numpy(a).cuda()
    tr = GpuTrainer(tref.model(tref.weights(), T), lr=1e-4, smplx_models=bodies, kp_weight=1.0)
    loss = tr.step(cu(x), cu(tgt), cu(mask), target_keypoints=cu(kps), betas=cu(betas), gender_id=np.asarray(gid))
    torch.cuda.synchronize()
    nan = int(torch.isnan(loss).sum()) + int(torch.isnan(tr.last_loss_parts).sum())
    nan += sum(int(torch.isnan(g).sum()) for g in tr.grads().values())
    nan += int(torch.isnan(tr.saved("dposes", 0, (N * Tp, 66))).sum())
    found["nan"] = nan
    me.release(tr, *bodies.values())


def main():
    if os.environ.get("TIK_GUARD") != "1":
        print(json.dumps({"family": "-", "error": "start this program with TIK_GUARD=1"}), flush=True)
        return 2
    import torch
    from temporal_inverse_kinematics_amd import _lib
    lib = me.lib()
    found = {"bad": 0, "report": "", "checks": 0, "nan": 0}

    def check():   # memedge.release calls this while the handles are alive and their work is done
        n = _lib.check(lib.tik_debug_check_guards(), "tik_debug_check_guards")
        found["checks"] += 1
        if n:
            found["bad"] += n
            found["report"] += _lib.last_error()[:1000]

    me.ON_RELEASE = check
    for name, (N, T, seed, gid) in zip(FAMILY_NAMES, SHAPES):
        found.update(bad=0, report="", checks=0, nan=0)
        try:
            step_family(N, T, seed, gid, found)
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
