"""Child program of tests/test_gpu_pose_metrics_guards.py (not a test module), in the pattern of
tests/lm_robust_guard_child.py: started with TIK_GUARD=1 (latched on first use, hence a process of its own) and
TIK_POISON=ff, it runs tik_fk_pose_metrics at B = 1, 3, 37 on both skinning table forms (with and without rows,
target_poses and joints_out, the missing rule on) and one validation step of GpuTrainer(val_metrics=True) at
(N,T) = (5,1) with two body models, on buffers that carry 1 MiB guard zones and a NaN fill, calls
tik_debug_check_guards() while each handle is alive and prints one JSON line {"family", "bad", "report", "checks",
"nan"} per configuration: nan counts the NaNs where the outputs must be finite. On any error it prints
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

FAMILIES = [("pose_metrics", "sparse"), ("pose_metrics", "dense"), ("val_metrics", "5x1")]
FAMILY_NAMES = [f"{k}:{c}" for k, c in FAMILIES]
BATCHES = (1, 3, 37)


def metrics_family(skin, found):
    import numpy as np
    import torch
    import pose_metrics_ref as P
    K = P.K
    with me.env(TIK_FK_SKIN=skin):
        m = K.R.SMPLX(K.consts(), batch_size=9)
    nan = 0
    rng = np.random.default_rng(7)
    for B in BATCHES:
        th = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 66)).astype(np.float32)).cuda()
        tg = torch.from_numpy(rng.uniform(-0.3, 0.3, (B, 66)).astype(np.float32)).cuda()
        k = rng.normal(0, 0.3, (B, 17, 3)).astype(np.float32)
        k[0, 9] = np.nan                     # a missing keypoint in the first frame
        kps = torch.from_numpy(k).cuda()
        betas = torch.from_numpy(rng.normal(0, 1, (B, 10)).astype(np.float32)).cuda()
        w = torch.ones(B, 17, device="cuda")
        rows = torch.from_numpy(rng.permutation(B)[:max(1, B // 2)].astype(np.int32)).cuda()
        for kw in (dict(), dict(betas=betas, joint_weight=w, target_poses=tg, out_joints=torch.zeros(B, 17, 3, device="cuda")),
                   dict(betas=betas[0], target_poses=tg, rows=rows, out=torch.zeros(B, 4, device="cuda"),
                        out_joints=torch.zeros(B, 17, 3, device="cuda")),
                   dict(rows=rows, out=torch.zeros(B, 4, device="cuda"))):
            out = m.pose_metrics(th, kps, skip_nonfinite=True, **kw)
            torch.cuda.synchronize()
            cols = ("mpjpe", "pa_mpjpe", "weight") + (("mpjae",) if "target_poses" in kw else ()) + \
                   (("joints",) if "out_joints" in kw else ())
            nan += sum(int(torch.isnan(out[c]).sum()) for c in cols)
    me.release(m)
    found["nan"] = nan


def val_family(_, found):
    import numpy as np
    import torch
    import pose_metrics_ref as P
    import trainref as tref
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    K = P.K
    N, T, seed, gid = 5, 1, 31, [0, 0, 1, 0, 1]
    c1 = dict(K.consts())
    c1["v_template"] = np.ascontiguousarray(c1["v_template"] * np.float32(1.1))
    bodies = {"a": K.R.SMPLX(K.consts(), batch_size=9), "b": K.R.SMPLX(c1, batch_size=9)}
    x, tgt, _ = tref.batch(N, T, seed)
    Tp = tgt.shape[1]
    kps = K.coco_of(tgt.reshape(-1, 66)).astype(np.float32).reshape(N, Tp, 17, 3)
    betas = np.random.default_rng(seed + 1000).normal(0, 1, (N, Tp, 10)).astype(np.float32)
    cu = lambda a: torch.from_numpy(a).cuda()
    tr = GpuTrainer(tref.model(tref.weights(), T), lr=1e-4, smplx_models=bodies, val_metrics=True)
    out = tr.validation_step({"keypoints_3d": cu(x), "poses": cu(tgt), "target_keypoints_3d": cu(kps), "betas": cu(betas),
                              "gender_id": torch.tensor(gid, dtype=torch.int32)})
    torch.cuda.synchronize()
    found["nan"] = sum(int(torch.isnan(v).sum()) for v in out.values())
    me.release(tr, *bodies.values())


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
            (metrics_family if kind == "pose_metrics" else val_family)(c, found)
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
