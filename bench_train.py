"""SURVEY.md §8f row 4 (optimizer half): the IKPoseTrainer training step on the GPU.

    python bench_train.py [--batch 256] [--T 9] [--steps 50] [--warmup 5] [--kp-loss W]

Workload: the reference's training defaults (pose_trainer.py:204-230:
--bs 256 windows, --win_size 9 -> 9-frame windows, 1 output frame, Adam lr
1e-4), synthetic AMASS-shaped windows and targets resident on the device,
seeded synthetic weights. One step = train-mode forward + MSE + backward +
Adam (GpuTrainer.step -> tik_trainer_step), device dropout masks. Metric:
training windows/s. Algorithmic work per window: forward FLOPs of the
dense contractions (oracle count, 92.9 MFLOP at T=9) x 3 (forward, input
gradient, weight gradient). CPU baseline: oracle/train.py (the reference's
step restated in PyTorch fp32 autograd) on the host, a bounded sample.
--kp-loss W times the step with the keypoint term at weight W (tik_trainer_step_kp:
the three synthetic SMPL-X bodies, a random gender per window, target keypoints =
the bodies' own FK of the target poses) and, alone, the keypoint kernel on the same
rows; without it the step is the plain one, unchanged.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def fwd_flops_per_window(T, layers=((3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 128, 1),
                                    (128, 128, 2), (128, 256, 2), (256, 256, 2))):
    V, fl, t = 17, 0.0, T
    for cin, cout, s in layers:
        to = (t - 1) // s + 1
        fl += 2.0 * t * V * cin * cout + 2.0 * t * V * V * cout + 2.0 * to * V * 3 * cout * cout
        if not (cin == cout and s == 1):
            fl += 2.0 * to * V * cin * cout
        t = to
    fl += 2.0 * t * (V * 256 * 512 + 512 * 66)
    return fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--T", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--eval", action="store_true",
                    help="also time GpuTrainer.validation_step on the same batches, in this process")
    ap.add_argument("--kp-loss", type=float, default=None, metavar="W",
                    help="add the keypoint term rel(FK(pred)) vs rel(keypoints) at weight W (>= 0) to the step")
    a = ap.parse_args()
    import numpy as np
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    _build.build()
    m = IKPoseTrainer(default_hparams(win_size=a.T))
    sd = syn.ik_state_dict(m.regressor.backbone.graph.A, seed=0)
    own = m.regressor.state_dict()
    m.regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=False)
    kp_on = a.kp_loss is not None
    bodies = None
    if kp_on:
        from temporal_inverse_kinematics_amd.smplx_fk import load_smplx_models
        bodies = load_smplx_models(None, "cuda", batch_size=a.batch)
    tr = GpuTrainer(m, lr=1e-4, smplx_models=bodies, kp_weight=a.kp_loss or 0.0)
    B, T = a.batch, a.T
    Tp = T
    for s in m.regressor.backbone.strides:
        Tp = (Tp - 1) // s + 1
    xs = [torch.from_numpy(syn.synthetic_windows(B, T, seed=50 + i)).cuda() for i in range(4)]
    rng = np.random.default_rng(0)
    ys = [torch.from_numpy(rng.normal(0, 0.5, (B, Tp, 66)).astype(np.float32)).cuda() for _ in range(4)]
    kw = [{} for _ in range(4)]
    if kp_on:
        order = sorted(bodies)
        for i in range(4):
            gid = torch.from_numpy(rng.integers(0, len(order), B).astype(np.int32))
            betas = torch.from_numpy(rng.normal(0, 1, (B, bodies[order[0]].num_betas)).astype(np.float32)).cuda()
            full = torch.zeros((B * Tp, 55, 3), device="cuda")
            full[:, :22] = ys[i].reshape(B * Tp, 22, 3)
            rb = betas.repeat_interleave(Tp, 0).contiguous()
            kps = torch.zeros((B * Tp, 17, 3), device="cuda")
            for g, name in enumerate(order):
                sel = torch.nonzero(gid.cuda().repeat_interleave(Tp) == g).flatten()
                if len(sel):
                    kps[sel] = bodies[name].joints(full[sel], rb[sel].contiguous(), select="coco")
            kw[i] = {"target_keypoints": kps.reshape(B, Tp, 17, 3), "betas": betas, "gender_id": gid}
    for i in range(a.warmup):
        tr.step(xs[i % 4], ys[i % 4], seed=i, **kw[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss = tr.step(xs[i % 4], ys[i % 4], seed=1000 + i, **kw[i % 4])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    fl = 3.0 * fwd_flops_per_window(T)
    out = {"metric": "IK training windows/sec (train-mode forward + MSE + backward + Adam)",
           "value": round(B / dt, 1), "unit": "windows/s", "ms_per_step": round(dt * 1e3, 4),
           "higher_is_better": True, "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "dtype": "f32",
           "data": "synthetic (AMASS-shaped windows, random target poses, seeded synthetic weights)",
           "config": {"workload": f"IKPoseTrainer step, bs={B} x {T}-frame windows -> {Tp} output frame(s), Adam lr 1e-4",
                      "batch": B, "window_frames": T},
           "algorithmic_tflops": round(fl * B / dt / 1e12, 2), "mflop_per_window": round(fl / 1e6, 2),
           "roofline": {"scope": "whole step (forward + backward GEMM FLOPs / step time)", "bound": "mfma",
                        "achieved": round(fl * B / dt / 1e12, 2), "peak": 157.3, "unit": "TFLOP/s",
                        "frac": round(fl * B / dt / 1e12 / 157.3, 4),
                        "peak_basis": "dense fp32 MFMA (v_mfma_f32_16x16x4_f32), MI355X_MICROARCH.md"},
           "loss_last": float(loss)}
    if kp_on:
        # the keypoint kernel alone: B * Tp frames of one body, loss and accumulated gradient, as the step launches it
        body = bodies[sorted(bodies)[0]]
        P = ys[0].reshape(B * Tp, 66).contiguous()
        K3, rb = kw[0]["target_keypoints"].reshape(B * Tp, 17, 3), kw[0]["betas"].repeat_interleave(Tp, 0).contiguous()
        ol, og = torch.zeros(B * Tp, device="cuda"), torch.zeros((B * Tp, 66), device="cuda")
        n = max(a.steps, 10)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(n + 3):
            if i == 3:
                ev[0].record()
            body.keypoint_loss(P, K3, betas=rb, out_loss=ol, out_grad=og, grad_scale=1e-3, accumulate=True)
        ev[1].record()
        torch.cuda.synchronize()
        parts = tr.last_loss_parts.cpu().numpy()
        out["kp_loss"] = {"weight": a.kp_loss, "frames": B * Tp, "bodies": len(bodies),
                          "kernel_ms": round(ev[0].elapsed_time(ev[1]) / n, 4),
                          "kernel_scope": f"{n} back-to-back tik_fk_keypoint_loss launches of all frames on one body, HIP events",
                          "pose_mse_last": float(parts[0]), "kp_mse_last": float(parts[1])}
    if a.eval:
        # the eval-mode pass on the live weights (tik_trainer_eval), same batches, same process
        batches = [{"keypoints_3d": xs[i], "poses": ys[i]} for i in range(4)]
        for i in range(max(a.warmup, 1)):
            tr.validation_step(batches[i % 4], i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            vl = tr.validation_step(batches[i % 4], i)["val_loss"]
        torch.cuda.synchronize()
        de = (time.perf_counter() - t0) / a.steps
        out["eval"] = {"metric": "validation_step (eval-mode forward + MSE on the trainer's live weights)",
                       "ms_per_batch": round(de * 1e3, 4), "value": round(B / de, 1), "unit": "windows/s",
                       "train_step_ms": round(dt * 1e3, 4), "val_loss_last": float(vl)}
    if not a.no_cpu_baseline:
        from oracle import train as otr
        nb = 16
        x = syn.synthetic_windows(nb, T, seed=9)
        tgt = np.random.default_rng(1).normal(0, 0.5, (nb, Tp, 66)).astype(np.float32)
        mask = (np.random.default_rng(2).random((nb * Tp, 512)) < 0.3).astype(np.float32)
        otr.train_steps(sd, [(x, tgt, mask)])
        done, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < a.cpu_seconds:
            otr.train_steps(sd, [(x, tgt, mask)])
            done += nb
        d = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(done / d, 1), "unit": "windows/s", "cores": torch.get_num_threads(),
                               "kind": "port", "sample": f"{done} windows in steps of {nb} through oracle/train.py "
                                                         f"(PyTorch fp32 autograd on the host) in {d:.1f}s"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
