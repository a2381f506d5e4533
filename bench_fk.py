"""Config #4: SMPL-X full 55-joint FK + 10475-vertex LBS, batch=4096, 1 GPU.

    python bench_fk.py [--batch 4096] [--steps 10] [--warmup 20] [--joints {all,coco}] [--jacobian] [--refine] [--refine-fused]
                       [--robust S] [--shape-jacobian] [--fit-shape] [--smooth] [--metrics]

Prints one JSON line: bodies/s, and per kernel (HIP events around every launch
of a second pass of the same steps, tik_fk_profile) the algorithmic TFLOP/s of
the blend-shape and skinning GEMMs against the bf16x3 MFMA roof and the
vertex bytes over HBM; then the oracle CPU baseline. bench.py --full reuses
measure_fk() for its "fk" key. --joints adds a "joints" key: the mesh-free
SMPLX.joints (all 144 joints, or the COCO-17 selection) against
full_forward(return_verts=False) at the same batch, the two legs alternating
in this process. --jacobian adds a "jacobian" key (SMPLX.joints_jacobian for
COCO-17 and the 22 body dofs, per-kernel HIP events against the HBM roof of the
bytes it must move), --refine a "refine" key (one Levenberg-Marquardt iteration
of refine.refine_poses: Jacobian, residual map, tik_lm_solve, candidate cost).
--shape-jacobian adds a "shape_jacobian" key (SMPLX.joints_shape_jacobian for
COCO-17, measured like --jacobian), --fit-shape a "fit_shape" key (one
refine.fit_shape of `batch` frames, and tik_lm_accumulate + tik_lm_solve_sum
alone), both at the same batch. --smooth adds a "smooth" key: tik_lm_solve_chain
at (m,n) = (51,66) for one sequence of 256 and of 4096 frames and for 64
sequences of 64 frames, the per-frame tik_lm_solve at the same frame counts, and
one iteration of refine.refine_smooth. --metrics adds a "metrics" key:
SMPLX.pose_metrics (one launch) beside the composed path (SMPLX.joints, torch ops and
a batched 3x3 torch.linalg.svd) and SMPLX.keypoint_loss at loss only (the same FK).
"""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BF16_MFMA_PEAK_TFLOPS = 2516.6   # dense bf16 MFMA (MI355X_MICROARCH.md); bf16x3 runs 6 products per fp32 product
HBM_PEAK_GBS = 8000.0
DTYPES = {"bf16x3": "f32 via bf16x3 (3 bf16 planes, 6 MFMA products, fp32 accumulate; fp32 exponent range)",
          "fp32": "f32 (exact fp32 MFMA)"}


def measure_fk(batch=4096, steps=10, warmup=20):
    """Time `steps` FK+LBS forwards of `batch` bodies (inputs resident), then the
    same steps again with per-launch HIP events: the step time and the per-kernel
    roofline of the two LBS GEMMs (bf16x3: 6 bf16 MFMA products per fp32 product)."""
    import torch
    from temporal_inverse_kinematics_amd import _build, _lib, synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    c = syn.synthetic_smplx_constants(seed=1)
    m = SMPLX(c, batch_size=batch)
    pose, betas = syn.synthetic_fk_inputs(batch, seed=1)
    P, Bt = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    # outputs into preallocated buffers (a serving loop's); 20 warmup steps: the
    # first ~10 FK steps on a fresh box run 5-20 % slow (clocks / caches settling,
    # scripts/diag_fkgap.py: 1.16 -> 0.98 ms/step)
    out = (torch.empty((batch, m.num_joints, 3), device="cuda"), torch.empty((batch, m.num_verts, 3), device="cuda"))
    for _ in range(warmup):
        m.full_forward(P, Bt, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        m.full_forward(P, Bt, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    lib = _lib.load()
    _lib.check(lib.tik_fk_profile(m._h, 8 * steps))
    for _ in range(steps):
        m.full_forward(P, Bt, out=out)
    torch.cuda.synchronize()
    agg = {}
    lab = ctypes.create_string_buffer(64)
    kms, fl, by = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    for i in range(_lib.check(lib.tik_fk_profile_count(m._h))):
        _lib.check(lib.tik_fk_profile_read(m._h, i, lab, 64, ctypes.byref(kms), ctypes.byref(fl), ctypes.byref(by)))
        a = agg.setdefault(lab.value.decode(), [0.0, 0, 0.0, 0.0])
        a[0] += kms.value; a[1] += 1; a[2] += fl.value; a[3] += by.value
    lib.tik_fk_profile(m._h, 0)
    nprod = 6 if m.precision == "bf16x3" else 1
    roof = BF16_MFMA_PEAK_TFLOPS / 6 if nprod == 6 else 157.3
    kernels = {}
    for k, (t, n, f, b) in agg.items():
        s = t / 1e3
        d = {"avg_ms": round(t / n, 4), "share": round(t / sum(v[0] for v in agg.values()), 3)}
        if f > 0:
            d.update({"tflops": round(f / s / 1e12, 2), "mfma_frac": round(f / s / 1e12 / roof, 4)})
        d.update({"gbs": round(b / s / 1e9, 1), "hbm_frac": round(b / s / 1e9 / HBM_PEAK_GBS, 4)})
        kernels[k] = d
    V = c["v_template"].shape[0]
    gemm_flops = 2.0 * batch * 3 * V * 507 + 2.0 * batch * V * 12 * 55 + 18.0 * batch * V
    vert_bytes = batch * V * 3 * 4
    return {"metric": "SMPL-X FK+LBS bodies/sec", "value": round(batch / (ms / 1e3), 1), "unit": "bodies/s",
            "n_gpus": 1, "ms_per_step": round(ms, 4), "steps": steps, "warmup": warmup,
            "dtype": DTYPES.get(m.precision, m.precision),
            "config": {"workload": f"SMPL-X 55-joint FK + {V}-vertex LBS + 144 joints, batch={batch}"},
            "gemm_tflops": round(gemm_flops / (ms / 1e3) / 1e12, 2), "mflop_per_body": round(gemm_flops / batch / 1e6, 2),
            "mfma_roof_tflops": round(roof, 1),
            "vertex_gbs": round(vert_bytes / (ms / 1e3) / 1e9, 1),
            "vertex_hbm_frac": round(vert_bytes / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
            "bytes_out_per_body": (V * 3 + 144 * 3) * 4, "kernels": kernels,
            "outputs": "joints and vertices written into preallocated buffers (SMPLX.full_forward(out=...))",
            "basis": "kernels: HIP events around each launch of a second pass of the same steps (tik_fk_profile); "
                     "tflops = algorithmic fp32 FLOPs / event time, mfma_frac against the bf16x3 roof "
                     f"({BF16_MFMA_PEAK_TFLOPS} TF dense bf16 / 6 products); vertex_gbs = vertex bytes written / step time"}


def _profile(m, run, steps):
    """Per-label HIP-event averages of `steps` calls of run() (tik_fk_profile)."""
    import torch
    from temporal_inverse_kinematics_amd import _lib
    lib = _lib.load()
    _lib.check(lib.tik_fk_profile(m._h, 8 * steps))
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    agg = {}
    lab = ctypes.create_string_buffer(64)
    kms, fl, by = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    for i in range(_lib.check(lib.tik_fk_profile_count(m._h))):
        _lib.check(lib.tik_fk_profile_read(m._h, i, lab, 64, ctypes.byref(kms), ctypes.byref(fl), ctypes.byref(by)))
        a = agg.setdefault(lab.value.decode(), [0.0, 0, 0.0, 0.0])
        a[0] += kms.value; a[1] += 1; a[2] += fl.value; a[3] += by.value
    lib.tik_fk_profile(m._h, 0)
    tot = sum(v[0] for v in agg.values())
    return {k: {"avg_ms": round(t / n, 4), "share": round(t / tot, 3), "gflops": round(f / (t / 1e3) / 1e9, 1),
                "gbs": round(b / (t / 1e3) / 1e9, 1)} for k, (t, n, f, b) in agg.items()}


def measure_joints(select="all", batch=4096, steps=10, warmup=20, rounds=5):
    """SMPLX.joints (select: "all" or "coco") against full_forward(return_verts=False)
    at `batch` bodies, outputs preallocated, inputs resident: `rounds` rounds, each
    timing `steps` calls of one leg and then of the other (HIP events), the median
    round per leg. The joints handle is a fresh one, so its workspace is the joints
    path's alone."""
    import statistics
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    c = syn.synthetic_smplx_constants(seed=1)
    mj, mf = SMPLX(c, batch_size=batch), SMPLX(c, batch_size=batch)
    pose, betas = syn.synthetic_fk_inputs(batch, seed=1)
    P, Bt = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    sel = None if select == "all" else select
    n = mj.num_joints if sel is None else 17
    oj = torch.empty((batch, n, 3), device="cuda")
    of = (torch.empty((batch, mf.num_joints, 3), device="cuda"), None)
    legs = {"joints": lambda: mj.joints(P, Bt, select=sel, out=oj),
            "full_forward": lambda: mf.full_forward(P, Bt, return_verts=False, out=of)}
    for _ in range(warmup):
        for run in legs.values():
            run()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, run in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ws = mj.workspace_bytes
    return {"select": select, "n_joints": n, "batch": batch, "steps": steps, "warmup": warmup, "rounds": rounds,
            "joints_ms": round(med["joints"], 4), "full_forward_ms": round(med["full_forward"], 4),
            "ratio": round(med["full_forward"] / med["joints"], 2),
            "joints_ms_rounds": [round(v, 4) for v in ms["joints"]],
            "full_forward_ms_rounds": [round(v, 4) for v in ms["full_forward"]],
            "workspace_bytes": ws, "full_forward_workspace_bytes": mf.workspace_bytes,
            "kernels": _profile(mj, legs["joints"], steps),
            "basis": "median of rounds, each `steps` calls per leg between HIP events, legs alternating; "
                     "full_forward(return_verts=False) builds the body in the handle's workspace"}


def _timed(run, steps, warmup, rounds=5):
    """Median over `rounds` of the HIP-event time of `steps` calls of run(), in ms per call."""
    import statistics
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return statistics.median(ms), [round(v, 4) for v in ms]


def measure_jacobian(batch=4096, steps=10, warmup=20):
    """SMPLX.joints_jacobian(select="coco", dof=None, return_joints=False) at `batch`
    bodies on a fresh handle: call time (HIP events, median of 5 rounds), the
    per-launch profile, and the fk_jacobian launches against the HBM roof of their
    algorithmic bytes (the (B,51,66) Jacobian out, the chain's outputs in)."""
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, betas = syn.synthetic_fk_inputs(batch, seed=1)
    P, Bt = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    run = lambda: m.joints_jacobian(P, Bt, select="coco", return_joints=False)
    med, rounds = _timed(run, steps, warmup)
    k = _profile(m, run, steps)
    jk = k.get("fk_jacobian", {})
    roof_ms = None
    if jk:
        roof_ms = jk["gbs"] * jk["avg_ms"] / HBM_PEAK_GBS   # bytes / peak bandwidth
    return {"select": "coco", "n_dof": 22, "batch": batch, "steps": steps, "warmup": warmup,
            "jacobian_ms": round(med, 4), "jacobian_ms_rounds": rounds, "workspace_bytes": m.workspace_bytes,
            "kernels": k, "fk_jacobian_hbm_roof_ms": None if roof_ms is None else round(roof_ms, 4),
            "fk_jacobian_share_of_hbm_roof": None if not roof_ms else round(roof_ms / jk["avg_ms"], 3),
            "basis": "median of 5 rounds of `steps` calls between HIP events; kernels: per-launch HIP events "
                     "(pre-pass and main kernel under one fk_jacobian label); roof = algorithmic bytes / 8 TB/s"}


def measure_refine(batch=4096, steps=10, warmup=20):
    """One LM iteration of refine.refine_poses at `batch` frames: the time of
    refine_poses(iters=1) minus refine_poses(iters=0) (uploads, the first cost and
    the copies back are in both), and tik_lm_solve alone on (batch,51,66)."""
    import numpy as np
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.refine import refine_poses
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX, lm_solve
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, _ = syn.synthetic_fk_inputs(batch, seed=1)
    th0 = np.ascontiguousarray(pose[:, :22].reshape(batch, 66))
    full = torch.zeros((batch, 55, 3), device="cuda")
    full[:, :22] = torch.from_numpy(pose[:, :22]).cuda() + 0.05
    kps = m.joints(full, select="coco").cpu().numpy()
    t1, r1 = _timed(lambda: refine_poses(th0, kps, m, iters=1), steps, warmup)
    t0, r0 = _timed(lambda: refine_poses(th0, kps, m, iters=0), steps, warmup)
    jac, joints = m.joints_jacobian(torch.from_numpy(pose).cuda(), select="coco")
    r = joints.reshape(batch, 51).contiguous()
    lam = torch.full((batch,), 1e-2, device="cuda")
    ts, rs = _timed(lambda: lm_solve(jac, r, lam, mu=1e-2), steps, warmup)
    return {"batch": batch, "steps": steps, "warmup": warmup, "lm_iteration_ms": round(t1 - t0, 4),
            "refine_iters1_ms": round(t1, 4), "refine_iters0_ms": round(t0, 4), "lm_solve_ms": round(ts, 4),
            "refine_iters1_ms_rounds": r1, "refine_iters0_ms_rounds": r0, "lm_solve_ms_rounds": rs,
            "basis": "median of 5 rounds of `steps` calls between HIP events; refine_poses includes its "
                     "host-to-device uploads and the copy back; lm_solve: (batch,51,66) systems, output allocated per call"}


def measure_refine_fused(batch=4096, steps=10, warmup=20, iters=3, robust=0.0):
    """The fused path beside measure_refine, same frames: refine_poses(fused=True) at `iters` and at 0 iterations
    (uploads, the first cost and the copies back are in both), their difference per iteration; and
    SMPLX.refine_frames alone on resident tensors, per iteration. robust > 0: the Geman-McClure data term at that
    scale (metres) in all four."""
    import numpy as np
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.refine import refine_poses
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, _ = syn.synthetic_fk_inputs(batch, seed=1)
    th0 = np.ascontiguousarray(pose[:, :22].reshape(batch, 66))
    full = torch.zeros((batch, 55, 3), device="cuda")
    full[:, :22] = torch.from_numpy(pose[:, :22]).cuda() + 0.05
    kps_d = m.joints(full, select="coco")
    kps = kps_d.cpu().numpy()
    tn, rn = _timed(lambda: refine_poses(th0, kps, m, iters=iters, fused=True, robust_sigma=robust), steps, warmup)
    t0, r0 = _timed(lambda: refine_poses(th0, kps, m, iters=0, fused=True, robust_sigma=robust), steps, warmup)
    th_d = torch.from_numpy(th0).cuda()
    kn, krn = _timed(lambda: m.refine_frames(th_d, kps_d, iters=iters, robust_sigma=robust), steps, warmup)
    k0, kr0 = _timed(lambda: m.refine_frames(th_d, kps_d, iters=0, robust_sigma=robust), steps, warmup)
    return {"batch": batch, "steps": steps, "warmup": warmup, "iters": iters, **({"robust_sigma": robust} if robust else {}),
            "lm_iteration_ms": round((tn - t0) / iters, 4), "refine_fused_ms": round(tn, 4), "refine_fused_iters0_ms": round(t0, 4),
            "kernel_iteration_ms": round((kn - k0) / iters, 4), "kernel_ms": round(kn, 4), "kernel_iters0_ms": round(k0, 4),
            "refine_fused_ms_rounds": rn, "refine_fused_iters0_ms_rounds": r0, "kernel_ms_rounds": krn, "kernel_iters0_ms_rounds": kr0,
            "basis": "median of 5 rounds of `steps` calls between HIP events; refine_poses(fused=True) includes its "
                     "host-to-device uploads and the copy back; kernel: SMPLX.refine_frames on resident tensors, outputs "
                     "allocated per call"}


def composed_metrics(m, full, kps):
    """mpjpe and pa_mpjpe (B,) of the composed path: SMPLX.joints, then Umeyama's alignment in torch ops with a batched
    3x3 torch.linalg.svd (unit weights, the proper rotation)."""
    import torch
    x = m.joints(full, select="coco")
    x = x - 0.5 * (x[:, 11:12] + x[:, 12:13])
    y = kps - 0.5 * (kps[:, 11:12] + kps[:, 12:13])
    mpjpe = (x - y).norm(dim=2).mean(dim=1)
    xc, yc = x - x.mean(dim=1, keepdim=True), y - y.mean(dim=1, keepdim=True)
    U, D, Vt = torch.linalg.svd(yc.transpose(1, 2) @ xc)
    sgn = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
    S = torch.ones_like(D)
    S[:, 2] = sgn
    Rm = (U * S[:, None, :]) @ Vt
    sc = (D * S).sum(dim=1) / (xc * xc).sum(dim=(1, 2))
    pa = (sc[:, None, None] * (xc @ Rm.transpose(1, 2)) - yc).norm(dim=2).mean(dim=1)
    return mpjpe, pa


def measure_metrics(batch=4096, steps=10, warmup=20):
    """SMPLX.pose_metrics at `batch` frames on resident tensors (one launch, outputs preallocated), the composed path
    on the same frames (composed_metrics above), and SMPLX.keypoint_loss at loss only through the C entry point: the
    same FK without the alignment. Also the largest difference between the two paths' values."""
    import torch
    from temporal_inverse_kinematics_amd import _build, _lib, synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, _ = syn.synthetic_fk_inputs(batch, seed=1)
    full = torch.zeros((batch, 55, 3), device="cuda")
    full[:, :22] = torch.from_numpy(pose[:, :22]).cuda()
    target = (full[:, :22] + 0.05).reshape(batch, 66).contiguous()
    tfull = torch.zeros_like(full)
    tfull[:, :22] = target.reshape(batch, 22, 3)
    kps = m.joints(tfull, select="coco")
    th = full[:, :22].reshape(batch, 66).contiguous()
    out, oj = torch.empty((batch, 4), device="cuda"), torch.empty((batch, 17, 3), device="cuda")
    tk, rk = _timed(lambda: m.pose_metrics(th, kps, target_poses=target, out=out), steps, warmup)
    tj, rj = _timed(lambda: m.pose_metrics(th, kps, target_poses=target, out=out, out_joints=oj), steps, warmup)
    tc, rc = _timed(lambda: composed_metrics(m, full, kps), steps, warmup)
    loss = torch.empty((batch,), device="cuda")
    lib, st = _lib.load(), _lib.stream_of(th)
    kploss = lambda: _lib.check(lib.tik_fk_keypoint_loss(m._h, th.data_ptr(), 66, kps.data_ptr(), None, 0, None, 0, None, None,
                                                         batch, loss.data_ptr(), None, 0, 1.0, 0, st))
    tl, rl = _timed(kploss, steps, warmup)
    got = m.pose_metrics(th, kps, target_poses=target, out=out)
    cm, cp = composed_metrics(m, full, kps)
    return {"batch": batch, "steps": steps, "warmup": warmup, "pose_metrics_ms": round(tk, 4),
            "pose_metrics_with_joints_ms": round(tj, 4), "composed_ms": round(tc, 4), "keypoint_loss_only_ms": round(tl, 4),
            "composed_over_kernel": round(tc / tk, 2), "pose_metrics_ms_rounds": rk, "pose_metrics_with_joints_ms_rounds": rj,
            "composed_ms_rounds": rc, "keypoint_loss_only_ms_rounds": rl,
            "max_abs_diff_mpjpe": float((got["mpjpe"] - cm).abs().max()), "max_abs_diff_pa_mpjpe": float((got["pa_mpjpe"] - cp).abs().max()),
            "mean_mpjpe": float(got["mpjpe"].mean()), "mean_pa_mpjpe": float(got["pa_mpjpe"].mean()),
            "mean_mpjae": float(got["mpjae"].mean()),
            "basis": "median of 5 rounds of `steps` calls between HIP events, resident tensors; pose_metrics: one launch, "
                     "outputs preallocated; composed: SMPLX.joints + torch ops + batched 3x3 torch.linalg.svd, outputs "
                     "allocated per call; keypoint_loss_only: tik_fk_keypoint_loss with grad = NULL"}


def measure_shape_jacobian(batch=4096, steps=10, warmup=20):
    """SMPLX.joints_shape_jacobian(select="coco", return_joints=False) at `batch` bodies
    on a fresh handle, measured like measure_jacobian: call time, the per-launch
    profile, and the fk_shape_jacobian launches against the HBM roof of their
    algorithmic bytes (the (B,51,nb) Jacobian out, the transforms in, the beta
    workspace written and read)."""
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, betas = syn.synthetic_fk_inputs(batch, seed=1)
    P, Bt = torch.from_numpy(pose).cuda(), torch.from_numpy(betas).cuda()
    run = lambda: m.joints_shape_jacobian(P, Bt, select="coco", return_joints=False)
    med, rounds = _timed(run, steps, warmup)
    k = _profile(m, run, steps)
    jk = k.get("fk_shape_jacobian", {})
    roof_ms = None
    if jk:
        roof_ms = jk["gbs"] * jk["avg_ms"] / HBM_PEAK_GBS   # bytes / peak bandwidth
    return {"select": "coco", "num_betas": m.num_betas, "batch": batch, "steps": steps, "warmup": warmup,
            "shape_jacobian_ms": round(med, 4), "shape_jacobian_ms_rounds": rounds, "workspace_bytes": m.workspace_bytes,
            "kernels": k, "fk_shape_jacobian_hbm_roof_ms": None if roof_ms is None else round(roof_ms, 4),
            "fk_shape_jacobian_share_of_hbm_roof": None if not roof_ms else round(roof_ms / jk["avg_ms"], 3),
            "basis": "median of 5 rounds of `steps` calls between HIP events; kernels: per-launch HIP events "
                     "(pre-pass and main kernel under one fk_shape_jacobian label); roof = algorithmic bytes / 8 TB/s"}


def measure_fit_shape(batch=4096, steps=10, warmup=20):
    """One refine.fit_shape of `batch` frames (shape Jacobian, residual map,
    tik_lm_accumulate, tik_lm_solve_sum, the candidate's cost; uploads and the
    copies back included), and the two tik_lm_* calls alone on (batch,51,nb)."""
    import numpy as np
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.refine import fit_shape
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX, lm_accumulate, lm_solve_sum
    _build.build()
    m = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=batch)
    pose, betas = syn.synthetic_fk_inputs(batch, seed=1)
    th = np.ascontiguousarray(pose[:, :22].reshape(batch, 66))
    full = torch.zeros((batch, 55, 3), device="cuda")
    full[:, :22] = torch.from_numpy(pose[:, :22]).cuda()
    one = torch.from_numpy(np.tile(betas[:1], (batch, 1))).cuda()   # one body shape for the whole sequence
    kps = m.joints(full, one, select="coco").cpu().numpy()
    tf, rf = _timed(lambda: fit_shape(th, kps, m), steps, warmup)
    jac, joints = m.joints_shape_jacobian(full, select="coco")
    r = joints.reshape(batch, 51).contiguous()
    partial = lm_accumulate(jac, r)
    ta, ra = _timed(lambda: lm_accumulate(jac, r, out=partial), steps, warmup)
    ts, rs = _timed(lambda: lm_solve_sum(partial, mu=1e-3), steps, warmup)
    return {"batch": batch, "num_betas": m.num_betas, "steps": steps, "warmup": warmup, "fit_shape_ms": round(tf, 4),
            "lm_accumulate_ms": round(ta, 4), "lm_solve_sum_ms": round(ts, 4), "partial_rows": int(partial.shape[0]),
            "fit_shape_ms_rounds": rf, "lm_accumulate_ms_rounds": ra, "lm_solve_sum_ms_rounds": rs,
            "basis": "median of 5 rounds of `steps` calls between HIP events; fit_shape includes its host-to-device "
                     "uploads, the cost before and after, and the copy back; lm_accumulate: (batch,51,nb) into a "
                     "preallocated buffer; lm_solve_sum: its rows, output allocated per call"}


def measure_smooth(steps=10, warmup=20):
    """smplx_fk.lm_solve_chain on random (F,51,66) systems (workspace preallocated,
    seq_starts resident): one sequence of F = 256 and of F = 4096 frames (the sweep
    is sequential in F: one workgroup), 64 sequences of 64 frames, each beside the
    per-frame lm_solve of the same frames; and one iteration of refine.refine_smooth
    at F = 4096 in 64 sequences (iters=1 minus iters=0, as measure_refine)."""
    import numpy as np
    import torch
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.refine import refine_smooth
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX, lm_chain_workspace_floats, lm_solve, lm_solve_chain
    _build.build()
    m, n, smooth, mu = 51, 66, 0.1, 1e-2
    out = {"m": m, "n": n, "smooth": smooth, "steps": steps, "warmup": warmup, "cases": {}}
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, F, S in (("1x256", 256, 1), ("1x4096", 4096, 1), ("64x64", 4096, 64)):
        J = torch.randn((F, m, n), device="cuda", generator=g)
        r = torch.randn((F, m), device="cuda", generator=g)
        th = torch.randn((F, n), device="cuda", generator=g)
        lam = torch.full((S,), 1e-2, device="cuda")
        lam_f = torch.full((F,), 1e-2, device="cuda")
        starts = torch.arange(0, F + 1, F // S, device="cuda", dtype=torch.int32)
        work = torch.empty((lm_chain_workspace_floats(F, n),), device="cuda")
        w = min(warmup, 3)   # a 4096-frame sweep takes long enough to settle the clocks in a few calls
        tc, rc = _timed(lambda: lm_solve_chain(J, r, lam, th, smooth, mu=mu, seq_starts=starts, workspace=work), steps, w)
        tf, rf = _timed(lambda: lm_solve(J, r, lam_f, mu=mu), steps, w)
        d = lm_solve_chain(J, r, lam, th, smooth, mu=mu, seq_starts=starts, workspace=work)
        out["cases"][name] = {"frames": F, "sequences": S, "lm_solve_chain_ms": round(tc, 4), "lm_solve_ms": round(tf, 4),
                              "ratio": round(tc / tf, 2), "us_per_frame_of_a_sequence": round(1e3 * tc / (F // S), 3),
                              "finite": bool(torch.isfinite(d).all()), "lm_solve_chain_ms_rounds": rc, "lm_solve_ms_rounds": rf}
    F, S = 4096, 64
    model = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=F)
    pose, _ = syn.synthetic_fk_inputs(F, seed=1)
    th0 = np.ascontiguousarray(pose[:, :22].reshape(F, 66))
    full = torch.zeros((F, 55, 3), device="cuda")
    full[:, :22] = torch.from_numpy(pose[:, :22]).cuda() + 0.05
    kps = model.joints(full, select="coco").cpu().numpy()
    st = np.arange(0, F + 1, F // S)
    t1, r1 = _timed(lambda: refine_smooth(th0, kps, model, smooth, iters=1, seq_starts=st), steps, min(warmup, 3))
    t0, r0 = _timed(lambda: refine_smooth(th0, kps, model, smooth, iters=0, seq_starts=st), steps, min(warmup, 3))
    out["refine_smooth"] = {"frames": F, "sequences": S, "iteration_ms": round(t1 - t0, 4), "iters1_ms": round(t1, 4),
                            "iters0_ms": round(t0, 4), "iters1_ms_rounds": r1, "iters0_ms_rounds": r0}
    out["basis"] = ("median of 5 rounds of `steps` calls between HIP events; lm_solve_chain: both launches, workspace and "
                    "seq_starts resident, delta allocated per call; refine_smooth includes its uploads and the copy back")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--joints", choices=["all", "coco"], default=None,
                    help="also time the mesh-free SMPLX.joints against full_forward(return_verts=False)")
    ap.add_argument("--jacobian", action="store_true",
                    help="also time SMPLX.joints_jacobian (COCO-17, the 22 body dofs)")
    ap.add_argument("--refine", action="store_true",
                    help="also time one Levenberg-Marquardt iteration of refine.refine_poses and tik_lm_solve alone")
    ap.add_argument("--refine-fused", action="store_true",
                    help="also time the fused path (refine_poses(fused=True), SMPLX.refine_frames) per LM iteration")
    ap.add_argument("--robust", type=float, default=0.0, metavar="S",
                    help="with --refine-fused: the Geman-McClure scale of the data term in metres (0: the plain square)")
    ap.add_argument("--shape-jacobian", action="store_true",
                    help="also time SMPLX.joints_shape_jacobian (COCO-17, all betas)")
    ap.add_argument("--fit-shape", action="store_true",
                    help="also time one refine.fit_shape and tik_lm_accumulate / tik_lm_solve_sum alone")
    ap.add_argument("--smooth", action="store_true",
                    help="also time tik_lm_solve_chain (1 x 256, 1 x 4096 and 64 x 64 frames) beside tik_lm_solve, and one "
                         "refine.refine_smooth iteration")
    ap.add_argument("--metrics", action="store_true",
                    help="also time SMPLX.pose_metrics beside the composed path (SMPLX.joints + torch.linalg.svd) and "
                         "SMPLX.keypoint_loss at loss only")
    a = ap.parse_args()
    from temporal_inverse_kinematics_amd import synthetic as syn
    out = measure_fk(a.batch, a.steps, a.warmup)
    if a.joints:
        out["joints"] = measure_joints(a.joints, a.batch, a.steps, a.warmup)
    if a.jacobian:
        out["jacobian"] = measure_jacobian(a.batch, a.steps, a.warmup)
    if a.refine:
        out["refine"] = measure_refine(a.batch, a.steps, a.warmup)
    if a.refine_fused:
        out["refine_fused"] = measure_refine_fused(a.batch, a.steps, a.warmup, robust=a.robust)
    if a.shape_jacobian:
        out["shape_jacobian"] = measure_shape_jacobian(a.batch, a.steps, a.warmup)
    if a.fit_shape:
        out["fit_shape"] = measure_fit_shape(a.batch, a.steps, a.warmup)
    if a.smooth:
        out["smooth"] = measure_smooth(a.steps, a.warmup)
    if a.metrics:
        out["metrics"] = measure_metrics(a.batch, a.steps, a.warmup)
    from oracle import smplx_lbs as sl
    c = syn.synthetic_smplx_constants(seed=1)
    pose, betas = syn.synthetic_fk_inputs(16, seed=1)
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < a.cpu_seconds:
        sl.smplx_forward(c, pose, betas); n += 16
    dt = time.perf_counter() - t0
    out["cpu_baseline"] = {"value": round(n / dt, 1), "unit": "bodies/s", "kind": "port",
                           "sample": f"{n} bodies through oracle/smplx_lbs.py (numpy f64) in {dt:.1f}s"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
