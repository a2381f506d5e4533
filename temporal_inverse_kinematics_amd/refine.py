"""Levenberg-Marquardt refinement of solved poses on the GPU.

The IK regressor's pose is a starting point; a few damped least-squares
iterations pull the FK joints of the pose onto the keypoints it was solved
from. Per frame, with theta the 66 pose values of joints 0..21 (the hands stay
zero, no translation: the layout of inference.fk_check):

    r(theta)    = rel(FK COCO-17(theta)) - rel(kps)        rel(x) = x - mean of COCO 11/12
    cost(theta) = 1/2 sum_k w_k |r_k|^2 + 1/2 prior_weight |theta - theta0|^2
    (J^T W J + (prior_weight + lambda) I) delta = -(J^T W r + prior_weight (theta - theta0))

J comes from SMPLX.joints_jacobian (tik_fk_joints_jacobian), the same linear
map `rel` applied to its rows; the solve is smplx_fk.lm_solve (tik_lm_solve),
one workgroup per frame. The prior toward the network's pose theta0 is what
makes the problem well-posed: 17 keypoints do not determine 22 rotations.
"""
from __future__ import annotations

import numpy as np
import torch

from .smplx_fk import lm_solve

NUM_DOF = 66


def _rel(x: torch.Tensor) -> torch.Tensor:
    """Root-relative as inference.fk_check: minus the mean of COCO 11 and 12, along dim 1."""
    return x - 0.5 * (x[:, 11:12] + x[:, 12:13])


def _check_args(poses, seq_3d_kps, iters, prior_weight, joint_weight, lam0):
    """The ValueErrors of refine_poses, before any device work."""
    p = np.asarray(poses)
    if p.ndim != 2 or p.shape[1] < NUM_DOF:
        raise ValueError(f"poses must be (F, >= {NUM_DOF}), got {p.shape}")
    k = np.asarray(seq_3d_kps.shape if hasattr(seq_3d_kps, "shape") else np.asarray(seq_3d_kps).shape)
    F = p.shape[0]
    if int(np.prod(k)) != F * 51:
        raise ValueError(f"seq_3d_kps must be ({F}, 17, 3), got {tuple(k)}")
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    if not float(prior_weight) > 0.0:
        raise ValueError("prior_weight must be > 0: 17 keypoints do not determine 22 rotations, "
                         "the prior toward the solved pose is what makes the problem well-posed")
    if not float(lam0) > 0.0:
        raise ValueError(f"lam0 must be > 0, got {lam0}")
    if joint_weight is not None:
        w = np.asarray(joint_weight, np.float32)
        if w.shape != (17,) or not (w >= 0).all():
            raise ValueError("joint_weight must be 17 non-negative values (COCO order)")


def refine_poses(poses, seq_3d_kps, smplx_model, betas=None, iters: int = 10, prior_weight: float = 1e-2,
                 joint_weight=None, lam0: float = 1e-2) -> dict:
    """poses (F,66) solved by the IK, seq_3d_kps (F,17,3) COCO -> {"poses": (F,66)
    float32 numpy, "cost": (iters+1, F) host array of the cost per frame}
    (cost[0] is theta0's, each later row the accepted pose's after that
    iteration; it never increases).

    Per frame and iteration: the LM step from the current pose, the candidate's
    cost with SMPLX.joints, accepted where the cost fell (lambda <- lambda / 3),
    the old pose kept elsewhere (lambda <- 3 lambda); a NaN step counts as
    rejected. All on the device with torch.where, no host round trip inside an
    iteration; the cost history is copied once at the end. Frames go through in
    chunks of at most inference.MAX_WINDOWS_PER_CALL."""
    _check_args(poses, seq_3d_kps, iters, prior_weight, joint_weight, lam0)
    from .inference import MAX_WINDOWS_PER_CALL
    dev = smplx_model.device
    iters, pw = int(iters), float(prior_weight)
    th_all = torch.as_tensor(np.ascontiguousarray(np.asarray(poses, dtype=np.float32)[:, :NUM_DOF]), device=dev)
    F = th_all.shape[0]
    kps_all = torch.as_tensor(np.ascontiguousarray(seq_3d_kps, dtype=np.float32), device=dev).reshape(F, 17, 3)
    wj = None if joint_weight is None else torch.as_tensor(np.asarray(joint_weight, np.float32), device=dev)
    row_w = None if wj is None else wj.repeat_interleave(3).contiguous()
    out = torch.empty((F, NUM_DOF), device=dev)
    hist = torch.empty((iters + 1, F), device=dev)

    with torch.no_grad():
        for s in range(0, F, MAX_WINDOWS_PER_CALL):
            n = min(MAX_WINDOWS_PER_CALL, F - s)
            th0 = th_all[s:s + n]
            target = _rel(kps_all[s:s + n])
            b = None
            if betas is not None:
                b = torch.as_tensor(np.asarray(betas, np.float32)[:smplx_model.num_betas][None], device=dev)
                b = b.expand(n, -1).contiguous()
            full = torch.zeros((n, 55, 3), device=dev)

            def full_pose(th):
                full[:, :22] = th.reshape(n, 22, 3)
                return full

            def cost_of(r, th):
                sq = r.reshape(n, 17, 3).square().sum(2)
                data = (sq if wj is None else sq * wj).sum(1)
                return 0.5 * data + 0.5 * pw * (th - th0).square().sum(1)

            th = th0.clone()
            lam = torch.full((n,), float(lam0), device=dev)
            cost = cost_of((_rel(smplx_model.joints(full_pose(th), b, None, None, select="coco")) - target).reshape(n, 51), th)
            hist[0, s:s + n] = cost
            for it in range(iters):
                jac, joints = smplx_model.joints_jacobian(full_pose(th), b, None, None, select="coco")
                r = (_rel(joints) - target).reshape(n, 51).contiguous()
                jr = _rel(jac.reshape(n, 17, 3, NUM_DOF)).reshape(n, 51, NUM_DOF).contiguous()
                delta = lm_solve(jr, r, lam, mu=pw, prior=(th - th0).contiguous(), row_weight=row_w)
                cand = th + delta
                rc = (_rel(smplx_model.joints(full_pose(cand), b, None, None, select="coco")) - target).reshape(n, 51)
                cc = cost_of(rc, cand)
                ok = cc < cost   # False for a NaN step
                th = torch.where(ok[:, None], cand, th)
                cost = torch.where(ok, cc, cost)
                lam = torch.where(ok, lam / 3.0, lam * 3.0)
                hist[it + 1, s:s + n] = cost
            out[s:s + n] = th
    return {"poses": out.cpu().numpy(), "cost": hist.cpu().numpy()}
