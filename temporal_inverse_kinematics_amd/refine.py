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

The body shape is one set of betas for the whole sequence:

    cost(theta, beta) = sum_f [ 1/2 sum_k w_k |r_fk|^2 + 1/2 prior_weight |theta_f - theta0_f|^2 ]
                        + 1/2 shape_weight |beta|^2

For fixed poses the joints are affine in beta, so the shape step (fit_shape)
is one linear least-squares problem shared by all frames, solved exactly:

    (sum_f Jb_f^T W Jb_f + shape_weight I) d = -(sum_f Jb_f^T W r_f + shape_weight beta)

Jb_f comes from SMPLX.joints_shape_jacobian (tik_fk_joints_shape_jacobian)
with `rel` applied to its rows; the per-frame normal equations are summed by
smplx_fk.lm_accumulate (tik_lm_accumulate) and solved once by
smplx_fk.lm_solve_sum (tik_lm_solve_sum). refine_sequence alternates that
step with refine_poses.

refine_poses treats every frame alone. refine_smooth ties the frames of a
sequence together:

    cost = sum_f cost(theta_f) + 1/2 smooth_weight sum_f |theta_{f+1} - theta_f|^2

Its Gauss-Newton matrix is block tridiagonal, the diagonal blocks those of
refine_poses plus smooth_weight c_f I (c_f neighbours), every off-diagonal
block -smooth_weight I; smplx_fk.lm_solve_chain (tik_lm_solve_chain) solves a
whole sequence in one workgroup. Weights per frame and keypoint let a keypoint,
or a whole frame, that was not detected be filled from the neighbours.

refine_poses(fused=True) runs all iterations of a chunk of frames in one launch
(SMPLX.refine_frames, tik_fk_refine); the same kernel refines one frame per push
inside streaming.OnlineIK.

The drivers share their pieces: _upload (host to device, once per call),
_chunks (the one reader of inference.MAX_WINDOWS_PER_CALL), _FKView (r, J and
Jb of a run of frames), _data_term and _lm_loop (the accept rule).
"""
from __future__ import annotations

import numpy as np
import torch

from . import inference
from .smplx_fk import (LM_RUN, check_robust_args, lm_accumulate, lm_chain_starts, lm_chain_workspace_floats, lm_partial_width, lm_solve,
                       lm_solve_chain, lm_solve_sum)

NUM_DOF = 66


def _rel(x: torch.Tensor) -> torch.Tensor:
    """Root-relative: minus the mean of COCO 11 and 12 (the hips), along dim 1."""
    return x - 0.5 * (x[:, 11:12] + x[:, 12:13])


# ---------------------------------------------------------------- argument checks, before any device work
def _check_frames(poses, seq_3d_kps) -> int:
    """poses (F, >= 66) and as many keypoints (F,17,3) -> F."""
    p = np.asarray(poses)
    if p.ndim != 2 or p.shape[1] < NUM_DOF:
        raise ValueError(f"poses must be (F, >= {NUM_DOF}), got {p.shape}")
    k = np.asarray(seq_3d_kps.shape if hasattr(seq_3d_kps, "shape") else np.asarray(seq_3d_kps).shape)
    F = p.shape[0]
    if int(np.prod(k)) != F * 51:
        raise ValueError(f"seq_3d_kps must be ({F}, 17, 3), got {tuple(k)}")
    return F


def _check_lm_scalars(iters, prior_weight, lam0):
    if int(iters) < 0:
        raise ValueError(f"iters must be >= 0, got {iters}")
    if not float(prior_weight) > 0.0:
        raise ValueError("prior_weight must be > 0: 17 keypoints do not determine 22 rotations, "
                         "the prior toward the solved pose is what makes the problem well-posed")
    if not float(lam0) > 0.0:
        raise ValueError(f"lam0 must be > 0, got {lam0}")


def _check_joint_weight(joint_weight, F=None):
    """None, or non-negative weights (17,), with a frame count F also (F,17) -> None or the float32 array."""
    if joint_weight is None:
        return None
    w = np.asarray(joint_weight, np.float32)
    shapes = ((17,),) if F is None else ((17,), (F, 17))
    if w.shape not in shapes or not (w >= 0).all():
        raise ValueError(f"joint_weight must be {' or '.join(map(str, shapes))} non-negative values (COCO order), "
                         f"got shape {w.shape}")
    return w


def check_fused_options(fused, robust_sigma, skip_nonfinite):
    """refine_poses' options for imperfect detections -> (sigma, skip). They exist in the fused kernel only: either
    one given with fused=False is a ValueError, as is a robust_sigma that is negative or not finite."""
    sigma, flags = check_robust_args(robust_sigma, skip_nonfinite)
    if not fused and (sigma > 0.0 or flags):
        raise ValueError("robust_sigma and skip_nonfinite need fused=True: the launched loops have no robust term "
                         "(refine_smooth treats non-finite keypoints as missing on its own)")
    return sigma, bool(flags)


def _check_prior_poses(prior_poses, F):
    if prior_poses is not None:
        q = np.asarray(prior_poses)
        if q.ndim != 2 or q.shape[0] != F or q.shape[1] < NUM_DOF:
            raise ValueError(f"prior_poses must be ({F}, >= {NUM_DOF}), got {q.shape}")


def _check_shape_args(smplx_model, betas, shape_weight):
    """The ValueErrors of the shape step."""
    if not float(shape_weight) > 0.0:
        raise ValueError("shape_weight must be > 0: a short or static sequence does not determine 10 shape values, "
                         "the prior toward the mean shape is what keeps the summed system positive definite")
    if betas is not None:
        b = np.asarray(betas)
        nb = getattr(smplx_model, "num_betas", None)
        if b.ndim != 1 or b.shape[0] < 1 or (nb is not None and b.shape[0] != nb) or not np.isfinite(b).all():
            raise ValueError(f"betas must be ({'nb' if nb is None else nb},) finite values, got shape {b.shape}")


# ---------------------------------------------------------------- the shared pieces
def _upload(smplx_model, poses, seq_3d_kps, prior_poses=None, betas=None):
    """Host arrays -> float32 tensors on the model's device: (theta (F,66), theta0 (F,66): theta itself
    without prior_poses, keypoints (F,17,3), beta (nb,) or None)."""
    dev = smplx_model.device

    def pose(p):
        return torch.as_tensor(np.ascontiguousarray(np.asarray(p, dtype=np.float32)[:, :NUM_DOF]), device=dev)

    th = pose(poses)
    th0 = th if prior_poses is None else pose(prior_poses)
    kps = torch.as_tensor(np.ascontiguousarray(seq_3d_kps, dtype=np.float32), device=dev).reshape(th.shape[0], 17, 3)
    beta = None if betas is None else torch.as_tensor(np.asarray(betas, np.float32)[:smplx_model.num_betas], device=dev)
    return th, th0, kps, beta


def _chunks(F: int):
    """[(first frame, frames)] of the runs of at most inference.MAX_WINDOWS_PER_CALL frames that one
    library call takes; the length is read now, not at import."""
    c = inference.MAX_WINDOWS_PER_CALL
    return [(s, min(c, F - s)) for s in range(0, F, c)]


def _rows(t, s: int, n: int):
    """t[s:s + n]; t itself where that is all of it or t is None (one chunk is the usual case, and
    every slice is a few microseconds of host time in calls that take a few hundred)."""
    return t if t is None or (s == 0 and n == t.shape[0]) else t[s:s + n]


def _joined(parts, dim: int):
    """torch.cat(parts, dim), without the copy where there is one part."""
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim)


class _FKView:
    """The FK of a run of n frames against their keypoints (n,17,3), all with the body shape beta
    ((nb,) device tensor, None: the mean shape): the residual r of the module docstring and its
    Jacobians, rows made root-relative. th is always (n,66) on the device; the library sees the
    frames in _chunks."""

    def __init__(self, smplx_model, kps, beta=None):
        self.model, self.n = smplx_model, kps.shape[0]
        self.target = _rel(kps)
        self.chunks = _chunks(self.n)
        self.full = torch.zeros((self.n, 55, 3), device=kps.device)   # the hands, jaw and eyes stay zero
        self.set_beta(beta)

    def set_beta(self, beta):
        """Another body shape for the same frames and keypoints."""
        self.betas = None if beta is None else beta[None].expand(self.n, -1).contiguous()

    def _inputs(self, th):
        """-> per chunk (first frame, frames, full_pose rows, betas rows)."""
        self.full[:, :22] = th.reshape(self.n, 22, 3)
        return [(s, n, _rows(self.full, s, n), _rows(self.betas, s, n)) for s, n in self.chunks]

    def coco(self, th):
        """-> FK COCO-17 joints (n,17,3)."""
        out = torch.empty((self.n, 17, 3), device=th.device)
        for s, n, full, b in self._inputs(th):
            self.model.joints(full, b, None, None, select="coco", out=_rows(out, s, n))
        return out

    def _residual_of(self, joints, s=0):
        return _rel(joints) - _rows(self.target, s, joints.shape[0])

    def residual(self, th):
        """-> r (n,17,3)."""
        return self._residual_of(self.coco(th))

    def _linearize(self, jacobian, th, k):
        def one(s, n, full, b):
            jac, joints = jacobian(full, b, None, None, select="coco")
            return (_rel(jac.reshape(n, 17, 3, k)).reshape(n, 51, k).contiguous(),
                    self._residual_of(joints, s).reshape(n, 51).contiguous())
        parts = self._inputs(th)
        if len(parts) == 1:                  # nothing to put together: no copy
            return one(*parts[0])
        jr, r = torch.empty((self.n, 51, k), device=th.device), torch.empty((self.n, 51), device=th.device)
        for s, n, full, b in parts:
            jr[s:s + n], r[s:s + n] = one(s, n, full, b)
        return jr, r

    def linearize(self, th):
        """-> (J (n,51,66) with respect to th, r (n,51))."""
        return self._linearize(self.model.joints_jacobian, th, NUM_DOF)

    def linearize_shape(self, th):
        """-> (Jb (n,51,nb) with respect to the betas, r (n,51))."""
        return self._linearize(self.model.joints_shape_jacobian, th, self.model.num_betas)


def _data_term(r, w=None, per_frame: bool = True):
    """1/2 sum_k w_k |r_k|^2: r (n,17,3) or (n,51), w None (one), (17,) or (n,17) -> (n,) per frame,
    or the 0-d sum over all n frames."""
    sq = r.reshape(-1, 17, 3).square().sum(2)
    sq = sq if w is None else sq * w
    return 0.5 * (sq.sum(1) if per_frame else sq.sum())


def _lm_loop(th, cost, lam, iters, step, cost_of, frames_of):
    """The Levenberg-Marquardt policy. A unit is what is accepted or rejected as a whole and has
    one lambda: a frame, or a sequence of frames. th (n,k) the starting poses, cost (units,)
    their cost, lam (units,); step(th, lam) -> delta (n,k); cost_of(th) -> (units,);
    frames_of(ok (units,) bool) -> (n,) bool, each frame's verdict. Per iteration: the candidate
    th + delta is kept for the units whose cost fell (lambda <- lambda / 3), the old poses for the
    others (lambda <- 3 lambda); a NaN cost is no fall. -> (poses (n,k), history (iters+1, units):
    row 0 `cost`, row it + 1 the cost after iteration it; it never increases). Pure torch."""
    hist = cost.new_empty((iters + 1,) + tuple(cost.shape))
    hist[0] = cost
    for it in range(iters):
        cand = th + step(th, lam)
        cc = cost_of(cand)
        ok = cc < cost   # False for a NaN step
        th = torch.where(frames_of(ok)[:, None], cand, th)
        cost = torch.where(ok, cc, cost)
        lam = torch.where(ok, lam / 3.0, lam * 3.0)
        hist[it + 1] = cost
    return th, hist


# ---------------------------------------------------------------- the drivers
def refine_poses(poses, seq_3d_kps, smplx_model, betas=None, iters: int = 10, prior_weight: float = 1e-2,
                 joint_weight=None, lam0: float = 1e-2, prior_poses=None, fused: bool = False, robust_sigma: float = 0.0,
                 skip_nonfinite: bool = False) -> dict:
    """poses (F,66) solved by the IK, seq_3d_kps (F,17,3) COCO -> {"poses": (F,66)
    float32 numpy, "cost": (iters+1, F) host array of the cost per frame}
    (cost[0] is theta0's, each later row the accepted pose's after that
    iteration; it never increases). prior_poses: None (the prior pulls toward
    `poses`) or (F,66), the theta0 of the cost when `poses` is a later iterate.

    Per frame and iteration (_lm_loop, a frame the unit): the LM step from the
    current pose, the candidate's cost with SMPLX.joints, accepted where the
    cost fell (lambda <- lambda / 3), the old pose kept elsewhere (lambda <- 3
    lambda); a NaN step counts as rejected. All on the device with torch.where,
    no host round trip inside an iteration; the cost history is copied once at
    the end. Frames go through in chunks of at most
    inference.MAX_WINDOWS_PER_CALL, all iterations of one chunk before the
    next, so the Jacobians of one chunk are all that is resident.

    fused=True: the same problem and policy with all iterations of a chunk in
    one SMPLX.refine_frames call (tik_fk_refine: one launch, one workgroup per
    frame, nothing but the poses and the cost rows leaves the chip) instead of
    about five launches and a dozen torch ops per iteration. The same dict; the
    sums run in another order, so the values agree to fp32 rounding, not bit
    for bit. The default path and its bits are untouched. Measured at 4096
    frames the launched path is the faster one per iteration (0.70 against
    1.38 ms): the fused kernel is for the stream and for calls
    that launches, not throughput, bound.

    robust_sigma > 0 and skip_nonfinite=True (fused=True only, ValueError
    otherwise): SMPLX.refine_frames' Geman-McClure data term, and non-finite
    keypoints treated as missing instead of freezing their frame."""
    F = _check_frames(poses, seq_3d_kps)
    _check_lm_scalars(iters, prior_weight, lam0)
    w = _check_joint_weight(joint_weight)
    _check_prior_poses(prior_poses, F)
    sigma, skip = check_fused_options(fused, robust_sigma, skip_nonfinite)
    iters, pw = int(iters), float(prior_weight)
    th_all, pr_all, kps, beta = _upload(smplx_model, poses, seq_3d_kps, prior_poses, betas)
    dev = th_all.device
    wj = None if w is None else torch.as_tensor(w, device=dev)
    row_w = None if wj is None else wj.repeat_interleave(3).contiguous()
    out, hist = [], []

    if fused:
        for s, n in _chunks(F):
            th, cost = smplx_model.refine_frames(_rows(th_all, s, n), _rows(kps, s, n), betas=beta,
                                                 prior=None if prior_poses is None else _rows(pr_all, s, n),
                                                 joint_weight=wj, iters=iters, mu=pw, lam0=float(lam0), robust_sigma=sigma,
                                                 skip_nonfinite=skip)
            out.append(th)
            hist.append(cost.t().contiguous())
        return {"poses": _joined(out, 0).cpu().numpy(), "cost": _joined(hist, 1).cpu().numpy()}

    with torch.no_grad():
        for s, n in _chunks(F):
            fk = _FKView(smplx_model, _rows(kps, s, n), beta)
            th0 = _rows(pr_all, s, n)

            def cost_of(th):
                return _data_term(fk.residual(th), wj) + 0.5 * pw * (th - th0).square().sum(1)

            def step(th, lam):
                jr, r = fk.linearize(th)
                return lm_solve(jr, r, lam, mu=pw, prior=(th - th0).contiguous(), row_weight=row_w)

            th = _rows(th_all, s, n)
            lam = torch.full((n,), float(lam0), device=dev)
            th, h = _lm_loop(th, cost_of(th), lam, iters, step, cost_of, lambda ok: ok)
            out.append(th)
            hist.append(h)
    return {"poses": _joined(out, 0).cpu().numpy(), "cost": _joined(hist, 1).cpu().numpy()}


def _frame_weights(joint_weight, seq_3d_kps, F):
    """joint_weight None, (17,) or (F,17) and keypoints (F,17,3) that may hold non-finite values ->
    (weights (F,17) float32, or None where every weight is one; keypoints float32 with the missing ones
    zeroed). ValueError on a bad shape or a negative weight. Host only."""
    kps = np.array(seq_3d_kps, dtype=np.float32).reshape(F, 17, 3)
    w = _check_joint_weight(joint_weight, F)
    seen = np.isfinite(kps).all(2)
    if not seen.all():
        w = np.ones((F, 17), np.float32) if w is None else np.broadcast_to(w, (F, 17)).copy()
        w[~seen] = 0.0
        w[~(seen[:, 11] & seen[:, 12])] = 0.0    # rel() needs both hips: without them the frame is missing
        kps[~seen] = 0.0
    elif w is not None:
        w = np.broadcast_to(w, (F, 17)).copy()
    return w, kps


def refine_smooth(poses, seq_3d_kps, smplx_model, smooth_weight, betas=None, iters: int = 10,
                  prior_weight: float = 1e-2, joint_weight=None, lam0: float = 1e-2, prior_poses=None,
                  seq_starts=None) -> dict:
    """refine_poses with neighbouring frames tied together: poses (F,66) solved by
    the IK, seq_3d_kps (F,17,3) COCO -> {"poses": (F,66) float32 numpy, "cost":
    (iters+1, S) host array of the cost per sequence}. seq_starts: None (one
    sequence) or S+1 frame indices (smplx_fk.lm_chain_starts). Per sequence

        cost = sum_f [ 1/2 sum_k w_fk |r_fk|^2 + 1/2 prior_weight |theta_f - theta0_f|^2 ]
               + 1/2 smooth_weight sum_f |theta_{f+1} - theta_f|^2

    the first sum refine_poses's cost, the second over the neighbours inside
    the sequence. The smoothness is on the axis-angle values themselves: it
    assumes consecutive frames are far from the +-pi wrap of a rotation vector,
    which holds for the network's output. smooth_weight > 0 has no default:
    nobody has measured a good one on real data, the caller chooses.

    joint_weight: None, (17,) or (F,17) non-negative, so a frame's undetected
    keypoints can be switched off. A non-finite keypoint counts as missing: its
    weight becomes 0 and its coordinates are zeroed before the upload. A frame
    whose COCO 11 or 12 is non-finite is missing entirely (rel needs both
    hips): all its 17 weights become 0, its pose comes from the neighbours and
    the prior.

    Per iteration (_lm_loop, a sequence the unit): the FK Jacobians of all F
    frames, (F,51,66), the library called in chunks of
    inference.MAX_WINDOWS_PER_CALL, one smplx_fk.lm_solve_chain call (block
    tridiagonal, one workgroup per sequence), the candidate's cost with
    SMPLX.joints, accepted per sequence where its cost fell (lambda <- lambda /
    3), the old poses kept elsewhere (lambda <- 3 lambda); a NaN step counts as
    rejected. One lambda per sequence. The sums per sequence are taken over a
    padded (S, longest) gather, so a sequence's cost, and with it its poses,
    do not depend on the other sequences. All on the device, no host round
    trip inside an iteration; cost never increases."""
    sw = float(smooth_weight)
    if not sw > 0.0:
        raise ValueError(f"smooth_weight must be > 0, got {smooth_weight}: refine_poses is the refinement "
                         "without the smoothness term")
    F = _check_frames(poses, seq_3d_kps)
    _check_lm_scalars(iters, prior_weight, lam0)
    _check_prior_poses(prior_poses, F)
    w_np, kps_np = _frame_weights(joint_weight, seq_3d_kps, F)
    starts = lm_chain_starts(F, seq_starts)
    iters, pw = int(iters), float(prior_weight)
    S = starts.shape[0] - 1
    lengths = np.diff(starts).astype(np.int64)
    longest = int(lengths.max())
    pad = starts[:-1, None].astype(np.int64) + np.arange(longest)[None]          # (S, longest) frame of each slot
    live = np.arange(longest)[None] < lengths[:, None]
    last = np.zeros(F, bool)
    last[starts[1:] - 1] = True

    th, th0, kps, beta = _upload(smplx_model, poses, kps_np, prior_poses, betas)
    dev = th.device
    wj = None if w_np is None else torch.as_tensor(w_np, device=dev)
    row_w = None if wj is None else wj.repeat_interleave(3, dim=1).contiguous()
    starts_d = torch.as_tensor(starts, device=dev)
    seg = torch.as_tensor(np.repeat(np.arange(S), lengths), device=dev)
    pad_d = torch.as_tensor(np.where(live, pad, 0), device=dev)
    live_d = torch.as_tensor(live, device=dev)
    tie = torch.as_tensor((~last[:-1]).astype(np.float32), device=dev)            # frame f has f + 1 in its sequence

    with torch.no_grad():
        fk = _FKView(smplx_model, kps, beta)
        work = torch.empty((lm_chain_workspace_floats(F, NUM_DOF),), device=dev)

        def cost_of(t):
            per = _data_term(fk.residual(t), wj) + 0.5 * pw * (t - th0).square().sum(1)
            if F > 1:
                per[:-1] += 0.5 * sw * tie * (t[1:] - t[:-1]).square().sum(1)
            return torch.where(live_d, per[pad_d], torch.zeros((), device=dev)).sum(1)

        def step(t, lam):
            jr, r = fk.linearize(t)
            return lm_solve_chain(jr, r, lam, t, sw, mu=pw, prior=(t - th0).contiguous(), row_weight=row_w,
                                  seq_starts=starts_d, workspace=work)

        lam = torch.full((S,), float(lam0), device=dev)
        th, hist = _lm_loop(th, cost_of(th), lam, iters, step, cost_of, lambda ok: ok[seg])
    return {"poses": th.cpu().numpy(), "cost": hist.cpu().numpy()}


def fit_shape(poses, seq_3d_kps, smplx_model, betas=None, shape_weight: float = 1e-3, joint_weight=None) -> dict:
    """poses (F,66), seq_3d_kps (F,17,3) COCO -> {"betas": (nb,) float32 numpy,
    "cost": (2,) host array}: the betas that minimise, for the given poses,
    1/2 sum_f sum_k w_k |r_fk|^2 + 1/2 shape_weight |beta|^2, and that cost
    before and after. One exact step from `betas` (None: zero): the joints are
    affine in beta, so the minimiser does not depend on where the step starts.
    Frames go through in chunks of at most inference.MAX_WINDOWS_PER_CALL, each
    into its own rows of one buffer of partial sums (lm_accumulate), solved
    once (lm_solve_sum with mu = shape_weight and prior = beta); the data term
    is summed chunk by chunk too. A step that is NaN is returned as it is;
    refine_sequence rejects it."""
    F = _check_frames(poses, seq_3d_kps)
    w = _check_joint_weight(joint_weight)
    _check_shape_args(smplx_model, betas, shape_weight)
    sw = float(shape_weight)
    nb = smplx_model.num_betas
    th, _, kps, beta = _upload(smplx_model, poses, seq_3d_kps, betas=betas)
    dev = th.device
    wj = None if w is None else torch.as_tensor(w, device=dev)
    row_w = None if wj is None else wj.repeat_interleave(3).contiguous()
    if beta is None:
        beta = torch.zeros((nb,), device=dev)
    with torch.no_grad():
        chunks = _chunks(F)
        rows = [(n + LM_RUN - 1) // LM_RUN for _, n in chunks]
        partial = torch.empty((sum(rows), lm_partial_width(nb)), device=dev)

        views = [(_FKView(smplx_model, _rows(kps, s, n), beta), _rows(th, s, n)) for s, n in chunks]
        data0 = data1 = torch.zeros((), device=dev)
        for (fk, t), out in zip(views, partial.split(rows)):
            jr, r = fk.linearize_shape(t)
            lm_accumulate(jr, r, row_weight=row_w, out=out)
            data0 = data0 + _data_term(r, wj, per_frame=False)
        new = beta + lm_solve_sum(partial, mu=sw, lam=0.0, prior=beta.contiguous(), n=nb)
        for fk, t in views:
            fk.set_beta(new)
            data1 = data1 + _data_term(fk.residual(t), wj, per_frame=False)
        c0 = data0 + 0.5 * sw * beta.square().sum()
        c1 = data1 + 0.5 * sw * new.square().sum()
    return {"betas": new.cpu().numpy(), "cost": torch.stack([c0, c1]).cpu().numpy()}


def refine_sequence(poses, seq_3d_kps, smplx_model, rounds: int = 3, iters: int = 5, prior_weight: float = 1e-2,
                    shape_weight: float = 1e-3, joint_weight=None, lam0: float = 1e-2, betas=None,
                    smooth_weight: float = 0.0) -> dict:
    """poses (F,66) solved by the IK, seq_3d_kps (F,17,3) COCO -> {"poses": (F,66)
    float32, "betas": (nb,) float32, "cost": (rounds+1,)}: `rounds` rounds of
    one shape step (fit_shape) followed by `iters` pose iterations
    (refine_poses with the round's betas). cost is the total cost of the module
    docstring, cost[0] that of the inputs; it never increases: new betas are
    kept only where the total cost fell (a NaN step is rejected), and
    refine_poses never raises a frame's cost. The pose prior stays anchored at
    the input poses theta0 through all rounds. betas: the starting shape, None
    = zero. rounds=0 returns the inputs. smooth_weight > 0: the pose iterations
    are refine_smooth's (the frames one sequence, 1/2 smooth_weight
    sum_f |theta_{f+1} - theta_f|^2 part of the cost); 0 changes nothing."""
    _check_frames(poses, seq_3d_kps)
    _check_lm_scalars(iters, prior_weight, lam0)
    _check_joint_weight(joint_weight)
    _check_shape_args(smplx_model, betas, shape_weight)
    smooth = float(smooth_weight)
    if not smooth >= 0.0:
        raise ValueError(f"smooth_weight must be >= 0, got {smooth_weight}")
    if int(rounds) < 0:
        raise ValueError(f"rounds must be >= 0, got {rounds}")
    rounds, sw, pw = int(rounds), float(shape_weight), float(prior_weight)
    nb = smplx_model.num_betas
    th0 = np.ascontiguousarray(np.asarray(poses, dtype=np.float32)[:, :NUM_DOF])
    beta = np.zeros(nb, np.float32) if betas is None else np.asarray(betas, np.float32).copy()
    th = th0.copy()

    def frames(th_np, beta_np, n_it):
        if smooth > 0.0:
            return refine_smooth(th_np, seq_3d_kps, smplx_model, smooth, betas=beta_np, iters=n_it, prior_weight=pw,
                                 joint_weight=joint_weight, lam0=lam0, prior_poses=th0)
        return refine_poses(th_np, seq_3d_kps, smplx_model, betas=beta_np, iters=n_it, prior_weight=pw,
                            joint_weight=joint_weight, lam0=lam0, prior_poses=th0)

    def total(per_frame, beta_np):
        # per frame (per sequence with smooth_weight) the terms as refine_poses (refine_smooth) itself
        # computes them: its history never increases, so neither does this sum
        return float(per_frame.astype(np.float64).sum()) + 0.5 * sw * float(np.square(beta_np.astype(np.float64)).sum())

    cost = [total(frames(th, beta, 0)["cost"][0], beta)]
    for _ in range(rounds):
        cand = fit_shape(th, seq_3d_kps, smplx_model, betas=beta, shape_weight=sw, joint_weight=joint_weight)["betas"]
        if np.isfinite(cand).all() and total(frames(th, cand, 0)["cost"][0], cand) < cost[-1]:
            beta = cand
        out = frames(th, beta, iters)
        th = out["poses"]
        cost.append(total(out["cost"][-1], beta))
    return {"poses": th, "betas": beta, "cost": np.asarray(cost)}
