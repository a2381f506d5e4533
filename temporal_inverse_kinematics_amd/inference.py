"""Entry point — drop-in for `inference.py` (`run_inference` :37-67, `run_test`
:110-149). Windows are gathered on the GPU (tik_window_gather) and the whole
sequence is solved in large batches by the fused HIP forward; like the
reference, each window's output frame 0 is the solution for frame idx
(inference.py:58-66, h_w_size = 0).

CLI (README.md:24-26):
    python -m temporal_inverse_kinematics_amd.inference <moveai_3d.npz> [SMPLX_DIR]
        [--ckpt model.ckpt] [--win-size 64] [--out poses.npy] [--check] [--refine N]
        [--fit-shape R] [--smooth W] [--robust S] [--metrics]
Without --ckpt the seeded synthetic weights are used (the trained checkpoint
is not distributed with the reference: .MISSING_LARGE_BLOBS:2).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np
import torch

from . import keypoints as kp
from .windowing import gather_windows

MAX_WINDOWS_PER_CALL = 8192


def run_inference(model, seq_3d_kps: np.ndarray) -> np.ndarray:
    """(F,17,3) keypoints -> (F,66) f32 SMPL-X body pose (inference.py:37-67)."""
    win = model.hparams.win_size
    dev = model.device
    if isinstance(seq_3d_kps, torch.Tensor):
        seq = seq_3d_kps.to(dev, torch.float32).contiguous()
    else:
        seq = torch.as_tensor(np.ascontiguousarray(seq_3d_kps, dtype=np.float32), device=dev)
    F = seq.shape[0]
    out = np.empty((F, 66), dtype=np.float32)
    with torch.no_grad():
        for s in range(0, F, MAX_WINDOWS_PER_CALL):
            n = min(MAX_WINDOWS_PER_CALL, F - s)
            windows = gather_windows(seq, win, idx0=s, n=n, relative_pose=True)
            poses = model(windows)["poses"]
            out[s:s + n] = poses[:, 0].float().cpu().numpy()
    return out


def synthetic_model(win_size: int = 64, device="cuda", seed: int = 0, precision=None):
    """IKPoseTrainer with the seeded synthetic weights of synthetic.ik_state_dict."""
    from . import synthetic as syn
    from .models import IKPoseTrainer, default_hparams
    model = IKPoseTrainer(default_hparams(win_size))
    sd = syn.ik_state_dict(model.regressor.backbone.graph.A, seed=seed)
    model.regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    model.regressor.tik_precision = precision
    return model.to(device).eval()


def fk_check(poses, seq_3d_kps, smplx_model, betas=None) -> dict:
    """How far the solved poses' FK lands from the keypoints they were solved
    from: poses (F,66), seq_3d_kps (F,17,3) COCO. The FK COCO-17 joints (the
    pose layout of run_test: hands zero, no translation; SMPLX.joints, no
    mesh) and the keypoints are both made root-relative (mean of COCO 11/12,
    the hips). -> {"per_joint": (F,17) distances on the host, "mpjpe": (F,),
    "mean": float}."""
    from .refine import _FKView, _upload
    th, _, kps, beta = _upload(smplx_model, poses, seq_3d_kps, betas=betas)
    with torch.no_grad():
        per_joint = _FKView(smplx_model, kps, beta).residual(th).norm(dim=2).cpu().numpy()
    mpjpe = per_joint.mean(axis=1)
    return {"per_joint": per_joint, "mpjpe": mpjpe, "mean": float(mpjpe.mean())}


def _nanmean(v: np.ndarray) -> float:
    """The mean over the finite entries; NaN where there is none (the mean over nothing)."""
    ok = np.isfinite(v)
    return float(v[ok].mean()) if ok.any() else float("nan")


def evaluate_poses(poses, seq_3d_kps, smplx_model, betas=None, target_poses=None, joint_weight=None,
                   seq_starts=None) -> dict:
    """The metrics a pose regressor is judged by, per frame, on the device
    (SMPLX.pose_metrics, one launch per run of MAX_WINDOWS_PER_CALL frames): poses
    (F,66), seq_3d_kps (F,17,3) COCO, both made root-relative as in fk_check.
    -> {"mpjpe", "pa_mpjpe", "mpjae", "weight", "accel": (F,) host arrays, and
    "mpjpe_mean", "pa_mpjpe_mean", "mpjae_mean", "accel_mean": their means over the
    frames that have a value (NaN where none has)}. mpjpe and pa_mpjpe in metres
    (pa_mpjpe after the best similarity transform with a proper rotation), mpjae
    in radians against target_poses (F,66) (NaN without them). accel: the
    acceleration error mean_k |(x_{f+1} - 2 x_f + x_{f-1}) - (y_{f+1} - 2 y_f + y_{f-1})|
    of the FK keypoints x and the keypoints y, for the interior frames of each
    sequence (NaN on a sequence's first and last frame); seq_starts: None (one
    sequence) or S+1 frame indices (smplx_fk.lm_chain_starts). betas: None,
    (nb,) or (F,nb); joint_weight: None, (17,) or (F,17) non-negative. A
    non-finite keypoint counts as missing (weight 0); a frame without both hips
    has weight 0 and no mpjpe."""
    from .refine import _check_joint_weight, _chunks, _rows, _upload
    from .smplx_fk import lm_chain_starts
    F = int(np.asarray(poses).shape[0])
    starts = lm_chain_starts(F, seq_starts)
    w = _check_joint_weight(joint_weight, F)
    b = None if betas is None else np.asarray(betas, np.float32)
    if b is not None and b.ndim == 2 and b.shape[0] != F:
        raise ValueError(f"betas must be (nb,) or ({F}, nb), got {b.shape}")
    th, _, kps, _ = _upload(smplx_model, poses, seq_3d_kps)
    dev = th.device
    nb = smplx_model.num_betas
    beta = None if b is None else torch.as_tensor(np.ascontiguousarray(b[..., :nb]), device=dev)
    tgt = None
    if target_poses is not None:
        t = np.asarray(target_poses, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] != F or t.shape[1] < 66:
            raise ValueError(f"target_poses must be ({F}, >= 66), got {t.shape}")
        tgt = torch.as_tensor(np.ascontiguousarray(t[:, :66]), device=dev)
    wd = None if w is None else torch.as_tensor(w, device=dev)
    out = torch.empty((F, 4), device=dev, dtype=torch.float32)
    x = torch.empty((F, 17, 3), device=dev, dtype=torch.float32)
    with torch.no_grad():
        for s, n in _chunks(F):
            smplx_model.pose_metrics(_rows(th, s, n), _rows(kps, s, n),
                                     betas=beta if beta is None or beta.dim() == 1 else _rows(beta, s, n),
                                     joint_weight=wd if wd is None or wd.dim() == 1 else _rows(wd, s, n),
                                     target_poses=_rows(tgt, s, n), skip_nonfinite=True, out=out[s:s + n],
                                     out_joints=x[s:s + n])
        accel = torch.full((F,), float("nan"), device=dev)
        e = x - (kps - 0.5 * (kps[:, 11:12] + kps[:, 12:13]))
        for q in range(len(starts) - 1):
            a, z = int(starts[q]), int(starts[q + 1])
            if z - a >= 3:
                accel[a + 1:z - 1] = (e[a + 2:z] - 2.0 * e[a + 1:z - 1] + e[a:z - 2]).norm(dim=2).mean(dim=1)
    h = out.cpu().numpy()
    res = {"mpjpe": h[:, 0], "pa_mpjpe": h[:, 1], "mpjae": h[:, 2], "weight": h[:, 3], "accel": accel.cpu().numpy()}
    for k in ("mpjpe", "pa_mpjpe", "mpjae", "accel"):
        res[k + "_mean"] = _nanmean(res[k])
    return res


def run_test(npz_path: str, smplx_dir: str | None = None, ckpt: str | None = None, win_size: int = 64,
             device="cuda", check: bool = False, refine: int = 0, fit_shape: int = 0, smooth: float = 0.0,
             robust: float = 0.0, metrics: bool = False):
    """inference.run_test:110-145: moveai npz -> COCO -> IK -> (optional) SMPL-X FK.
    check=True (with an SMPL-X dir): the result gains "fk_check" (fk_check above).
    refine=N > 0 (with an SMPL-X dir): N Levenberg-Marquardt iterations on the
    solved poses (refine.refine_poses); the result gains "poses_refined" and,
    with check, "fk_check_refined". refine=0 leaves every output as it is.
    fit_shape=R > 0 (with an SMPL-X dir and refine=N > 0): R rounds of one shape
    step and N pose iterations (refine.refine_sequence); the result gains
    "betas", "poses_refined" comes from those rounds and "fk_check_refined" is
    taken with those betas. fit_shape=0 leaves every output as it is.
    smooth=W > 0 (with an SMPL-X dir and refine=N > 0): the pose iterations tie
    neighbouring frames with 1/2 W sum_f |theta_{f+1} - theta_f|^2
    (refine.refine_smooth, the track one sequence), alone or inside the rounds
    of fit_shape; the output keys are those of refine. smooth=0 leaves every
    output as it is.
    robust=S > 0 (with an SMPL-X dir and refine=N > 0, without fit_shape and
    smooth): the N iterations run in the fused kernel (refine_poses(fused=True))
    with the Geman-McClure scale S in metres and non-finite keypoints treated
    as missing. There is no tuned S; robust=0 leaves every output as it is.
    metrics=True (with an SMPL-X dir): the result gains "metrics"
    (evaluate_poses of the solved poses against the keypoints) and, where poses
    were refined, "metrics_refined". metrics=False leaves every output as it is."""
    if refine < 0:
        raise ValueError(f"refine must be >= 0, got {refine}")
    if fit_shape < 0:
        raise ValueError(f"fit_shape must be >= 0, got {fit_shape}")
    if fit_shape and not (smplx_dir and refine > 0):
        raise ValueError("fit_shape needs an SMPL-X dir (or 'synthetic') and refine=N > 0, the pose iterations per round")
    if not smooth >= 0:
        raise ValueError(f"smooth must be >= 0, got {smooth}")
    if smooth and not (smplx_dir and refine > 0):
        raise ValueError("smooth needs an SMPL-X dir (or 'synthetic') and refine=N > 0, the pose iterations it smooths")
    if refine and not smplx_dir:
        raise ValueError("refine needs an SMPL-X dir (or 'synthetic'): the refinement runs the FK")
    if not (robust >= 0 and robust < float("inf")):
        raise ValueError(f"robust must be >= 0 and finite, got {robust}")
    if robust and (not (smplx_dir and refine > 0) or fit_shape or smooth):
        raise ValueError("robust needs an SMPL-X dir (or 'synthetic') and refine=N > 0, and neither fit_shape nor smooth: "
                         "the robust term lives in the fused kernel, not in the launched loops")
    if metrics and not smplx_dir:
        raise ValueError("metrics needs an SMPL-X dir (or 'synthetic'): the metrics run the FK")
    d = np.load(npz_path, allow_pickle=False)
    # the moveai_3d -> COCO conversion on the device (one gather kernel, bit-identical to the host form)
    seq = kp.moveai3d_to_coco_device(torch.as_tensor(np.ascontiguousarray(d["joints_3d"], dtype=np.float32),
                                                     device=device), d["joint_3d_names"].tolist())
    if ckpt:
        from .models import IKPoseTrainer
        model = IKPoseTrainer.load_from_checkpoint(ckpt).to(device).eval()
    else:
        model = synthetic_model(win_size, device)
    poses = run_inference(model, seq)
    result = {"coco": seq.cpu().numpy(), "poses": poses}
    if smplx_dir:
        from .smplx_fk import load_smplx_models, run_smpl_inference
        models = load_smplx_models(smplx_dir, device, 9)
        sample = np.zeros((poses.shape[0], 156), dtype=np.float32)
        sample[:, :66] = poses
        joints, verts = run_smpl_inference({"poses": sample, "gender": "male"}, models, device,
                                           apply_trans=False, apply_shape=False, return_mesh=True)
        result.update(joints=joints, vertices=verts)
        if check:
            result["fk_check"] = fk_check(poses, result["coco"], models["male"])
        if refine and fit_shape:
            from .refine import refine_sequence
            seq_fit = refine_sequence(poses, result["coco"], models["male"], rounds=fit_shape, iters=refine,
                                      smooth_weight=smooth)
            result.update(poses_refined=seq_fit["poses"], betas=seq_fit["betas"])
            if check:
                result["fk_check_refined"] = fk_check(result["poses_refined"], result["coco"], models["male"],
                                                      betas=result["betas"])
        elif refine:
            from .refine import refine_poses, refine_smooth
            if smooth:
                result["poses_refined"] = refine_smooth(poses, result["coco"], models["male"], smooth, iters=refine)["poses"]
            elif robust:
                result["poses_refined"] = refine_poses(poses, result["coco"], models["male"], iters=refine, fused=True,
                                                       robust_sigma=robust, skip_nonfinite=True)["poses"]
            else:
                result["poses_refined"] = refine_poses(poses, result["coco"], models["male"], iters=refine)["poses"]
            if check:
                result["fk_check_refined"] = fk_check(result["poses_refined"], result["coco"], models["male"])
        if metrics:
            result["metrics"] = evaluate_poses(poses, result["coco"], models["male"])
            if "poses_refined" in result:
                result["metrics_refined"] = evaluate_poses(result["poses_refined"], result["coco"], models["male"],
                                                           betas=result.get("betas"))
    return result


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("npz")
    p.add_argument("smplx_dir", nargs="?")
    p.add_argument("--ckpt")
    p.add_argument("--win-size", type=int, default=64)
    p.add_argument("--out")
    p.add_argument("--check", action="store_true",
                   help="with SMPLX_DIR: compare the FK joints of the solved poses with the input keypoints")
    p.add_argument("--refine", type=int, default=0, metavar="N",
                   help="with SMPLX_DIR: N Levenberg-Marquardt iterations pulling the FK joints of the solved "
                        "poses onto the keypoints (--out then saves the refined poses)")
    p.add_argument("--fit-shape", type=int, default=0, metavar="R",
                   help="with SMPLX_DIR and --refine N: R rounds of one body-shape solve shared by all frames followed "
                        "by N pose iterations (--out X.npy then also saves the betas to X.betas.npy)")
    p.add_argument("--smooth", type=float, default=0.0, metavar="W",
                   help="with SMPLX_DIR and --refine N: the pose iterations tie neighbouring frames with the weight W on "
                        "the squared difference of their poses (one block-tridiagonal solve for the whole track)")
    p.add_argument("--robust", type=float, default=0.0, metavar="S",
                   help="with SMPLX_DIR and --refine N (without --fit-shape and --smooth): the iterations run in the fused "
                        "kernel with a Geman-McClure data term of scale S metres, and non-finite keypoints count as missing")
    p.add_argument("--metrics", action="store_true",
                   help="with SMPLX_DIR: print mpjpe, pa_mpjpe (metres) and the acceleration error of the solved poses "
                        "against the input keypoints, and with --refine N those of the refined poses")
    return p


def _betas_path(out: str) -> str:
    """poses X.npy -> X.betas.npy (numpy appends .npy to a name without it)."""
    return (out[:-4] if out.endswith(".npy") else out) + ".betas.npy"


def main(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if a.refine < 0 or (a.refine and not a.smplx_dir):
        p.error("--refine N needs N >= 0 and an SMPLX_DIR")
    if a.fit_shape < 0 or (a.fit_shape and not (a.smplx_dir and a.refine > 0)):
        p.error("--fit-shape R needs R >= 0, an SMPLX_DIR and --refine N with N > 0 (the pose iterations per round)")
    if not a.smooth >= 0 or (a.smooth and not (a.smplx_dir and a.refine > 0)):
        p.error("--smooth W needs W >= 0, an SMPLX_DIR and --refine N with N > 0 (the pose iterations it smooths)")
    if not (a.robust >= 0 and a.robust < float("inf")) or (a.robust and (not (a.smplx_dir and a.refine > 0) or a.fit_shape or a.smooth)):
        p.error("--robust S needs S >= 0, an SMPLX_DIR and --refine N with N > 0, and neither --fit-shape nor --smooth")
    if a.metrics and not a.smplx_dir:
        p.error("--metrics needs an SMPLX_DIR")
    r = run_test(a.npz, a.smplx_dir, a.ckpt, a.win_size, check=a.check, refine=a.refine, fit_shape=a.fit_shape,
                 smooth=a.smooth, robust=a.robust, metrics=a.metrics)
    if a.out:
        np.save(a.out, r.get("poses_refined", r["poses"]))
        if "betas" in r:
            np.save(_betas_path(a.out), r["betas"])
    print(f"solved {r['poses'].shape[0]} frames -> poses {r['poses'].shape}")
    if "fk_check" in r:
        print(f"FK check: mean root-relative joint distance {r['fk_check']['mean']:.6f}")
    if "poses_refined" in r:
        print(f"refined {r['poses_refined'].shape[0]} frames with {a.refine} LM iterations"
              + (f", smoothness weight {a.smooth:g}" if a.smooth else ""))
    if "betas" in r:
        print(f"fitted {r['betas'].shape[0]} betas in {a.fit_shape} rounds: {np.array2string(r['betas'], precision=3)}")
    if "fk_check_refined" in r:
        print(f"FK check: before {r['fk_check']['mean']:.6f} -> after {r['fk_check_refined']['mean']:.6f}")
    for key, what in (("metrics", "solved"), ("metrics_refined", "refined")):
        if key in r:
            m = r[key]
            print(f"metrics of the {what} poses: mpjpe {m['mpjpe_mean']:.6f} pa_mpjpe {m['pa_mpjpe_mean']:.6f} "
                  f"accel {m['accel_mean']:.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
