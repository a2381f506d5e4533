"""Float64 reference of the fused LM refinement on imperfect detections, shared by tests/test_lm_robust_host.py,
tests/test_gpu_lm_robust.py, tests/test_gpu_stream_conf.py and tests/lm_robust_guard_child.py. Not a test module.
It imports the new Python names at import time, so every module built on it fails to import where the feature is
absent.

lm_refine_ref.lm with weights per frame and keypoint (n,17), the Geman-McClure data term and the missing rule:

    s_k      = |r_k|^2                                   r = rel(oracle COCO-17(th)) - rel(kps)
    rho(s)   = sigma^2 s / (sigma^2 + s)                 (sigma = 0: rho(s) = s)
    cost(th) = 1/2 sum_k w_k rho(s_k) + 1/2 mu |th - th0|^2
    omega_k  = w_k (sigma^2 / (sigma^2 + s_k))^2         from the current pose's residual
    (J^T Omega J + (mu + lam) I) delta = -(J^T Omega r + mu (th - th0))

accept / reject on the robust cost of the candidate, lam / 3 and 3 lam as before. Missing (skip=True,
refine._frame_weights' rule): a keypoint with a non-finite component has weight 0 and target 0; a frame without
column 11 or 12 has all 17 weights 0.

Two scenarios on the inputs of lm_refine_ref.case_refine() (F = 6, seed 3, 10 iterations, mu = lam0 = 1e-2), each
computed once and left unchanged:
  outlier   keypoint 9's x raised by 0.5 in every frame; sigma = 0.1 against sigma = 0
  missing   keypoint 9 NaN in every frame, keypoint 11's z NaN in frame 4
"""
import functools

import numpy as np

import lm_refine_ref as L
from temporal_inverse_kinematics_amd.refine import check_fused_options                        # noqa: F401  (the feature)
from temporal_inverse_kinematics_amd.smplx_fk import REFINE_SKIP_NONFINITE, check_robust_args  # noqa: F401
from temporal_inverse_kinematics_amd.streaming import check_conf, check_stream_robust          # noqa: F401

SIGMA = 0.1
OUT_KP, OUT_SHIFT = 9, 0.5
FILL = 0.25          # the finite stand-in of a missing coordinate in the weights-0 runs: any finite value does


def clean(kps, weights=None):
    """The missing rule -> (kps float64 with the missing keypoints zeroed, weights (n,17))."""
    kps = np.array(kps, np.float64)
    n = kps.shape[0]
    w = np.ones((n, 17)) if weights is None else np.broadcast_to(np.asarray(weights, np.float64), (n, 17)).copy()
    seen = np.isfinite(kps).all(2)
    w[~seen] = 0.0
    w[~(seen[:, 11] & seen[:, 12])] = 0.0
    kps[~seen] = 0.0
    return kps, w


def rho(s, sigma):
    return s if sigma == 0 else sigma * sigma * s / (sigma * sigma + s)


def omega(w, s, sigma):
    """w (.., 17), s = |r_k|^2 (.., 17) -> the IRLS weights."""
    return w if sigma == 0 else w * (sigma * sigma / (sigma * sigma + s)) ** 2


def lm(th0, kps, iters, mu=L.MU, lam0=L.LAM0, weights=None, sigma=0.0, skip=False):
    """th0 (n,66) prior and start, kps (n,17,3), weights None, (17,) or (n,17) -> {"th": (n,66), "hist": (iters+1, n)}."""
    th0 = np.asarray(th0, np.float64)
    n = th0.shape[0]
    if skip:
        kps, w = clean(kps, weights)
    else:
        kps = np.asarray(kps, np.float64)
        w = np.ones((n, 17)) if weights is None else np.broadcast_to(np.asarray(weights, np.float64), (n, 17))
    target = L.rel(kps)

    def resid(th):
        return L.rel(L.coco_of(th)) - target                      # (n,17,3)

    def cost_of(r, th):
        return 0.5 * (w * rho((r * r).sum(2), sigma)).sum(1) + 0.5 * mu * ((th - th0) ** 2).sum(1)

    th, lam = th0.copy(), np.full(n, lam0)
    cost = cost_of(resid(th), th)
    hist = [cost.copy()]
    for _ in range(iters):
        J = L.jacobian(th)
        r = resid(th)
        om3 = np.repeat(omega(w, (r * r).sum(2), sigma), 3, axis=1)   # (n,51)
        r = r.reshape(n, 51)
        cand = th.copy()
        for b in range(n):
            N = (J[b].T * om3[b]) @ J[b] + (mu + lam[b]) * np.eye(66)
            cand[b] += np.linalg.solve(N, -((J[b].T * om3[b]) @ r[b] + mu * (th[b] - th0[b])))
        cc = cost_of(resid(cand), cand)
        ok = cc < cost
        th = np.where(ok[:, None], cand, th)
        cost = np.where(ok, cc, cost)
        lam = np.where(ok, lam / 3.0, lam * 3.0)
        hist.append(cost.copy())
    return {"th": th, "hist": np.stack(hist)}


def worst_distance(th, kps_clean):
    """Per frame, the largest distance of a root-relative FK keypoint of pose th (n,66), evaluated with the float64
    oracle, to the clean root-relative keypoint -> (n,)."""
    d = L.rel(L.coco_of(th)) - L.rel(np.asarray(kps_clean, np.float64))
    return np.sqrt((d * d).sum(2)).max(1)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def outlier_inputs():
    """-> th0 (6,66) float32, kps with the outlier (6,17,3) float32, the clean kps, iters."""
    c = L.case_refine()
    kps = c["kps"].copy()
    kps[:, OUT_KP, 0] += np.float32(OUT_SHIFT)
    return c["th0"], kps, c["kps"], c["iters"]


@functools.lru_cache(maxsize=None)
def case_outlier():
    """-> inputs, the plain and the robust run, and their worst keypoint distances to the clean truth per frame."""
    th0, kps, kps_clean, iters = outlier_inputs()
    plain, robust = lm(th0, kps, iters), lm(th0, kps, iters, sigma=SIGMA)
    return _frozen({"th0": th0, "kps": kps, "kps_clean": kps_clean, "iters": iters, "plain": plain["th"], "th": robust["th"],
                    "hist": robust["hist"], "d_plain": worst_distance(plain["th"], kps_clean),
                    "d_robust": worst_distance(robust["th"], kps_clean)})


def missing_inputs():
    """-> th0, kps with the NaNs (6,17,3) float32, the same with FILL in their place, the weights (6,17) of the rule, iters."""
    c = L.case_refine()
    kps = c["kps"].copy()
    kps[:, 9] = np.nan
    kps[4, 11, 2] = np.nan
    filled = np.where(np.isfinite(kps), kps, np.float32(FILL)).astype(np.float32)
    w = np.ones((6, 17), np.float32)
    w[:, 9] = 0
    w[4] = 0
    return c["th0"], kps, filled, w, c["iters"]


@functools.lru_cache(maxsize=None)
def case_missing():
    """-> the run with the missing rule ("th", "hist") and the run on finite keypoints with weights 0 ("th_w", "hist_w")."""
    th0, kps, filled, w, iters = missing_inputs()
    a, b = lm(th0, kps, iters, skip=True), lm(th0, filled, iters, weights=w)
    return _frozen({"th0": th0, "kps": kps, "filled": filled, "w": w, "iters": iters, "th": a["th"], "hist": a["hist"],
                    "th_w": b["th"], "hist_w": b["hist"]})


# ---------------------------------------------------------------- the stream's rules, in numpy
def hold_last(frames, conf):
    """tik_stream_push_conf's fill on a sequence whose every keypoint is present in frame 0: frames (F,17,3) that may
    hold non-finite values, conf (F,17) -> (filled (F,17,3) float32, conf with the missing keypoints' set to 0)."""
    frames, conf = np.array(frames, np.float32), np.array(conf, np.float32)
    missing = (conf == 0) | ~np.isfinite(frames).all(2)
    assert not missing[0].any()
    out = frames.copy()
    for f in range(1, len(frames)):
        out[f][missing[f]] = out[f - 1][missing[f]]
    conf[missing] = 0
    return out, conf


def effective_weights(conf, joint_w=None):
    """conf (F,17) after hold_last, joint_w (17,) or None -> the refine launch's weights (F,17) float32: conf * joint_w,
    one fp32 multiply, all 0 in a frame whose conf[11] or conf[12] is 0."""
    conf = np.asarray(conf, np.float32)
    w = conf * (np.ones(17, np.float32) if joint_w is None else np.asarray(joint_w, np.float32))
    w[(conf[:, 11] == 0) | (conf[:, 12] == 0)] = 0
    return w.astype(np.float32)
