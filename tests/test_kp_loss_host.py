"""The keypoint loss on the CPU: the float64 reference of tests/kp_loss_ref.py is pinned by a central difference of
its own loss, and the pure argument checks (trainer.check_kp_args, smplx_fk.check_kp_loss_tensors) raise before any
device work."""
import numpy as np
import pytest
import torch

import kp_loss_ref as K


def test_reference_gradient_is_the_derivative_of_its_loss():
    """g64 = J^T W r against (loss64(th + h e_q) - loss64(th - h e_q)) / 2h, h = 1e-6, on 3 frames with betas and
    per-frame weights. The difference quotient of a float64 loss of size 1 carries about 1e-16 / 1e-6 = 1e-10 of
    rounding and h^2 |loss'''| / 6 ~ 1e-12 of truncation; g64 itself holds J by the same step: 1e-7 leaves room."""
    th, betas, kps = K.inputs65()
    th, betas, kps = th[:3].astype(np.float64), betas[:3], kps[:3]
    w = K.weights65("frame")[1:4]
    ref = K.reference(th, kps, betas, w)
    h = K.R.STEP
    P = np.repeat(th, 132, axis=0)
    q = np.arange(66)
    for b in range(3):
        P[(b * 66 + q) * 2, q] += h
        P[(b * 66 + q) * 2 + 1, q] -= h
    rep = lambda a: np.repeat(a, 132, axis=0)
    l = K.loss64(P, rep(kps), rep(betas), rep(w)).reshape(3, 66, 2)
    fd = (l[:, :, 0] - l[:, :, 1]) / (2 * h)
    err = np.abs(fd - ref["g"]).max()
    print(f"max |g64 - central difference of loss64| = {err:.3e}, max |g64| = {np.abs(ref['g']).max():.3e}")
    assert np.abs(ref["g"]).max() > 1e-2
    assert err < 1e-7


def test_reference_matches_lm_refine_ref_without_betas():
    th, _, kps = K.inputs65()
    assert np.array_equal(K.coco_of(th[:2]), K.L.coco_of(th[:2]))
    assert np.array_equal(K.jacobian(th[:2]), K.L.jacobian(th[:2].astype(np.float64)))
    lb, gb = K.bounds(K.reference(th[:2], kps[:2]))
    assert lb.shape == (2,) and gb.shape == (2, 66) and (lb > 0).all() and (gb > 0).all()


def test_check_kp_args():
    from temporal_inverse_kinematics_amd.trainer import check_kp_args
    assert check_kp_args(0.0, 0) == 0.0 and check_kp_args(0.5, 2) == 0.5 and check_kp_args(0.0, 1) == 0.0
    kps, betas = torch.zeros(4, 2, 17, 3), torch.zeros(4, 10)
    ok = dict(N=4, To=2, num_betas=10, target_keypoints=kps, betas=betas, gender_id=np.array([0, 1, 1, 0]))
    assert check_kp_args(1.0, 2, **ok) == 1.0
    assert check_kp_args(1.0, 1, **{**ok, "gender_id": None, "betas": torch.zeros(10)}) == 1.0
    for bad in (dict(kp_weight=-1.0, n_models=1), dict(kp_weight=float("nan"), n_models=1), dict(kp_weight=float("nan"), n_models=0),
                dict(kp_weight=float("inf"), n_models=1), dict(kp_weight=0.1, n_models=0), dict(kp_weight=1.0, n_models=4),
                dict(kp_weight=1.0, n_models=1, pose_dim=72), dict(kp_weight=1.0, n_models=1, kp_joint_weight=np.ones(16))):
        with pytest.raises(ValueError):
            check_kp_args(**bad)
    for k, v in (("target_keypoints", None), ("target_keypoints", torch.zeros(4, 1, 17, 3)), ("target_keypoints", torch.zeros(4, 2, 51)),
                 ("betas", torch.zeros(4, 9)), ("betas", torch.zeros(8, 10)), ("gender_id", None), ("gender_id", np.array([0, 1, 2, 0])),
                 ("gender_id", np.array([0, -1, 1, 0])), ("gender_id", np.array([0, 1, 1])), ("gender_id", np.array([0., 1., 1., 0.]))):
        with pytest.raises(ValueError):
            check_kp_args(1.0, 2, **{**ok, k: v})


def test_check_kp_loss_tensors():
    f = K.check_kp_loss_tensors
    P, kp = torch.zeros(3, 66), torch.zeros(3, 17, 3)
    assert f(10, P, kp, None, None, None, None, None, 1.0) == (3, 66, 0, 0)
    wide = torch.zeros(3, 68)
    assert f(10, wide[:, :66], kp, torch.zeros(3, 10), torch.ones(3, 17), torch.zeros(2, dtype=torch.int32), torch.zeros(3),
             wide[:, :66], 0.5) == (3, 68, 10, 17)
    assert f(10, P, kp, torch.zeros(10), torch.ones(17), None, None, None, 1.0) == (3, 66, 0, 0)
    bad = [dict(poses=torch.zeros(3, 65)), dict(poses=torch.zeros(66, 3).t()), dict(poses=P.double()), dict(kps=torch.zeros(3, 51)),
           dict(kps=torch.zeros(2, 17, 3)), dict(betas=torch.zeros(3, 9)), dict(joint_weight=torch.ones(3, 16)),
           dict(rows=torch.zeros(2, dtype=torch.int64)), dict(rows=torch.zeros(4, dtype=torch.int32)), dict(out_loss=torch.zeros(2)),
           dict(out_grad=torch.zeros(3, 65)), dict(out_grad=torch.zeros(3, 132)[:, ::2]), dict(grad_scale=float("nan")),
           dict(grad_scale=float("inf"))]
    for kw in bad:
        a = dict(poses=P, kps=kp, betas=None, joint_weight=None, rows=None, out_loss=None, out_grad=None, grad_scale=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            f(10, **a)
