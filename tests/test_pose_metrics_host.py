"""The pose metrics on the CPU: the float64 reference of tests/pose_metrics_ref.py is pinned before anything trusts it
(its SVD form against an independent Horn-quaternion form, its invariances, its edge cases, its angles), the factor
the GPU test's bounds rest on is checked on the test's own frames, and the pure argument checks
(smplx_fk.check_pose_metrics_tensors) raise without the library."""
import numpy as np
import pytest
import torch

import pose_metrics_ref as P

K, R = P.K, P.R


def frames(weighted="frame"):
    w, ref = P.case65("frame", weighted)
    return ref["x"], ref["y"], P.weights_of(w, 65)


def similarity0():
    """A fixed similarity transform: s0, a proper R0 (rotation vector (0.4, -1.1, 0.7)), t0."""
    R0 = P.sl.batch_rodrigues(np.array([[0.4, -1.1, 0.7]]))[0]
    return 1.7, R0, np.array([0.3, -0.2, 0.5])


def test_svd_form_against_horn_form():
    worst = 0.0
    for weighted in (None, "shared", "frame"):
        x, y, w = frames(weighted)
        for xx in (x, P.mirrored(x)):
            a = P.point_metrics(xx, y, w)["pa_mpjpe"]
            b = P.point_metrics(xx, y, w, P.similarity_horn)["pa_mpjpe"]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            ok = ~np.isnan(a)
            assert ok.sum() >= 63
            worst = max(worst, float(np.abs(a[ok] - b[ok]).max()))
    print(f"worst |pa_mpjpe(svd) - pa_mpjpe(horn)| = {worst:.2e}")
    assert worst <= 1e-10


def test_similarity_invariance():
    x, y, w = frames()
    s0, R0, t0 = similarity0()
    ok = (w > 0).sum(1) >= 3
    moved = s0 * y @ R0.T + t0
    exact = P.point_metrics(y, moved, w)["pa_mpjpe"][ok]
    print(f"pa_mpjpe(y, s0 R0 y + t0): worst {exact.max():.2e}")
    assert (exact <= 1e-12).all()
    a = P.point_metrics(x, y, w)["pa_mpjpe"][ok]
    b = P.point_metrics(s0 * x @ R0.T + t0, y, w)["pa_mpjpe"][ok]
    print(f"pa_mpjpe(x, y) against pa_mpjpe(s0 R0 x + t0, y): worst {np.abs(a - b).max():.2e}")
    assert np.abs(a - b).max() <= 1e-10
    assert (a > 1e-3).all()                                     # the frames are not aligned to begin with


def test_mirrored_body_is_not_aligned_by_a_reflection():
    x, y, w = frames(None)
    for f in range(0, 65, 8):
        xm = P.mirrored(y[f])                                   # y's own mirror image: a reflection would align it exactly
        got = P.point_metrics(xm[None], y[f][None], w[f][None])["pa_mpjpe"][0]
        horn = P.point_metrics(xm[None], y[f][None], w[f][None], P.similarity_horn)["pa_mpjpe"][0]
        assert got > 1e-3 and abs(got - horn) <= 1e-10
        # the reference's rotation is proper and no proper rotation nearby does better on the squared objective
        s, Rm, mx, my = P.similarity_svd(xm, y[f], w[f])
        assert abs(np.linalg.det(Rm) - 1.0) <= 1e-12
        cost = lambda Rq: (w[f] * ((s * (xm - mx) @ Rq.T - (y[f] - my)) ** 2).sum(1)).sum()
        rng = np.random.default_rng(f)
        for _ in range(8):
            dR = P.sl.batch_rodrigues(rng.normal(0, 0.05, (1, 3)))[0]
            assert cost(Rm) <= cost(dR @ Rm) + 1e-15
        # the reflection's value, for contrast: zero
        s2, R2, _, _ = P.similarity_svd(y[f], y[f], w[f])
        assert abs(s2 - 1.0) <= 1e-12 and np.abs(R2 - np.eye(3)).max() <= 1e-12


def test_missing_weights():
    x, y, _ = frames()
    w = np.ones((4, 17))
    w[0] = 0.0                                                  # W = 0
    w[1] = 0.0
    w[1, [5, 12]] = (0.7, 1.3)                                  # n = 2
    w[2] = 0.0
    w[2, [0, 5, 12]] = 1.0                                      # n = 3
    m = P.point_metrics(x[:4], y[:4], w)
    assert np.isnan(m["mpjpe"][0]) and np.isnan(m["pa_mpjpe"][0]) and m["weight"][0] == 0.0
    assert np.isfinite(m["mpjpe"][1]) and np.isnan(m["pa_mpjpe"][1]) and m["weight"][1] == 2.0
    assert np.isfinite(m["mpjpe"][2:]).all() and np.isfinite(m["pa_mpjpe"][2:]).all()
    w65 = P.weights65("frame")
    assert (w65[0] == 0).all() and (w65[1] > 0).sum() == 2


def test_mpjae():
    """A pose against itself: exactly 0. One joint turned by a about its own axis: a / 22, up to the oracle's own
    Rodrigues, which takes the angle of v + 1e-8 but the axis of v: the matrix is off the rotation by a about v / |v|
    by about 1e-8 (1 + a) / |v| per entry, 2e-7 on the angle at the |v| of these frames and 1e-8 after the division
    by 22; float64 rounding is far below."""
    th = K.inputs65()[0].astype(np.float64)
    assert (P.mpjae(th, th) == 0.0).all()                       # exact: D is symmetric to the bit
    for a in P.CONSTRUCTED + (1e-6, 3.0):
        for j in (0, 5, 21):
            t = np.stack([P.turned(th[f], j, a) for f in range(8)])
            got = P.mpjae(th[:8], t)
            assert np.abs(got - a / 22.0).max() <= 1e-8, (a, j, np.abs(got - a / 22.0).max())
    t65 = P.targets65().astype(np.float64)
    got = P.mpjae(K.inputs65()[0], t65)[:4]
    assert np.abs(got - np.array(P.CONSTRUCTED) / 22.0).max() <= 1e-7      # the float32 rounding of the targets


def test_tolerance_factor():
    """What the GPU bounds rest on: an error of at most R.TOL in every entry of x moves mpjpe by at most sqrt(3) TOL
    (exact: each |x_k - y_k| moves by at most |dx_k| <= sqrt(3) TOL, and the weights sum to W) and, measured here on
    the test's frames and their mirror images with 16 random sign patterns each, pa_mpjpe by no more."""
    T = R.TOL
    rng = np.random.default_rng(29)
    worst = [0.0, 0.0]
    for weighted in (None, "frame"):
        x, y, w = frames(weighted)
        for xx in (x, P.mirrored(x)):
            base = P.point_metrics(xx, y, w)
            for _ in range(16):
                got = P.point_metrics(xx + T * rng.choice([-1.0, 1.0], xx.shape), y, w)
                for i, k in enumerate(("mpjpe", "pa_mpjpe")):
                    ok = ~np.isnan(base[k])
                    assert np.array_equal(~np.isnan(got[k]), ok)
                    worst[i] = max(worst[i], float(np.abs(got[k][ok] - base[k][ok]).max()))
    print(f"x +- TOL per entry: mpjpe moves by {worst[0] / (P.SQ3 * T):.3f} sqrt(3) TOL, "
          f"pa_mpjpe by {worst[1] / (P.SQ3 * T):.3f} sqrt(3) TOL")
    assert worst[0] <= P.SQ3 * T * (1 + 1e-9) and worst[1] <= P.SQ3 * T


def test_accel_reference():
    rng = np.random.default_rng(3)
    x, y = rng.normal(0, 1, (12, 17, 3)), rng.normal(0, 1, (12, 17, 3))
    a = P.accel(x, y, [0, 7, 12])
    assert np.isnan(a[[0, 6, 7, 11]]).all() and np.isfinite(a[[1, 2, 3, 4, 5, 8, 9, 10]]).all()
    f = 9
    want = np.linalg.norm((x[f + 1] - 2 * x[f] + x[f - 1]) - (y[f + 1] - 2 * y[f] + y[f - 1]), axis=1).mean()
    assert abs(a[f] - want) <= 1e-14
    t = np.arange(12.0)[:, None, None]
    assert np.nanmax(P.accel(y + 3.0 * t + 1.0, y)) <= 1e-12    # a constant velocity has no acceleration error


def test_check_pose_metrics_tensors():
    from temporal_inverse_kinematics_amd import _lib
    loaded = _lib._lib
    f = P.check_pose_metrics_tensors
    Pz, kp = torch.zeros(3, 66), torch.zeros(3, 17, 3)
    none = dict(betas=None, joint_weight=None, target_poses=None, rows=None, out=None, out_joints=None)
    assert f(10, Pz, kp, **none) == (3, 66, 0, 0, 0)
    wide = torch.zeros(3, 68)
    assert f(10, wide[:, :66], kp, torch.zeros(3, 10), torch.ones(3, 17), torch.zeros(3, 70)[:, :66],
             torch.zeros(2, dtype=torch.int32), torch.zeros(3, 4), torch.zeros(3, 17, 3)) == (3, 68, 10, 17, 70)
    assert f(10, Pz, kp, torch.zeros(10), torch.ones(17), Pz, None, None, None) == (3, 66, 0, 0, 66)
    assert f(10, Pz[:1], kp[:1], **none) == (1, 66, 0, 0, 0)
    bad = [dict(poses=torch.zeros(3, 65)), dict(poses=torch.zeros(66, 3).t()), dict(poses=Pz.double()), dict(poses=torch.zeros(0, 66)),
           dict(kps=torch.zeros(3, 51)), dict(kps=torch.zeros(2, 17, 3)), dict(kps=kp.double()), dict(betas=torch.zeros(3, 9)),
           dict(joint_weight=torch.ones(3, 16)), dict(target_poses=torch.zeros(2, 66)), dict(target_poses=torch.zeros(3, 65)),
           dict(target_poses=Pz.double()), dict(target_poses=torch.zeros(3, 132)[:, ::2]),
           dict(rows=torch.zeros(2, dtype=torch.int64)), dict(rows=torch.zeros(4, dtype=torch.int32)), dict(out=torch.zeros(3, 3)),
           dict(out=torch.zeros(3, 8)[:, ::2]), dict(out=torch.zeros(3, 4, dtype=torch.float64)), dict(out_joints=torch.zeros(3, 51)),
           dict(out_joints=torch.zeros(2, 17, 3))]
    for kw in bad:
        a = dict(poses=Pz, kps=kp, **none)
        a.update(kw)
        with pytest.raises(ValueError):
            f(10, **a)
    for kw in (dict(poses=np.zeros((3, 66), np.float32)), dict(kps=None), dict(betas=np.zeros(10, np.float32)),
               dict(joint_weight=[1.0] * 17), dict(target_poses=np.zeros((3, 66), np.float32)), dict(rows=[0, 1]),
               dict(out=np.zeros((3, 4), np.float32)), dict(out_joints=0)):
        a = dict(poses=Pz, kps=kp, **none)
        a.update(kw)
        with pytest.raises(TypeError):
            f(10, **a)
    assert _lib._lib is loaded                                   # the library was not asked
