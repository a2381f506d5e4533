"""refine.refine_poses (tik_fk_joints_jacobian + tik_lm_solve + SMPLX.joints per
iteration) end to end, and the inference interface around it.

The end-to-end case: F = 6 frames on a cut-down synthetic body
(fk_jacobian_ref.small_consts(1, 1): 77 vertices), truth poses with every
body-joint component uniform in +-0.3, keypoints = the oracle's COCO-17 of the
truth, theta0 = truth + N(0, 0.1^2). The GPU's final cost is compared with a
float64 reference LM in this file: the same algorithm on the CPU, residuals
from the numpy oracle, the Jacobian by central differences of it.

Reference on the CPU (seed 3, prior_weight 1e-2, lam0 1e-2, 10 iterations): the
data term 1/2 |r|^2 summed over the frames falls from 1.267 to 7.60e-4, a
factor 1667 (asserted >= 10 before the GPU is touched); its final cost per
frame is 1.1e-3 .. 1.6e-3, mostly the prior term. Measured on the MI355X: the
GPU's final cost per frame agrees with the reference's to all 6 printed digits
(ratio 1.00 against the allowed 1.5); fk_check mean 0.128 -> 0.0034.
"""
import numpy as np
import pytest

import fk_jacobian_ref as R
import memedge as me
from oracle import smplx_lbs as sl

pytestmark = pytest.mark.gpu
F, ITERS, PRIOR, LAM0, SEED = 6, 10, 1e-2, 1e-2, 3
_CASE = {}


def consts():
    return R.small_consts(1, 1)


def rel(x):
    return x - 0.5 * (x[:, 11:12] + x[:, 12:13])


def coco_of(theta):
    full = np.zeros((theta.shape[0], 55, 3))
    full[:, :22] = theta.reshape(-1, 22, 3)
    return sl.smplx_forward(consts(), full, return_verts=False)[:, R.COCO]


def case():
    """truth, theta0 (fp32 values), keypoints (fp32 values), and the float64 reference LM's cost history."""
    if _CASE:
        return _CASE
    rng = np.random.default_rng(SEED)
    truth = rng.uniform(-0.3, 0.3, (F, 66))
    th0 = (truth + rng.normal(0, 0.1, (F, 66))).astype(np.float32).astype(np.float64)
    kps = coco_of(truth).astype(np.float32).astype(np.float64)
    target = rel(kps)

    def resid(th):
        return (rel(coco_of(th)) - target).reshape(-1, 51)

    def cost_of(r, th):
        return 0.5 * (r * r).sum(1) + 0.5 * PRIOR * ((th - th0) ** 2).sum(1)

    def jacobian(th):
        P = np.repeat(th, 2 * 66, axis=0)
        for b in range(F):
            for q in range(66):
                P[(b * 66 + q) * 2, q] += R.STEP
                P[(b * 66 + q) * 2 + 1, q] -= R.STEP
        J = rel(coco_of(P)).reshape(F, 66, 2, 51)
        return ((J[:, :, 0] - J[:, :, 1]) / (2 * R.STEP)).transpose(0, 2, 1)   # (F, 51, 66)

    th, lam = th0.copy(), np.full(F, LAM0)
    r = resid(th)
    cost = cost_of(r, th)
    hist, data0 = [cost.copy()], 0.5 * (r * r).sum()
    for _ in range(ITERS):
        J = jacobian(th)
        r = resid(th)
        cand = th.copy()
        for b in range(F):
            N = J[b].T @ J[b] + (PRIOR + lam[b]) * np.eye(66)
            cand[b] += np.linalg.solve(N, -(J[b].T @ r[b] + PRIOR * (th[b] - th0[b])))
        cc = cost_of(resid(cand), cand)
        ok = cc < cost
        th = np.where(ok[:, None], cand, th)
        cost = np.where(ok, cc, cost)
        lam = np.where(ok, lam / 3.0, lam * 3.0)
        hist.append(cost.copy())
    r = resid(th)
    _CASE.update(th0=th0.astype(np.float32), kps=kps.astype(np.float32).reshape(F, 17, 3), hist=np.stack(hist),
                 data0=data0, data1=0.5 * (r * r).sum())
    return _CASE


@pytest.fixture(scope="module")
def model():
    me.lib()
    return R.SMPLX(consts(), batch_size=9)


def test_refine_against_the_float64_reference(model):
    from temporal_inverse_kinematics_amd.inference import fk_check
    from temporal_inverse_kinematics_amd.refine import refine_poses
    c = case()
    print(f"reference LM: data term {c['data0']:.3e} -> {c['data1']:.3e} (x{c['data0'] / c['data1']:.0f}), "
          f"final cost per frame {c['hist'][-1]}")
    assert c["data1"] * 10 <= c["data0"]                      # on the CPU, before the GPU is touched
    assert (np.diff(c["hist"], axis=0) <= 0).all()
    out = refine_poses(c["th0"], c["kps"], model, iters=ITERS, prior_weight=PRIOR, lam0=LAM0)
    assert out["poses"].shape == (F, 66) and out["poses"].dtype == np.float32
    assert out["cost"].shape == (ITERS + 1, F)
    assert np.isfinite(out["cost"]).all() and np.isfinite(out["poses"]).all()
    assert (np.diff(out["cost"], axis=0) <= 0).all(), out["cost"]
    print(f"GPU final cost per frame {out['cost'][-1]}")
    assert np.abs(out["cost"][0] - c["hist"][0]).max() < 1e-4   # the same starting cost (fp32 FK vs float64)
    assert (out["cost"][-1] <= 1.5 * c["hist"][-1] + 1e-8).all(), (out["cost"][-1], c["hist"][-1])
    before = fk_check(c["th0"], c["kps"], model)["mean"]
    after = fk_check(out["poses"], c["kps"], model)["mean"]
    print(f"fk_check mean: {before:.5f} -> {after:.5f}")
    assert after < before
    same = refine_poses(c["th0"], c["kps"], model, iters=0, prior_weight=PRIOR)
    assert np.array_equal(same["poses"], c["th0"]) and same["cost"].shape == (1, F)
    w = np.ones(17, np.float32)
    weighted = refine_poses(c["th0"], c["kps"], model, iters=2, prior_weight=PRIOR, lam0=LAM0, joint_weight=w)
    assert np.array_equal(weighted["cost"], out["cost"][:3])   # unit weights: the same arithmetic (x * 1)


def test_prior_weight_is_required(model):
    from temporal_inverse_kinematics_amd.refine import refine_poses
    c = case()
    for pw in (0, 0.0, -1.0):
        with pytest.raises(ValueError, match="prior_weight"):
            refine_poses(c["th0"], c["kps"], model, prior_weight=pw)


def test_run_test_refine(tmp_path):
    from conftest import golden
    from temporal_inverse_kinematics_amd.inference import run_test
    me.lib()
    k = golden("keypoints.npz")
    src = tmp_path / "cam01_track00.npz"
    np.savez(src, joints_3d=k["moveai_joints"].astype(np.float32), joint_3d_names=k["moveai_names"])
    plain = run_test(str(src), "synthetic", win_size=64, check=True)
    zero = run_test(str(src), "synthetic", win_size=64, check=True, refine=0)
    assert sorted(zero) == sorted(plain) == ["coco", "fk_check", "joints", "poses", "vertices"]
    for key in ("coco", "joints", "poses", "vertices"):
        assert np.array_equal(zero[key], plain[key]), key
    got = run_test(str(src), "synthetic", win_size=64, check=True, refine=3)
    assert sorted(got) == ["coco", "fk_check", "fk_check_refined", "joints", "poses", "poses_refined", "vertices"]
    assert np.array_equal(got["poses"], plain["poses"]) and np.array_equal(got["joints"], plain["joints"])
    assert got["poses_refined"].shape == plain["poses"].shape and got["poses_refined"].dtype == np.float32
    print(f"run_test fk_check mean: {got['fk_check']['mean']:.5f} -> {got['fk_check_refined']['mean']:.5f}")
    assert np.array_equal(got["fk_check"]["per_joint"], plain["fk_check"]["per_joint"])
    assert np.isfinite(got["fk_check_refined"]["per_joint"]).all()
    with pytest.raises(ValueError):
        run_test(str(src), None, win_size=64, refine=2)
