"""refine.refine_smooth (tik_fk_joints_jacobian + tik_lm_solve_chain + SMPLX.joints
per iteration) end to end, refine_sequence(smooth_weight=...) and the inference
interface around them.

The scenario: F = 8 frames on the cut-down synthetic body
(fk_jacobian_ref.small_consts(1, 1)), truth a + b sin(phi + 0.25 f) per pose
component with a, b uniform in +-0.3 and phi in (0, 2 pi), default_rng(3);
theta0 = truth + N(0, 0.1^2); the keypoints are the oracle's COCO-17 of the
truth. Weights (F,17): frame 3 all zero and its keypoints NaN (a frame nobody
detected), frame 5 without its wrists (COCO 9, 10). 8 iterations,
smooth_weight 0.1, prior_weight 1e-2, lam0 1e-2.

The float64 reference is in this file: the same algorithm on the CPU, residuals
from the numpy oracle, Jacobians by central differences, the coupled system
solved densely, acceptance per sequence. Asserted on it before the GPU is
touched: a monotone history; the mean |theta_{f+1} - 2 theta_f + theta_{f-1}|
of its result at most 1/5 of theta0's (reference 0.0074 against 0.187); frame
3's mean keypoint error against the true keypoints at most 1/3 of what a
float64 per-frame LM with the same weights leaves (reference 0.0087 against
0.103: per frame, an unobserved frame stays at theta0).

The GPU run must start from the same cost (1e-4), end at most at 1.5 x the
reference's final cost (both margins are test_gpu_refine.py's) and pass the same
two ratios. Measured on the MI355X: cost 1.452795 -> 0.033921 on the GPU and in
the reference (GPU / reference = 1.0000 against the allowed 1.5), second
difference 0.0074, frame 3's keypoint error 0.0087. run_test on the shipped
sample, 3 iterations, synthetic weights: the mean second difference of the
network's poses is 0.0040, of the per-frame refinement 0.187, with smooth=0.1
0.022 (fk_check mean 0.544 -> 0.327 / 0.312). DESIGN.md "LM chain solve".
"""
import numpy as np
import pytest

import fk_jacobian_ref as R
import memedge as me
from oracle import smplx_lbs as sl

pytestmark = pytest.mark.gpu
F, ITERS, PRIOR, LAM0, SEED, SMOOTH = 8, 8, 1e-2, 1e-2, 3, 0.1
_CASE = {}


def consts():
    return R.small_consts(1, 1)


def rel(x):
    return x - 0.5 * (x[:, 11:12] + x[:, 12:13])


def coco_of(theta):
    full = np.zeros((theta.shape[0], 55, 3))
    full[:, :22] = np.asarray(theta, np.float64).reshape(-1, 22, 3)
    return sl.smplx_forward(consts(), full, return_verts=False)[:, R.COCO]


def second_difference(th):
    th = np.asarray(th, np.float64)
    return float(np.abs(th[2:] - 2 * th[1:-1] + th[:-2]).mean())


def jacobian(th):
    n = th.shape[0]
    P = np.repeat(th, 2 * 66, axis=0)
    for b in range(n):
        for q in range(66):
            P[(b * 66 + q) * 2, q] += R.STEP
            P[(b * 66 + q) * 2 + 1, q] -= R.STEP
    J = rel(coco_of(P)).reshape(n, 66, 2, 51)
    return ((J[:, :, 0] - J[:, :, 1]) / (2 * R.STEP)).transpose(0, 2, 1)   # (n, 51, 66)


def reference_lm(th0, target, w, smooth, starts):
    """Float64 LM with the smoothness term (smooth = 0: every frame a sequence of its own is the
    per-frame LM) -> (poses, cost history (ITERS+1, S))."""
    n = th0.shape[0]
    W = np.repeat(w, 3, axis=1)
    seqs = list(zip(starts[:-1], starts[1:]))

    def resid(th):
        return (rel(coco_of(th)) - target).reshape(n, 51)

    def cost_of(r, th):
        per = 0.5 * (W * r * r).sum(1) + 0.5 * PRIOR * ((th - th0) ** 2).sum(1)
        return np.array([per[a:b].sum() + 0.5 * smooth * ((th[a + 1:b] - th[a:b - 1]) ** 2).sum() for a, b in seqs])

    th, lam = th0.copy(), np.full(len(seqs), LAM0)
    cost = cost_of(resid(th), th)
    hist = [cost.copy()]
    for _ in range(ITERS):
        J, r = jacobian(th), resid(th)
        cand = th.copy()
        for q, (a, b) in enumerate(seqs):
            L = b - a
            A, g = np.zeros((L * 66, L * 66)), np.zeros(L * 66)
            for k in range(L):
                f = a + k
                c = int(k > 0) + int(k < L - 1)
                blk = slice(k * 66, (k + 1) * 66)
                A[blk, blk] = (J[f].T * W[f]) @ J[f] + (PRIOR + lam[q] + smooth * c) * np.eye(66)
                t = c * th[f] - (th[f - 1] if k > 0 else 0) - (th[f + 1] if k < L - 1 else 0)
                g[blk] = (J[f].T * W[f]) @ r[f] + PRIOR * (th[f] - th0[f]) + smooth * t
                if k:
                    A[blk, (k - 1) * 66:k * 66] = A[(k - 1) * 66:k * 66, blk] = -smooth * np.eye(66)
            cand[a:b] += np.linalg.solve(A, -g).reshape(L, 66)
        cc = cost_of(resid(cand), cand)
        ok = cc < cost
        for q, (a, b) in enumerate(seqs):
            if ok[q]:
                th[a:b] = cand[a:b]
        cost = np.where(ok, cc, cost)
        lam = np.where(ok, lam / 3.0, lam * 3.0)
        hist.append(cost.copy())
    return th, np.stack(hist)


def case():
    """The scenario and its float64 references (computed once, read only)."""
    if _CASE:
        return _CASE
    rng = np.random.default_rng(SEED)
    a, b = rng.uniform(-0.3, 0.3, 66), rng.uniform(-0.3, 0.3, 66)
    phi = rng.uniform(0, 2 * np.pi, 66)
    truth = a + b * np.sin(phi + 0.25 * np.arange(F)[:, None])
    th0 = (truth + rng.normal(0, 0.1, (F, 66))).astype(np.float32).astype(np.float64)
    kps = coco_of(truth).astype(np.float32).astype(np.float64)
    w = np.ones((F, 17))
    w[3] = 0.0
    w[5, [9, 10]] = 0.0
    target = rel(kps)
    smooth_th, smooth_hist = reference_lm(th0, target, w, SMOOTH, np.array([0, F]))
    frame_th, _ = reference_lm(th0, target, w, 0.0, np.arange(F + 1))
    holes = kps.astype(np.float32).reshape(F, 17, 3).copy()
    holes[3] = np.nan

    def frame3_error(th):
        return float(np.linalg.norm(rel(coco_of(th[3:4])) - target[3:4], axis=2).mean())

    _CASE.update(truth=truth, th0=th0.astype(np.float32), kps=kps.astype(np.float32).reshape(F, 17, 3), holes=holes,
                 w=w.astype(np.float32), smooth_th=smooth_th, hist=smooth_hist, frame3=frame3_error,
                 frame3_smooth=frame3_error(smooth_th), frame3_per_frame=frame3_error(frame_th),
                 d2_th0=second_difference(th0), d2_smooth=second_difference(smooth_th), d2_truth=second_difference(truth))
    return _CASE


@pytest.fixture(scope="module")
def model():
    me.lib()
    return R.SMPLX(consts(), batch_size=9)


def test_refine_smooth_against_the_float64_reference(model):
    from temporal_inverse_kinematics_amd.refine import refine_smooth
    c = case()
    print(f"reference: cost {c['hist'][0, 0]:.6f} -> {c['hist'][-1, 0]:.6f}; second difference theta0 {c['d2_th0']:.4f}, "
          f"result {c['d2_smooth']:.4f}, truth {c['d2_truth']:.4f}; frame 3 keypoint error smooth {c['frame3_smooth']:.4f}, "
          f"per-frame LM {c['frame3_per_frame']:.4f}")
    assert (np.diff(c["hist"], axis=0) <= 0).all()                       # on the CPU, before the GPU is touched
    assert c["d2_smooth"] <= c["d2_th0"] / 5
    assert c["frame3_smooth"] <= c["frame3_per_frame"] / 3
    out = refine_smooth(c["th0"], c["holes"], model, SMOOTH, iters=ITERS, prior_weight=PRIOR, joint_weight=c["w"], lam0=LAM0)
    assert out["poses"].shape == (F, 66) and out["poses"].dtype == np.float32
    assert out["cost"].shape == (ITERS + 1, 1)
    assert np.isfinite(out["cost"]).all() and np.isfinite(out["poses"]).all()
    assert (np.diff(out["cost"], axis=0) <= 0).all(), out["cost"]
    d2, f3 = second_difference(out["poses"]), c["frame3"](out["poses"])
    print(f"GPU: cost {out['cost'][0, 0]:.6f} -> {out['cost'][-1, 0]:.6f} (ratio to the reference "
          f"{out['cost'][-1, 0] / c['hist'][-1, 0]:.4f}); second difference {d2:.4f}; frame 3 keypoint error {f3:.4f}")
    assert abs(out["cost"][0, 0] - c["hist"][0, 0]) < 1e-4               # the same starting cost (fp32 FK vs float64)
    assert out["cost"][-1, 0] <= 1.5 * c["hist"][-1, 0] + 1e-8, (out["cost"][-1], c["hist"][-1])
    assert d2 <= c["d2_th0"] / 5
    assert f3 <= c["frame3_per_frame"] / 3
    # weights that say the same without NaN keypoints: the same arithmetic
    same = refine_smooth(c["th0"], c["kps"], model, SMOOTH, iters=2, prior_weight=PRIOR, joint_weight=c["w"], lam0=LAM0)
    assert np.array_equal(same["cost"], out["cost"][:3])
    zero = refine_smooth(c["th0"], c["holes"], model, SMOOTH, iters=0, prior_weight=PRIOR, joint_weight=c["w"])
    assert np.array_equal(zero["poses"], c["th0"]) and zero["cost"].shape == (1, 1)


def test_sequences_do_not_see_each_other(model):
    from temporal_inverse_kinematics_amd.refine import refine_smooth
    c = case()
    kw = dict(iters=4, prior_weight=PRIOR, joint_weight=c["w"], lam0=LAM0, seq_starts=[0, 3, F])
    out = refine_smooth(c["th0"], c["holes"], model, SMOOTH, **kw)
    assert out["cost"].shape == (5, 2) and np.isfinite(out["cost"]).all()
    assert (np.diff(out["cost"], axis=0) <= 0).all()
    moved = c["holes"].copy()
    moved[:3] += np.random.default_rng(1).normal(0, 0.05, (3, 17, 3)).astype(np.float32)
    other = refine_smooth(c["th0"], moved, model, SMOOTH, **kw)
    assert np.array_equal(other["poses"][3:], out["poses"][3:])
    assert np.array_equal(other["cost"][:, 1], out["cost"][:, 1])
    assert not np.array_equal(other["poses"][:3], out["poses"][:3])


def test_refine_sequence_with_smoothness(model):
    from temporal_inverse_kinematics_amd.refine import refine_sequence
    c = case()
    kw = dict(rounds=2, iters=3, prior_weight=PRIOR, lam0=LAM0)
    plain = refine_sequence(c["th0"], c["kps"], model, **kw)
    zero = refine_sequence(c["th0"], c["kps"], model, smooth_weight=0.0, **kw)
    for key in ("poses", "betas", "cost"):
        assert np.array_equal(zero[key], plain[key]), key
    out = refine_sequence(c["th0"], c["kps"], model, smooth_weight=SMOOTH, **kw)
    print(f"refine_sequence total cost: plain {plain['cost']}, smooth {out['cost']}; second difference "
          f"{second_difference(plain['poses']):.4f} -> {second_difference(out['poses']):.4f}")
    assert out["cost"].shape == (3,) and np.isfinite(out["cost"]).all() and np.isfinite(out["poses"]).all()
    assert (np.diff(out["cost"]) <= 0).all(), out["cost"]
    assert out["poses"].shape == (F, 66) and out["poses"].dtype == np.float32


def test_run_test_smooth(tmp_path):
    from conftest import golden
    from temporal_inverse_kinematics_amd.inference import run_test
    me.lib()
    k = golden("keypoints.npz")
    src = tmp_path / "cam01_track00.npz"
    np.savez(src, joints_3d=k["moveai_joints"].astype(np.float32), joint_3d_names=k["moveai_names"])
    plain = run_test(str(src), "synthetic", win_size=64, check=True, refine=3)
    got = run_test(str(src), "synthetic", win_size=64, check=True, refine=3, smooth=0.1)
    assert sorted(got) == sorted(plain) == ["coco", "fk_check", "fk_check_refined", "joints", "poses", "poses_refined", "vertices"]
    assert np.array_equal(got["poses"], plain["poses"])
    assert got["poses_refined"].shape == plain["poses"].shape and got["poses_refined"].dtype == np.float32
    assert np.isfinite(got["poses_refined"]).all()
    d_in, d_plain, d_smooth = (second_difference(x) for x in (got["poses"], plain["poses_refined"], got["poses_refined"]))
    print(f"run_test second difference: poses {d_in:.5f}, refined {d_plain:.5f}, refined with smooth=0.1 {d_smooth:.5f}; "
          f"fk_check mean {got['fk_check']['mean']:.5f} -> {plain['fk_check_refined']['mean']:.5f} (refine) / "
          f"{got['fk_check_refined']['mean']:.5f} (smooth)")
    assert d_smooth < d_plain
    both = run_test(str(src), "synthetic", win_size=64, check=True, refine=2, fit_shape=1, smooth=0.1)
    assert sorted(both) == sorted(list(plain) + ["betas"]) and np.isfinite(both["poses_refined"]).all()
    with pytest.raises(ValueError):
        run_test(str(src), "synthetic", win_size=64, smooth=0.1)
