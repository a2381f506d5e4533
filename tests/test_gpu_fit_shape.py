"""refine.fit_shape / refine.refine_sequence (tik_fk_joints_shape_jacobian +
tik_lm_accumulate + tik_lm_solve_sum, alternated with refine_poses) end to end,
and the inference interface around them.

The case follows tests/test_gpu_refine.py: F = 6 frames on the 77-vertex body
fk_jacobian_ref.small_consts(1, 1), seed 3, truth poses uniform in +-0.3,
theta0 = truth + N(0, 0.1^2), and here truth betas N(0, 1) rounded to fp32;
the keypoints are the oracle's COCO-17 of the truth, rounded to fp32. The
float64 reference is tests/fk_shape_ref.py: the same algorithm on the CPU.

Reference on the CPU (shape_weight 1e-3, prior_weight 1e-2, lam0 1e-2):
fit_shape at the truth poses from zero betas takes the data + shape cost from
0.282 to 4.29e-3 and a second step moves the betas by 2e-15; the prior biases
the solution by up to 0.038 against the truth betas, so the GPU is compared
with the reference solution of the same regularised system. 3 rounds of one
shape step + 5 pose iterations leave a data term of 3.39e-3, 15 pose-only
iterations 3.82e-2.

The bound on |betas(GPU) - betas(reference)| is BETAS_BOUND = 10 x the
difference measured on the MI355X (MEASURED_BETAS = 1.254e-6; a second GPU
step from the result moved the betas by 1.07e-6), never above 1e-2, which is
what the FK tolerance allows: a residual error of 1e-4 sqrt(306) over the
smallest singular value of the stacked shape Jacobian, 0.136. Measured there too: refine_sequence's total cost 1.45300709, 0.02733767,
0.01897694, 0.01605493 against the reference's 1.45300703, 0.02733765,
0.01897693, 0.01605491; fk_check mean 0.02470 (15 pose iterations, mean shape)
-> 0.00726 (3 rounds of shape + 5 pose iterations).
"""
import numpy as np
import pytest

import fk_jacobian_ref as R
import fk_shape_ref as S
import memedge as me

pytestmark = pytest.mark.gpu
F, SEED, PRIOR, SHAPE_W, LAM0 = 6, 3, 1e-2, 1e-3, 1e-2
MEASURED_BETAS = 1.254e-6                   # max |betas(GPU) - betas(float64)| on the MI355X
BETAS_BOUND = min(1e-2, 10 * MEASURED_BETAS)
_CASE = {}


def consts():
    return R.small_consts(1, 1)


def case():
    if _CASE:
        return _CASE
    rng = np.random.default_rng(SEED)
    truth = rng.uniform(-0.3, 0.3, (F, 66))
    th0 = (truth + rng.normal(0, 0.1, (F, 66))).astype(np.float32).astype(np.float64)
    betas = rng.normal(0, 1, 10).astype(np.float32).astype(np.float64)
    kps = S.coco_of(consts(), truth, betas).astype(np.float32).astype(np.float64)
    _CASE.update(truth=truth, th0=th0, betas=betas, kps=kps, kps32=kps.astype(np.float32).reshape(F, 17, 3))
    return _CASE


def sequence_reference():
    c = case()
    if "seq" not in c:
        c["seq"] = S.refine_sequence(consts(), c["th0"], c["kps"], rounds=3, iters=5, prior_weight=PRIOR, shape_weight=SHAPE_W,
                                     lam0=LAM0)
        th, _ = S.refine_poses(consts(), c["th0"], c["kps"], None, c["th0"], 15, PRIOR, LAM0)
        c["pose_only_data"] = S.data_term(consts(), th, c["kps"], None)
    return c["seq"], c["pose_only_data"]


@pytest.fixture(scope="module")
def model():
    me.lib()
    return S.SMPLX(consts(), batch_size=9)


# ---------------------------------------------------------------- 1. the shape step
def test_fit_shape_against_the_float64_reference(model):
    from temporal_inverse_kinematics_amd.refine import fit_shape
    c = case()
    ref = S.fit_shape(consts(), c["truth"], c["kps"], None, SHAPE_W)
    again = S.fit_shape(consts(), c["truth"], c["kps"], ref["betas"], SHAPE_W)
    print(f"reference fit_shape: cost {ref['cost'][0]:.4e} -> {ref['cost'][1]:.4e}, a second step moves the betas by "
          f"{np.abs(again['betas'] - ref['betas']).max():.1e}, bias against the truth {np.abs(ref['betas'] - c['betas']).max():.3f}")
    assert ref["cost"][1] * 10 <= ref["cost"][0]              # on the CPU, before the GPU is touched
    assert np.abs(again["betas"] - ref["betas"]).max() < 1e-12
    N, _ = S.shape_system(consts(), c["truth"], c["kps"], np.zeros(10), 0.0)
    smin = np.sqrt(np.linalg.eigvalsh(N)[0])
    assert 1e-4 * np.sqrt(306) / smin >= BETAS_BOUND, smin     # the bound is not above what the FK tolerance allows
    th = c["truth"].astype(np.float32)
    out = fit_shape(th, c["kps32"], model, shape_weight=SHAPE_W)
    assert out["betas"].shape == (10,) and out["betas"].dtype == np.float32 and out["cost"].shape == (2,)
    assert np.isfinite(out["betas"]).all() and np.isfinite(out["cost"]).all()
    diff = np.abs(out["betas"].astype(np.float64) - ref["betas"]).max()
    print(f"max |betas(GPU) - betas(float64)| = {diff:.3e} (bound {BETAS_BOUND:.1e}); GPU cost {out['cost']}")
    assert diff < BETAS_BOUND
    assert abs(out["cost"][0] - ref["cost"][0]) < 1e-4 * F and out["cost"][1] < out["cost"][0]
    two = fit_shape(th, c["kps32"], model, betas=out["betas"], shape_weight=SHAPE_W)
    step = np.abs(two["betas"] - out["betas"]).max()
    print(f"a second GPU step moves the betas by {step:.3e}")
    assert step < BETAS_BOUND
    w = np.ones(17, np.float32)
    weighted = fit_shape(th, c["kps32"], model, shape_weight=SHAPE_W, joint_weight=w)
    assert np.array_equal(weighted["betas"], out["betas"])     # unit weights: the same arithmetic (x * 1)


def test_shape_weight_is_required(model):
    from temporal_inverse_kinematics_amd.refine import fit_shape, refine_sequence
    c = case()
    th = c["th0"].astype(np.float32)
    for sw in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="shape_weight"):
            fit_shape(th, c["kps32"], model, shape_weight=sw)
        with pytest.raises(ValueError, match="shape_weight"):
            refine_sequence(th, c["kps32"], model, shape_weight=sw)


# ---------------------------------------------------------------- 2. the sequence
def test_refine_sequence_against_the_float64_reference(model):
    from temporal_inverse_kinematics_amd.inference import fk_check
    from temporal_inverse_kinematics_amd.refine import refine_poses, refine_sequence
    c = case()
    ref, pose_only = sequence_reference()
    print(f"reference: total cost {ref['cost']}, data term {ref['data']:.3e} against {pose_only:.3e} of 15 pose-only iterations")
    assert ref["data"] * 5 <= pose_only                        # on the CPU, before the GPU is touched
    assert (np.diff(ref["cost"]) <= 0).all()
    th0 = c["th0"].astype(np.float32)
    out = refine_sequence(th0, c["kps32"], model, rounds=3, iters=5, prior_weight=PRIOR, shape_weight=SHAPE_W, lam0=LAM0)
    assert out["poses"].shape == (F, 66) and out["poses"].dtype == np.float32
    assert out["betas"].shape == (10,) and out["betas"].dtype == np.float32
    assert out["cost"].shape == (4,) and np.isfinite(out["cost"]).all()
    assert np.isfinite(out["poses"]).all() and np.isfinite(out["betas"]).all()
    print(f"GPU total cost {out['cost']}, betas {out['betas']}")
    assert (np.diff(out["cost"]) <= 0).all(), out["cost"]
    assert abs(out["cost"][0] - ref["cost"][0]) < 1e-4 * F     # the same starting cost (fp32 FK vs float64)
    assert out["cost"][-1] <= 1.5 * ref["cost"][-1] + 1e-8, (out["cost"][-1], ref["cost"][-1])
    pose_only_gpu = refine_poses(th0, c["kps32"], model, iters=15, prior_weight=PRIOR, lam0=LAM0)["poses"]
    mean_shape = fk_check(pose_only_gpu, c["kps32"], model)["mean"]
    fitted = fk_check(out["poses"], c["kps32"], model, betas=out["betas"])["mean"]
    print(f"fk_check mean: {mean_shape:.5f} (15 pose iterations, mean shape) -> {fitted:.5f} (3 rounds of shape + 5)")
    assert fitted < mean_shape
    same = refine_sequence(th0, c["kps32"], model, rounds=0, prior_weight=PRIOR, shape_weight=SHAPE_W)
    assert np.array_equal(same["poses"], th0) and np.array_equal(same["betas"], np.zeros(10, np.float32))
    assert same["cost"].shape == (1,) and same["cost"][0] == out["cost"][0]
    b0 = np.linspace(-1, 1, 10).astype(np.float32)
    kept = refine_sequence(th0, c["kps32"], model, rounds=0, betas=b0)
    assert np.array_equal(kept["poses"], th0) and np.array_equal(kept["betas"], b0)


# ---------------------------------------------------------------- 3. refine_poses is unchanged
def test_refine_poses_prior_default_is_unchanged(model):
    from temporal_inverse_kinematics_amd.refine import refine_poses
    c = case()
    th0 = c["th0"].astype(np.float32)
    base = refine_poses(th0, c["kps32"], model, iters=4, prior_weight=PRIOR, lam0=LAM0)
    for kw in ({"prior_poses": None}, {"prior_poses": th0}):
        got = refine_poses(th0, c["kps32"], model, iters=4, prior_weight=PRIOR, lam0=LAM0, **kw)
        assert np.array_equal(got["poses"], base["poses"]) and np.array_equal(got["cost"], base["cost"]), kw
    # another anchor is another cost: the starting cost gains the prior term
    moved = refine_poses(th0, c["kps32"], model, iters=0, prior_weight=PRIOR, prior_poses=th0 + np.float32(0.1))
    assert (moved["cost"][0] > base["cost"][0]).all()
    with pytest.raises(ValueError, match="prior_poses"):
        refine_poses(th0, c["kps32"], model, prior_poses=th0[:3])


# ---------------------------------------------------------------- 4. run_test
def test_run_test_fit_shape(tmp_path):
    from conftest import golden
    from temporal_inverse_kinematics_amd.inference import run_test
    me.lib()
    k = golden("keypoints.npz")
    src = tmp_path / "cam01_track00.npz"
    np.savez(src, joints_3d=k["moveai_joints"].astype(np.float32), joint_3d_names=k["moveai_names"])
    plain = run_test(str(src), "synthetic", win_size=64, check=True)
    refined = run_test(str(src), "synthetic", win_size=64, check=True, refine=3)
    zero = run_test(str(src), "synthetic", win_size=64, check=True, refine=3, fit_shape=0)
    assert sorted(zero) == sorted(refined)
    for key in ("coco", "joints", "poses", "vertices", "poses_refined"):
        assert np.array_equal(zero[key], refined[key]), key
    assert np.array_equal(zero["fk_check_refined"]["per_joint"], refined["fk_check_refined"]["per_joint"])
    got = run_test(str(src), "synthetic", win_size=64, check=True, refine=3, fit_shape=2)
    assert sorted(got) == sorted(list(refined) + ["betas"])
    assert got["betas"].shape == (10,) and got["betas"].dtype == np.float32 and np.isfinite(got["betas"]).all()
    for key in ("poses", "joints"):
        assert np.array_equal(got[key], plain[key]), key
    assert np.array_equal(got["fk_check"]["per_joint"], plain["fk_check"]["per_joint"])
    assert got["poses_refined"].shape == plain["poses"].shape and got["poses_refined"].dtype == np.float32
    print(f"run_test fk_check mean: {got['fk_check']['mean']:.5f} -> {refined['fk_check_refined']['mean']:.5f} (--refine 3) "
          f"-> {got['fk_check_refined']['mean']:.5f} (--refine 3 --fit-shape 2)")
    assert np.isfinite(got["fk_check_refined"]["per_joint"]).all()
    with pytest.raises(ValueError):
        run_test(str(src), "synthetic", win_size=64, fit_shape=2, refine=0)
    with pytest.raises(ValueError):
        run_test(str(src), None, win_size=64, fit_shape=2, refine=3)
