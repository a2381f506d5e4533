"""The refinement drivers past one chunk of inference.MAX_WINDOWS_PER_CALL.

Every other refine test has F <= 8 against a chunk of 8192, so the chunk loops
of refine_poses, refine_smooth, fit_shape and refine_sequence, and the offsets
into fit_shape's buffer of partial sums, only ever run once there. Here the
chunk is shrunk below F and the result compared with the one-chunk run of the
same call. The kernels promise a body's bits for any batch size and place
(include/tik.h), and the torch reductions of the pose drivers are per frame,
so the comparison is bitwise wherever the runs of LM_RUN bodies that
lm_accumulate sums are the same in both runs (fit_shape's two cost values are
sums per chunk; at these inputs they come out the same to the bit as well).
Where a chunk is no multiple of LM_RUN the partial sums regroup: that case is
held to test_gpu_fit_shape.py's bound against the float64 reference instead.

The cases follow tests/test_gpu_fit_shape.py: the 77-vertex body
fk_jacobian_ref.small_consts(1, 1), default_rng(3), truth poses uniform in
+-0.3, theta0 = truth + N(0, 0.1^2), truth betas N(0, 1) rounded to fp32, the
keypoints the oracle's COCO-17 of the truth rounded to fp32.
"""
import numpy as np
import pytest

import fk_shape_ref as S
import memedge as me
import test_gpu_fit_shape as T

pytestmark = pytest.mark.gpu
PRIOR, SHAPE_W, LAM0 = T.PRIOR, T.SHAPE_W, T.LAM0
_CASES = {}


def case(F):
    """(theta0 (F,66) float32, keypoints (F,17,3) float32), computed once per F and left alone."""
    if F not in _CASES:
        rng = np.random.default_rng(T.SEED)
        truth = rng.uniform(-0.3, 0.3, (F, 66))
        th0 = (truth + rng.normal(0, 0.1, (F, 66))).astype(np.float32)
        betas = rng.normal(0, 1, 10).astype(np.float32).astype(np.float64)
        kps = S.coco_of(T.consts(), truth, betas).astype(np.float32).reshape(F, 17, 3)
        _CASES[F] = (th0, kps)
    return _CASES[F]


@pytest.fixture(scope="module")
def model():
    me.lib()
    return S.SMPLX(T.consts(), batch_size=9)


def one_chunk_and(monkeypatch, c, F, call):
    """call() with all F frames in one chunk, then with chunks of c < F frames."""
    from temporal_inverse_kinematics_amd import inference
    assert c < F <= inference.MAX_WINDOWS_PER_CALL
    one = call()
    monkeypatch.setattr(inference, "MAX_WINDOWS_PER_CALL", c)
    return one, call()


def assert_same_bits(one, many):
    assert sorted(one) == sorted(many)
    differ = [k for k in one if not np.array_equal(one[k], many[k], equal_nan=True)]
    for k in differ:
        print(f"{k}: max |chunked - one chunk| = {np.abs(many[k].astype(np.float64) - one[k]).max():.3e}")
    assert not differ
    for k in one:
        assert np.isfinite(one[k]).all(), k


def test_refine_poses_in_three_chunks(model, monkeypatch):
    from temporal_inverse_kinematics_amd.refine import refine_poses
    F = 8
    th0, kps = case(F)
    one, many = one_chunk_and(monkeypatch, 3, F, lambda: refine_poses(th0, kps, model, iters=3, prior_weight=PRIOR, lam0=LAM0))
    assert one["cost"].shape == (4, F) and (one["cost"][-1] < one["cost"][0]).all()
    assert_same_bits(one, many)


def test_refine_smooth_chunk_edge_inside_a_sequence(model, monkeypatch):
    from temporal_inverse_kinematics_amd.refine import refine_smooth
    F = 8
    th0, kps = case(F)
    holes = kps.copy()
    holes[6] = np.nan
    w = np.ones((F, 17), np.float32)
    w[1, 9], w[4, [15, 16]] = 0.5, 0.0
    one, many = one_chunk_and(monkeypatch, 5, F, lambda: refine_smooth(
        th0, holes, model, 0.1, iters=3, prior_weight=PRIOR, joint_weight=w, lam0=LAM0, seq_starts=[0, 3, 8]))
    assert one["cost"].shape == (4, 2) and (one["cost"][-1] < one["cost"][0]).all()
    assert_same_bits(one, many)


def test_fit_shape_and_refine_sequence_across_a_whole_run(model, monkeypatch):
    """F = 40 in chunks of 32 = LM_RUN: lm_accumulate's runs are bodies 0..31 and 32..39 either way."""
    from temporal_inverse_kinematics_amd.refine import fit_shape, refine_sequence
    F, c = 40, 32
    assert c % S.LM_RUN == 0
    th0, kps = case(F)

    def call():
        out = {"fit." + k: v for k, v in fit_shape(th0, kps, model, shape_weight=SHAPE_W).items()}
        for smooth in (0.0, 0.1):
            seq = refine_sequence(th0, kps, model, rounds=1, iters=2, prior_weight=PRIOR, shape_weight=SHAPE_W, lam0=LAM0,
                                  smooth_weight=smooth)
            out.update({f"seq{smooth}.{k}": v for k, v in seq.items()})
        return out
    one, many = one_chunk_and(monkeypatch, c, F, call)
    assert one["fit.cost"][1] < one["fit.cost"][0] and np.abs(one["fit.betas"]).max() > 0.1
    for smooth in (0.0, 0.1):
        assert one[f"seq{smooth}.cost"][1] < one[f"seq{smooth}.cost"][0]
    assert_same_bits(one, many)


def test_fit_shape_chunk_that_regroups_the_partial_sums(model, monkeypatch):
    """test_gpu_fit_shape.py's F = 6 in chunks of 4: the sums are over bodies 0..3 and 4..5, then added."""
    from temporal_inverse_kinematics_amd.refine import fit_shape
    c = T.case()
    ref = S.fit_shape(T.consts(), c["truth"], c["kps"], None, SHAPE_W)
    th = c["truth"].astype(np.float32)
    one, many = one_chunk_and(monkeypatch, 4, T.F, lambda: fit_shape(th, c["kps32"], model, shape_weight=SHAPE_W))
    for name, out in (("one chunk", one), ("chunks of 4", many)):
        diff = np.abs(out["betas"].astype(np.float64) - ref["betas"]).max()
        print(f"{name}: max |betas(GPU) - betas(float64)| = {diff:.3e} (bound {T.BETAS_BOUND:.1e}); GPU cost {out['cost']}")
        assert diff < T.BETAS_BOUND
    assert abs(many["cost"][0] - ref["cost"][0]) < 1e-4 * T.F and many["cost"][1] < many["cost"][0]
