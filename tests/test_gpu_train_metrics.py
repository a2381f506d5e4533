"""GpuTrainer(val_metrics=True): the validation step's mpjpe, pa_mpjpe and mpjae against SMPLX.pose_metrics per body
model on predict's poses (the same launch, so the per-frame bytes are the same; the accuracy of the metrics is
tests/test_gpu_pose_metrics.py's), with two body models whose rows split unevenly. Off, the step's keys are today's.
"""
import numpy as np
import pytest
import torch

import memedge as me
import pose_metrics_ref as P
import trainref as tref

pytestmark = pytest.mark.gpu
K = P.K
METRICS = ("mpjpe", "pa_mpjpe", "mpjae")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def two():
    """Two handles whose constants differ: small_consts(1, 1), and the same with v_template scaled by 1.1."""
    me.lib()
    c1 = dict(K.consts())
    c1["v_template"] = np.ascontiguousarray(c1["v_template"] * np.float32(1.1))
    return {"a": K.R.SMPLX(K.consts(), batch_size=9), "b": K.R.SMPLX(c1, batch_size=9)}


def val_batch(N, T, seed, gid):
    x, tgt, _ = tref.batch(N, T, seed)
    Tp = tgt.shape[1]
    kps = K.coco_of(tgt.reshape(-1, 66)).astype(np.float32).reshape(N, Tp, 17, 3)
    betas = np.random.default_rng(seed + 1000).normal(0, 1, (N, Tp, 10)).astype(np.float32)
    return {"keypoints_3d": cu(x), "poses": cu(tgt), "target_keypoints_3d": cu(kps), "betas": cu(betas),
            "gender_id": torch.tensor(gid, dtype=torch.int32)}


@pytest.mark.parametrize("N,T,seed,gid", [(5, 1, 31, [0, 0, 1, 0, 1]), (3, 64, 14, [1, 0, 1])])
def test_validation_step_metrics(two, N, T, seed, gid):
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    batch = val_batch(N, T, seed, gid)
    tr = GpuTrainer(tref.model(tref.weights(), T), lr=1e-4, smplx_models=two, val_metrics=True)
    out = tr.validation_step(batch)
    assert set(out) == {"val_loss", "pose_mse", "kp_mse", *METRICS}
    assert all(out[k].shape == () and out[k].is_cuda for k in METRICS)
    poses = tr.predict(batch["keypoints_3d"])["poses"]
    Tp = poses.shape[1]
    R = N * Tp
    rows_of = np.repeat(np.asarray(gid), Tp)
    assert 0 < (rows_of == 0).sum() != (rows_of == 1).sum() > 0                # the rows split unevenly
    table = torch.full((R, 4), float("nan"), device="cuda")
    for i, name in enumerate(sorted(two)):
        rows = torch.from_numpy(np.nonzero(rows_of == i)[0].astype(np.int32)).cuda()
        two[name].pose_metrics(poses.reshape(R, 66), batch["target_keypoints_3d"].reshape(R, 17, 3),
                               betas=batch["betas"].reshape(R, 10), target_poses=batch["poses"].reshape(R, 66), rows=rows,
                               out=table)
    per_frame = tr.pose_metrics(poses, batch["target_keypoints_3d"], batch["poses"], batch["betas"], batch["gender_id"])
    h = table.cpu().numpy().astype(np.float64)
    assert np.isfinite(h).all() and (h[:, 3] == 17.0).all()
    for c, k in enumerate(METRICS + ("weight",)):
        assert torch.equal(per_frame[k], table[:, c]), k                         # the same launch: the same bytes
    for c, k in enumerate(METRICS):
        want = h[:, c].mean()
        # a float32 sum of R non-negative terms and one division: (R + 1) roundings of at most 2^-24 of the sum each
        assert abs(float(out[k]) - want) <= (R + 1) * 2.0 ** -24 * want, (k, float(out[k]), want)
        assert want > 0
    # the epoch's end averages the keys it finds and logs them
    end = tr.validation_epoch_end([out, out])
    for k in METRICS:
        assert float(end["log"][f"val/{k}"]) == pytest.approx(float(out[k]), rel=1e-6)
    assert float(end["val_loss"]) == pytest.approx(float(out["val_loss"]), rel=1e-6)


def test_off_is_todays_step_and_construction_needs_models(two):
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    batch = val_batch(5, 1, 31, [0, 0, 1, 0, 1])
    sd = tref.weights()
    off = GpuTrainer(tref.model(sd, 1), lr=1e-4, smplx_models=two)
    on = GpuTrainer(tref.model(sd, 1), lr=1e-4, smplx_models=two, val_metrics=True)
    a, b = off.validation_step(batch), on.validation_step(batch)
    assert set(a) == {"val_loss", "pose_mse", "kp_mse"}
    for k in a:
        assert torch.equal(a[k], b[k]), k                                        # the option changes no bit of today's keys
    assert set(off.validation_epoch_end([a])["log"]) == {"val/pose_mse", "val/kp_mse", "val/val_loss"}
    plain = GpuTrainer(tref.model(sd, 1), lr=1e-4)
    assert set(plain.validation_step(batch)) == {"val_loss", "pose_mse"}
    with pytest.raises(ValueError, match="smplx_models"):
        GpuTrainer(tref.model(sd, 1), lr=1e-4, val_metrics=True)
    with pytest.raises(ValueError, match="smplx_models"):
        plain.pose_metrics(batch["poses"], batch["target_keypoints_3d"])
