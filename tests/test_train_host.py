"""CPU-side checks of the training loop's host half: calc_mean_losses against the
reference's semantics (pose_trainer.py:27-39, restated below), the command
line's argument names and defaults (pose_trainer.py:204-230, restated below as
a table), and the three validation / resume entry points of the C ABI refusing
null handles before touching the device."""
import numpy as np
import pytest
import torch


def _reference_calc_mean_losses(outputs, loss_keys):
    """pose_trainer.py:27-39, restated."""
    means = {k: 0.0 for k in loss_keys}
    cnts = {k: 0 for k in loss_keys}
    for o in outputs:
        for k in loss_keys:
            if k in o:
                means[k] += o[k]
                cnts[k] += 1
    for k in loss_keys:
        if cnts[k] > 0:
            means[k] /= cnts[k]
    return {k: v for k, v in means.items() if cnts[k] > 0}


@pytest.mark.parametrize("outputs", [
    [{"val_loss": 1.0, "pose_mse": 3.0}, {"val_loss": 2.0, "pose_mse": 5.0}],
    [{"val_loss": 1.0}, {"pose_mse": 4.0}, {"val_loss": 0.5, "pose_mse": 2.0, "other": 9.0}],
    [{"other": 1.0}],
    [],
])
def test_calc_mean_losses_matches_reference(outputs):
    from temporal_inverse_kinematics_amd.trainer import calc_mean_losses
    keys = ["pose_mse", "val_loss"]
    got = calc_mean_losses(outputs, keys)
    ref = _reference_calc_mean_losses(outputs, keys)
    assert list(got) == list(ref)
    for k in ref:
        assert got[k] == ref[k]


def test_calc_mean_losses_on_tensors():
    from temporal_inverse_kinematics_amd.trainer import calc_mean_losses
    outs = [{"val_loss": torch.tensor(0.25)}, {"val_loss": torch.tensor(0.75), "pose_mse": torch.tensor(2.0)}]
    got = calc_mean_losses(outs, ["pose_mse", "val_loss"])
    assert float(got["val_loss"]) == 0.5 and float(got["pose_mse"]) == 2.0


# pose_trainer.py:204-230 (add_model_specific_args + add_args)
REFERENCE_DEFAULTS = {
    "lr": 1e-4, "win_size": 9, "bs": 256, "kps_channel": 3, "graph_layout": "coco", "max_hop": 2, "dilation": 1,
    "keypoint_format": "coco", "n_out_joints": 22, "n_out_channels": 3,
    "amass": "/media/F/datasets/amass", "data_dir": "/media/F/datasets/amass/ik_model", "n_workers": 8,
    "max_epoch": 200, "smpl_mean": "/media/F/thesis/motion_capture/data/smpl/smpl_mean_params.npz",
    "n_train": -1, "n_valid": -1, "resume_ckpt": "",
}


def test_parser_defaults_match_reference():
    from temporal_inverse_kinematics_amd.trainer import build_parser
    hp = vars(build_parser().parse_args([]))
    for k, v in REFERENCE_DEFAULTS.items():
        assert hp[k] == v and type(hp[k]) is type(v), k
    assert hp["synthetic_smplx"] is False
    assert set(hp) == set(REFERENCE_DEFAULTS) | {"synthetic_smplx"}


def test_parser_takes_reference_arguments():
    from temporal_inverse_kinematics_amd.trainer import build_parser
    hp = build_parser().parse_args(["--amass", "a", "--data_dir", "d", "--max_epoch", "3", "--n_train", "5",
                                    "--n_valid", "2", "--resume_ckpt", "x.ckpt", "--lr", "0.01", "--win_size", "17",
                                    "--bs", "32", "--keypoint_format", "coco", "--graph_layout", "coco", "--max_hop",
                                    "2", "--dilation", "1", "--n_workers", "0"])
    assert (hp.amass, hp.data_dir, hp.max_epoch, hp.n_train, hp.n_valid) == ("a", "d", 3, 5, 2)
    assert (hp.resume_ckpt, hp.lr, hp.win_size, hp.bs, hp.n_workers) == ("x.ckpt", 0.01, 17, 32, 0)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--graph_layout", "nope"])


def test_eval_write_set_steps_reject_null_handles_without_gpu():
    from temporal_inverse_kinematics_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    with pytest.raises(ValueError, match="tik_trainer_eval"):
        _lib.check(lib.tik_trainer_eval(None, None, 1, 9, None, None, None, None))
    assert "tik_trainer_eval" in _lib.last_error()
    with pytest.raises(ValueError, match="tik_trainer_write"):
        _lib.check(lib.tik_trainer_write(None, 0, 0, None, None))
    assert "tik_trainer_write" in _lib.last_error()
    assert lib.tik_trainer_set_steps(None, 3) == _lib.TIK_E_INVALID
    assert "tik_trainer_set_steps" in _lib.last_error()
    assert np.all([s in _lib.SIGNATURES for s in ("tik_trainer_eval", "tik_trainer_write", "tik_trainer_set_steps")])
