"""The training step on the GPU (optimizer half).

`GpuTrainer` runs what Lightning does with `IKPoseTrainer` for one batch
(pose_trainer.py:146-155 `training_step`, the backward, and the Adam step
from `configure_optimizers`, :196-197) as one stream-ordered call into
libtik.so (`tik_trainer_step`, csrc/train_step.cpp; the handle in
csrc/train_model.cpp, the state dict's validation and layout in csrc/train_plan.h):

  * train-mode forward: BatchNorm on batch statistics with the running-stat
    momentum update (st_gcn_aaai18.py:74-75,178,186,203), Dropout(0.7) in the
    head (pose_trainer.py:91), the learnable edge importance (:104-108,129);
  * nn.MSELoss(poses, batch["poses"]) (PoseLosses, pose_trainer.py:42-50);
  * the backward of every operation and torch.optim.Adam(lr=hparams.lr).

Parameters, gradients, Adam state and BatchNorm buffers stay on the device
between steps; `state_dict()` / `load_into(module)` export them under the
reference's names (the weight ABI of SURVEY.md §8b), so a trained model
drops straight into `PoseRegressor` inference or a `.ckpt`.

Around the step: `predict` / `validation_step` run the eval-mode forward on
the live device weights (`tik_trainer_eval`: running statistics folded on the
device, no dropout, the fp32 arithmetic being trained; :158-172),
`save_checkpoint` / `from_checkpoint` write and resume Lightning-shaped
`.ckpt` files with the Adam state, `fit` is the epoch loop with top-k
checkpoints and `on_epoch_end` (:174-177, :240-256), and `run_train`
(`python -m temporal_inverse_kinematics_amd.trainer`) is the reference's
command line.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import sys
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .models import IKPoseTrainer, PoseRegressor, _Handle, _state_numpy

_WHAT = {"value": 0, "grad": 1, "exp_avg": 2, "exp_avg_sq": 3}
_CKPT_NAME = re.compile(r"^checkpoint_epoch=(\d+)-val_loss=(-?\d+\.\d\d|nan|inf)\.ckpt$")
KP_POSE_DIM, KP_JOINTS = 66, 17   # include/tik.h, tik_trainer_step_kp
VAL_METRICS = ("mpjpe", "pa_mpjpe", "mpjae")   # validation_step's extra keys with val_metrics (SMPLX.pose_metrics)


def check_kp_args(kp_weight, n_models: int, pose_dim: int = KP_POSE_DIM, N=None, To=None, num_betas=None,
                  target_keypoints=None, betas=None, gender_id=None, kp_joint_weight=None) -> float:
    """The keypoint term's arguments of GpuTrainer, constructor and step alike -> kp_weight as a float.
    A pure function of shapes and host values: neither the library nor the device is touched.
    n_models: body models given (0: none). With N and To (the step's batch): target_keypoints must be
    (N,To,17,3), betas None, (nb,), (N,nb) or (N,To,nb), gender_id None (one model only) or N integers in [0, n_models)
    (a host sequence or array). ValueError: kp_weight negative or NaN; kp_weight > 0 without body models; with
    body models a pose_dim other than 66, a wrong shape, an unknown gender index, kp_joint_weight not (17,)."""
    w = float(kp_weight)
    if not w >= 0.0 or w == float("inf"):
        raise ValueError(f"kp_weight must be >= 0 and finite, got {kp_weight}")
    if n_models == 0:
        if w > 0.0:
            raise ValueError("kp_weight > 0 needs smplx_models: the keypoint term runs FK on the predicted poses")
        return w
    if not 1 <= n_models <= 3:
        raise ValueError(f"the keypoint term takes 1..3 body models, got {n_models}")
    if int(pose_dim) != KP_POSE_DIM:
        raise ValueError(f"the keypoint term needs pose_dim {KP_POSE_DIM} (22 joints x 3), the model has {pose_dim}")
    if kp_joint_weight is not None and tuple(np.shape(kp_joint_weight)) != (KP_JOINTS,):
        raise ValueError(f"kp_joint_weight must be ({KP_JOINTS},), got {tuple(np.shape(kp_joint_weight))}")
    if N is None:
        return w
    if target_keypoints is None or tuple(target_keypoints.shape) != (N, To, KP_JOINTS, 3):
        got = None if target_keypoints is None else tuple(target_keypoints.shape)
        raise ValueError(f"target_keypoints must be {(N, To, KP_JOINTS, 3)}, got {got}")
    if betas is not None and tuple(betas.shape) not in ((num_betas,), (N, num_betas), (N, To, num_betas)):
        raise ValueError(f"betas must be {(num_betas,)}, {(N, num_betas)} or {(N, To, num_betas)}, got {tuple(betas.shape)}")
    if gender_id is None:
        if n_models != 1:
            raise ValueError(f"gender_id is required with {n_models} body models")
        return w
    g = np.asarray(gender_id)
    if g.shape != (N,) or g.dtype.kind not in "iu":
        raise ValueError(f"gender_id must be {(N,)} integers, got {g.dtype} {g.shape}")
    if N and (g.min() < 0 or g.max() >= n_models):
        raise ValueError(f"gender_id holds an index outside [0, {n_models}): the body models are sorted(smplx_models)")
    return w


def _rows_betas(b: torch.Tensor, To: int) -> torch.Tensor:
    """betas (nb,), (N,nb) or (N,T',nb) -> one shared row (nb,) or one row per pose row (N T', nb), contiguous."""
    if b.dim() == 2:
        b = b.repeat_interleave(To, 0)
    elif b.dim() == 3:
        b = b.reshape(-1, b.shape[2])
    return b.contiguous()


class GpuTrainer:
    """IKPoseTrainer's training loop body on the GPU.

    >>> tr = GpuTrainer(IKPoseTrainer(hparams))      # lr = hparams.lr
    >>> out = tr.training_step(batch, 0)             # forward + MSE + backward + Adam
    >>> out["loss"], out["log"]["train/pose_mse"]
    """

    def __init__(self, model, lr: Optional[float] = None, device="cuda", smplx_models=None, kp_weight: float = 0.0,
                 kp_joint_weight=None, val_metrics: bool = False):
        """smplx_models ({gender: SMPLX}, at most 3) switches the keypoint term on: the step
        becomes tik_trainer_step_kp, loss = pose_mse + kp_weight * kp_mse with kp_mse the
        nn.MSELoss of rel(FK(predicted poses)) against rel(batch["target_keypoints_3d"]),
        back-propagated through FK. kp_weight = 0 only monitors kp_mse (the update keeps the
        bits of the plain step). kp_joint_weight: 17 non-negative keypoint weights or None.
        val_metrics=True (needs smplx_models): validation_step also reports mpjpe, pa_mpjpe
        and mpjae (pose_metrics below); off, every dict is what it is without the option."""
        reg = model.regressor if isinstance(model, IKPoseTrainer) else model
        if not isinstance(reg, PoseRegressor):
            raise TypeError("GpuTrainer expects an IKPoseTrainer or PoseRegressor")
        self.smplx_models = dict(smplx_models) if smplx_models else None
        self._genders = sorted(self.smplx_models) if self.smplx_models else []
        self.kp_weight = check_kp_args(kp_weight, len(self._genders), reg.pose_dim, kp_joint_weight=kp_joint_weight)
        self.val_metrics = bool(val_metrics)
        if self.val_metrics and not self.smplx_models:
            raise ValueError("val_metrics=True needs smplx_models: the metrics run FK on the predicted poses")
        self._kp_jw = None
        if kp_joint_weight is not None and self.smplx_models:
            self._kp_jw = torch.as_tensor(np.asarray(kp_joint_weight, np.float32)).to(device).contiguous()
        hp = getattr(model, "hparams", None)
        if lr is None:
            lr = float(getattr(hp, "lr", 1e-4)) if hp is not None else 1e-4
        self.lr = float(lr)
        self.hparams = hp
        self.device = torch.device(device)
        self.regressor = reg
        named = _state_numpy(reg)
        named.append(("tik.strides", np.array(reg.backbone.strides, dtype=np.float32)))
        arr, keep = _lib.pack_tensors(named)
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.tik_trainer_create(arr, len(named), ctypes.c_float(self.lr), ctypes.byref(h)), "GpuTrainer")
        self._h = _Handle(h.value, lib.tik_trainer_destroy)
        self._names = []
        for i in range(_lib.check(lib.tik_trainer_count(self._h.h))):
            name = ctypes.create_string_buffer(256)
            shape = (ctypes.c_int64 * 4)()
            nd, kind = ctypes.c_int(), ctypes.c_int()
            _lib.check(lib.tik_trainer_tensor(self._h.h, i, name, 256, shape, ctypes.byref(nd), ctypes.byref(kind)))
            self._names.append((name.value.decode(), tuple(shape[:nd.value]), kind.value))
        self._index = {n: i for i, (n, _, _) in enumerate(self._names)}
        self._loss = torch.zeros(1, device=self.device)
        self._parts = torch.zeros(2, device=self.device)   # {pose_mse, kp_mse} of the last keypoint step
        # the BatchNorm step counters the model arrived with (checkpoint / earlier training)
        self._nbt0 = {k: int(v.item()) for k, v in reg.state_dict().items() if k.endswith("num_batches_tracked")}

    # ------------------------------------------------------------------ step
    def step(self, keypoints_3d: torch.Tensor, poses: torch.Tensor, dropout_mask: Optional[torch.Tensor] = None,
             seed: int = 0, target_keypoints=None, betas=None, gender_id=None) -> torch.Tensor:
        """One optimizer step on (keypoints_3d (N,T,17,3), poses (N,T',66)); returns the
        pre-update loss as a device scalar. `dropout_mask` (N*T', 512) of 0/1 fixes the
        head's dropout draw (tests); otherwise a counter-based mask keyed by `seed`.
        With smplx_models (tik_trainer_step_kp): target_keypoints (N,T',17,3) the clean
        keypoints of the target poses (not root-relative: the kernel applies rel), betas
        None, (nb,), (N,nb) (a window's betas serve its T' rows) or (N,T',nb), gender_id (N,) integers
        indexing sorted(smplx_models) (None with one model); the loss returned is
        pose_mse + kp_weight * kp_mse and `last_loss_parts` holds the two terms."""
        x = keypoints_3d.contiguous()
        y = poses.contiguous()
        _lib.require_gpu(x, y)
        if x.dim() != 4 or x.shape[2:] != (17, 3):
            raise ValueError(f"expected (N,T,17,3) keypoints, got {tuple(x.shape)}")
        N, T = x.shape[:2]
        lib = _lib.load()
        To = _lib.check(lib.tik_trainer_out_frames(self._h.h, T))
        if tuple(y.shape) != (N, To, self.regressor.pose_dim):
            raise ValueError(f"expected target poses {(N, To, self.regressor.pose_dim)}, got {tuple(y.shape)}")
        if x.dtype != torch.float32 or y.dtype != torch.float32:
            raise TypeError("keypoints and poses must be float32")
        mptr = None
        if dropout_mask is not None:
            dropout_mask = dropout_mask.to(self.device, torch.float32).contiguous()
            if dropout_mask.numel() != N * To * 512:
                raise ValueError("dropout_mask must hold N*T'*512 values")
            mptr = dropout_mask.data_ptr()
        if self.smplx_models:
            self._step_kp(lib, x, y, N, T, To, mptr, int(seed) & (2**64 - 1), target_keypoints, betas, gender_id)
            return self._loss[0].clone()
        _lib.check(lib.tik_trainer_step(self._h.h, x.data_ptr(), N, T, y.data_ptr(), mptr, int(seed) & (2**64 - 1),
                                        self._loss.data_ptr(), _lib.stream_of(x)), "GpuTrainer.step")
        # a fresh tensor per step (the reference returns a new loss each step;
        # the persistent device buffer is overwritten by the next step)
        return self._loss[0].clone()

    def _step_kp(self, lib, x, y, N, T, To, mptr, seed, target_keypoints, betas, gender_id):
        """The tik_trainer_step_kp call: every check on the host first, the per-model row lists built on the device."""
        models = [self.smplx_models[g] for g in self._genders]
        nb = models[0].num_betas
        gid_host = None
        if gender_id is not None:
            gid_host = gender_id.detach().cpu().numpy() if isinstance(gender_id, torch.Tensor) else np.asarray(gender_id)
        check_kp_args(self.kp_weight, len(models), self.regressor.pose_dim, N, To, nb, target_keypoints, betas, gid_host)
        kps = target_keypoints.to(self.device, torch.float32).contiguous()
        R = N * To
        kp = _lib.TikKpLoss()
        kp.n_models = len(models)
        keep = [kps]
        if gid_host is None:
            kp.fk[0], kp.rows[0], kp.n_rows[0] = models[0]._h, None, R
        else:
            # the row lists on the device, back to back in one tensor: a stable sort of the rows by model keeps each list
            # ascending; the counts come from the host copy the check has read already (no further synchronisation)
            gid = (gender_id if isinstance(gender_id, torch.Tensor) else torch.as_tensor(gid_host)).to(self.device)
            rows = torch.argsort(gid.long().repeat_interleave(To), stable=True).to(torch.int32).contiguous()
            keep.append(rows)
            counts = np.bincount(gid_host.astype(np.int64), minlength=len(models)) * To
            off = 0
            for i, m in enumerate(models):
                # an empty list still gets a non-null pointer: the all-rows case is the only null
                kp.fk[i], kp.rows[i], kp.n_rows[i] = m._h, rows.data_ptr() + 4 * off, int(counts[i])
                off += int(counts[i])
        kp.kps = kps.data_ptr()
        if betas is not None:
            b = _rows_betas(betas.to(self.device, torch.float32), To)
            keep.append(b)
            kp.betas, kp.betas_ld = b.data_ptr(), (nb if b.dim() == 2 else 0)
        kp.joint_w = _lib.ptr(self._kp_jw) or None
        kp.weight = self.kp_weight
        _lib.check(lib.tik_trainer_step_kp(self._h.h, x.data_ptr(), N, T, y.data_ptr(), mptr, seed, ctypes.byref(kp),
                                           self._loss.data_ptr(), self._parts.data_ptr(), _lib.stream_of(x)),
                   "GpuTrainer.step")
        self._kp_keep = keep   # the step is stream-ordered: its inputs live until the next one replaces them

    @property
    def last_loss_parts(self) -> torch.Tensor:
        """{pose_mse, kp_mse} of the last keypoint step, a fresh (2,) device tensor."""
        return self._parts.clone()

    def training_step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0, dropout_mask=None):
        """pose_trainer.py:146-155 plus Lightning's backward and optimizer step. With
        smplx_models the batch also carries target_keypoints_3d, betas and (more than one
        model) gender_id, and the log has both terms of the loss."""
        seed = self.steps * 1000003 + batch_idx
        if not self.smplx_models:
            loss = self.step(batch["keypoints_3d"].to(self.device), batch["poses"].to(self.device), dropout_mask, seed=seed)
            return {"loss": loss, "log": {"train/pose_mse": loss}}
        loss = self.step(batch["keypoints_3d"].to(self.device), batch["poses"].to(self.device), dropout_mask, seed=seed,
                         target_keypoints=batch["target_keypoints_3d"], betas=batch.get("betas"),
                         gender_id=batch.get("gender_id"))
        parts = self.last_loss_parts
        return {"loss": loss, "log": {"train/pose_mse": parts[0], "train/kp_mse": parts[1]}}

    # ------------------------------------------------------------------ state
    @property
    def steps(self) -> int:
        return int(_lib.load().tik_trainer_steps(self._h.h))

    def tensor(self, name: str, what: str = "value") -> torch.Tensor:
        i = self._index[name]
        _, shape, _ = self._names[i]
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        _lib.check(_lib.load().tik_trainer_read(self._h.h, i, _WHAT[what], out.data_ptr(),
                                                _lib.stream_of(out)), name)
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """PoseRegressor state dict after the last step (reference key names)."""
        sd = {n: self.tensor(n) for n, _, _ in self._names}
        # each BatchNorm counts on from the value it was loaded with (nn.BatchNorm increments its own buffer)
        for k, v0 in self._nbt0.items():
            sd[k] = torch.tensor(v0 + self.steps, dtype=torch.long)
        return sd

    def grads(self) -> Dict[str, torch.Tensor]:
        return {n: self.tensor(n, "grad") for n, _, k in self._names if k == 0}

    _SAVED = {"O": 0, "U": 2, "H": 3, "Z": 4, "Y": 5, "P": 6, "poses": 7, "dposes": 8}

    def saved(self, kind: str, layer: int, shape) -> torch.Tensor:
        """The last step's saved forward activation (test / debug hook): block `layer`'s
        output "O", tcn conv output "U", post-ReLU tcn input "H", graph-mix output "Z",
        gcn conv output "Y" (channels-last (N,T,17,C)); "P" the head's first Linear
        output (N*T', 512); "poses" the head's train-mode output and "dposes" the loss
        gradient with respect to it (layer 0, (N*T', 66))."""
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        _lib.check(_lib.load().tik_trainer_debug(self._h.h, self._SAVED[kind], layer, out.data_ptr(), out.numel(),
                                                 _lib.stream_of(out)), "saved")
        return out

    def load_into(self, module=None):
        """Copy the trained state into `module` (default: the regressor it was built from)."""
        reg = self.regressor if module is None else (module.regressor if isinstance(module, IKPoseTrainer) else module)
        own = reg.state_dict()
        sd = {k: v.to(own[k].device, own[k].dtype) for k, v in self.state_dict().items() if k in own}
        reg.load_state_dict(sd, strict=False)
        return reg

    def write_tensor(self, name: str, src: torch.Tensor, what: str = "value") -> None:
        """The inverse of `tensor`: a device tensor -> the value / grad / exp_avg /
        exp_avg_sq of `name` (tik_trainer_write). Buffers have a value only."""
        i = self._index[name]
        _, shape, _ = self._names[i]
        src = src.contiguous()
        _lib.require_gpu(src)    # on the device (RuntimeError), float32 (TypeError)
        if tuple(src.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(src.shape)}")
        _lib.check(_lib.load().tik_trainer_write(self._h.h, i, _WHAT[what], src.data_ptr(), _lib.stream_of(src)), name)

    # ------------------------------------------------------------------ eval
    def evaluate(self, keypoints_3d: torch.Tensor, poses: Optional[torch.Tensor] = None, want_poses: bool = True):
        """Eval-mode forward on the live weights (tik_trainer_eval): BatchNorm on the
        running statistics, no dropout, the trainer's own fp32 arithmetic. Returns
        (predicted poses (N,T',66) or None, MSE against `poses` as a fresh device
        scalar or None). Changes no trainer state."""
        x = keypoints_3d.contiguous()
        y = None if poses is None else poses.contiguous()
        _lib.require_gpu(x, y)   # on the device (RuntimeError), float32 (TypeError): the kernels read fp32
        if x.dim() != 4 or x.shape[2:] != (17, 3):
            raise ValueError(f"expected (N,T,17,3) keypoints, got {tuple(x.shape)}")
        N, T = x.shape[:2]
        lib = _lib.load()
        To = _lib.check(lib.tik_trainer_out_frames(self._h.h, T)) if T > 0 else 0
        if y is not None and tuple(y.shape) != (N, To, self.regressor.pose_dim):
            raise ValueError(f"expected target poses {(N, To, self.regressor.pose_dim)}, got {tuple(y.shape)}")
        out = torch.empty((N, To, self.regressor.pose_dim), device=x.device, dtype=torch.float32) if want_poses else None
        loss = torch.empty((), device=x.device, dtype=torch.float32) if y is not None else None
        if N == 0 or T == 0:
            if loss is not None:
                loss.fill_(float("nan"))   # the mean over no elements, as nn.MSELoss gives
            return out, loss
        _lib.check(lib.tik_trainer_eval(self._h.h, x.data_ptr(), N, T, _lib.ptr(y), _lib.ptr(out), _lib.ptr(loss),
                                        _lib.stream_of(x)), "GpuTrainer.evaluate")
        return out, loss

    def predict(self, keypoints_3d: torch.Tensor) -> Dict[str, torch.Tensor]:
        """IKPoseTrainer.forward in eval mode on the weights being trained -> {"poses": (N,T',66)}."""
        return {"poses": self.evaluate(keypoints_3d)[0]}

    def validation_step(self, batch: Dict[str, torch.Tensor], batch_idx: int = 0):
        """pose_trainer.py:158-164; the loss is a fresh device scalar each call."""
        if not self.smplx_models:
            _, lss = self.evaluate(batch["keypoints_3d"].to(self.device), batch["poses"].to(self.device), want_poses=False)
            return {"val_loss": lss, "pose_mse": lss}
        poses, lss = self.evaluate(batch["keypoints_3d"].to(self.device), batch["poses"].to(self.device))
        kp = self.keypoint_mse(poses, batch["target_keypoints_3d"], batch.get("betas"), batch.get("gender_id"))
        out = {"val_loss": lss + self.kp_weight * kp, "pose_mse": lss, "kp_mse": kp}
        if self.val_metrics:
            m = self.pose_metrics(poses, batch["target_keypoints_3d"], batch["poses"].to(self.device), batch.get("betas"),
                                  batch.get("gender_id"))
            for k in VAL_METRICS:   # a device scalar: the mean over the frames with W > 0 that have a value (NaN where none has)
                has = (m["weight"] > 0) & torch.isfinite(m[k])
                out[k] = torch.where(has, m[k], torch.zeros_like(m[k])).sum() / has.sum()
        return out

    def pose_metrics(self, poses, target_keypoints, target_poses=None, betas=None, gender_id=None) -> Dict[str, torch.Tensor]:
        """SMPLX.pose_metrics of poses (N,T',66) against target_keypoints (N,T',17,3) and
        target_poses (N,T',66) or None: one launch per body model on its rows, as
        keypoint_mse walks them -> {"mpjpe", "pa_mpjpe", "mpjae", "weight"}, each (N T',)
        and a view of one (N T', 4) device tensor. The keypoint weights are the trainer's
        kp_joint_weight. validation_step averages each over the frames with W > 0 that have
        a value: a frame with fewer than 3 positive weights has no pa_mpjpe and is left out
        of that mean alone (a kp_joint_weight with fewer than 3 positive entries leaves
        val/pa_mpjpe NaN)."""
        if not self.smplx_models:
            raise ValueError("pose_metrics needs smplx_models: the metrics run FK on the poses")
        N, To = int(poses.shape[0]), int(poses.shape[1])
        models = [self.smplx_models[g] for g in self._genders]
        gid_host = None
        if gender_id is not None:
            gid_host = gender_id.detach().cpu().numpy() if isinstance(gender_id, torch.Tensor) else np.asarray(gender_id)
        check_kp_args(self.kp_weight, len(models), poses.shape[2], N, To, models[0].num_betas, target_keypoints, betas, gid_host)
        R = N * To
        if target_poses is not None and tuple(target_poses.shape) != (N, To, KP_POSE_DIM):
            raise ValueError(f"expected target poses {(N, To, KP_POSE_DIM)}, got {tuple(target_poses.shape)}")
        P = poses.reshape(R, KP_POSE_DIM).contiguous()
        K = target_keypoints.to(self.device, torch.float32).reshape(R, KP_JOINTS, 3).contiguous()
        Tp = None if target_poses is None else target_poses.to(self.device, torch.float32).reshape(R, KP_POSE_DIM).contiguous()
        b = None if betas is None else _rows_betas(betas.to(self.device, torch.float32), To)
        out = torch.full((R, 4), float("nan"), device=self.device)
        gid = None if gid_host is None else torch.as_tensor(gid_host.astype(np.int64)).to(self.device).repeat_interleave(To)
        for i, m in enumerate(models):
            rows = None if gid is None else torch.nonzero(gid == i).flatten().to(torch.int32).contiguous()
            m.pose_metrics(P, K, betas=b, joint_weight=self._kp_jw, target_poses=Tp, rows=rows, out=out)
        return {"mpjpe": out[:, 0], "pa_mpjpe": out[:, 1], "mpjae": out[:, 2], "weight": out[:, 3]}

    def keypoint_mse(self, poses, target_keypoints, betas=None, gender_id=None) -> torch.Tensor:
        """kp_mse of poses (N,T',66) against target_keypoints (N,T',17,3), the step's
        normalisation 2 sum(loss) / (51 N T'), through SMPLX.keypoint_loss per body model."""
        N, To = int(poses.shape[0]), int(poses.shape[1])
        models = [self.smplx_models[g] for g in self._genders]
        gid_host = None
        if gender_id is not None:
            gid_host = gender_id.detach().cpu().numpy() if isinstance(gender_id, torch.Tensor) else np.asarray(gender_id)
        check_kp_args(self.kp_weight, len(models), poses.shape[2], N, To, models[0].num_betas, target_keypoints, betas, gid_host)
        R = N * To
        P = poses.reshape(R, KP_POSE_DIM).contiguous()
        K = target_keypoints.to(self.device, torch.float32).reshape(R, KP_JOINTS, 3).contiguous()
        b = None
        if betas is not None:
            b = _rows_betas(betas.to(self.device, torch.float32), To)
        loss = torch.zeros(R, device=self.device)
        grad = torch.empty((R, KP_POSE_DIM), device=self.device)
        for i, m in enumerate(models):
            rows = None
            if gid_host is not None:
                gid = torch.as_tensor(gid_host.astype(np.int64)).to(self.device).repeat_interleave(To)
                rows = torch.nonzero(gid == i).flatten().to(torch.int32).contiguous()
            m.keypoint_loss(P, K, betas=b, joint_weight=self._kp_jw, rows=rows, out_loss=loss, out_grad=grad)
        return loss.double().sum().mul(2.0 / (51.0 * R)).float()

    def validation_epoch_end(self, outputs):
        """pose_trainer.py:166-172: the mean of the batch means."""
        losses = calc_mean_losses(outputs, ["pose_mse", "kp_mse", "val_loss", *VAL_METRICS])
        return {"val_loss": losses["val_loss"], "log": {f"val/{k}": v for k, v in losses.items()}}

    def validate(self, val_ds, batch_size: int):
        """One pass over `val_ds` in dataset order -> validation_epoch_end's dict."""
        n = len(val_ds)
        outs = [self.validation_step(val_ds.get_batch(np.arange(lo, min(lo + batch_size, n))), b)
                for b, lo in enumerate(range(0, n, batch_size))]
        return self.validation_epoch_end(outs)

    # ------------------------------------------------------------------ checkpoints
    def _param_order(self):
        """regressor.named_parameters() order: the index of torch.optim.Adam's state."""
        return [n for n, _ in self.regressor.named_parameters()]

    def save_checkpoint(self, path, epoch: int, **extra) -> str:
        """A `.ckpt` that IKPoseTrainer.load_from_checkpoint and `from_checkpoint` read
        (plain tensors and containers: torch.load(weights_only=True) accepts it):
        epoch, global_step, state_dict (`regressor.` keys, BatchNorm counters
        included), hparams (a dict), optimizer_states = [torch.optim.Adam.state_dict()
        layout], plus `extra` (fit stores val_loss)."""
        steps = self.steps
        names = self._param_order()
        hp = getattr(self, "hparams", None)
        hpd = {k: v for k, v in (vars(hp) if hp is not None else {}).items()
               if isinstance(v, (bool, int, float, str, type(None)))}
        hpd["lr"] = self.lr
        state = {i: {"step": torch.tensor(float(steps), dtype=torch.float32),
                     "exp_avg": self.tensor(n, "exp_avg").cpu(), "exp_avg_sq": self.tensor(n, "exp_avg_sq").cpu()}
                 for i, n in enumerate(names)}
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(names)))}
        ck = {"epoch": int(epoch), "global_step": int(steps),
              "state_dict": {"regressor." + k: v.cpu() for k, v in self.state_dict().items()},
              "hparams": hpd, "optimizer_states": [{"state": state, "param_groups": [group]}]}
        ck.update(extra)
        os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
        torch.save(ck, str(path))
        return str(path)

    def _restore(self, path, device, **kp_kwargs) -> dict:
        """Rebuild this trainer from a checkpoint: weights and running statistics
        (IKPoseTrainer.load_from_checkpoint), both Adam moments, steps and lr. A file
        without optimizer_states gives fresh Adam state and steps = 0.

        This re-runs __init__ on `self`: the device handle, `regressor`, `hparams`
        and `lr` become the checkpoint's, as Lightning's resume_from_checkpoint
        replaces the module's and the optimizer's state. The file is read twice
        (by load_from_checkpoint for the model, here for the optimizer state),
        with the allow-list load_from_checkpoint has already registered."""
        model = IKPoseTrainer.load_from_checkpoint(str(path))
        ck = torch.load(str(path), map_location="cpu", weights_only=True)
        opt = (ck.get("optimizer_states") or [None])[0]
        lr = float(opt["param_groups"][0]["lr"]) if opt else None
        GpuTrainer.__init__(self, model, lr=lr, device=device, **kp_kwargs)
        if opt:
            for i, n in enumerate(self._param_order()):
                st = opt["state"].get(i)
                if st is None:
                    continue
                self.write_tensor(n, st["exp_avg"].to(self.device, torch.float32), "exp_avg")
                self.write_tensor(n, st["exp_avg_sq"].to(self.device, torch.float32), "exp_avg_sq")
            steps = int(ck.get("global_step", 0))
            _lib.check(_lib.load().tik_trainer_set_steps(self._h.h, steps), "from_checkpoint")
            # the saved counters already include these steps; state_dict() adds `steps` again
            self._nbt0 = {k: v - steps for k, v in self._nbt0.items()}
        return ck

    @classmethod
    def from_checkpoint(cls, path, device="cuda", smplx_models=None, kp_weight: float = 0.0,
                        kp_joint_weight=None, val_metrics: bool = False) -> "GpuTrainer":
        """A trainer that continues where `save_checkpoint` stopped. The keypoint term's
        arguments are the constructor's: the checkpoint does not store them."""
        tr = cls.__new__(cls)
        tr._restore(path, device, smplx_models=smplx_models, kp_weight=kp_weight, kp_joint_weight=kp_joint_weight,
                    val_metrics=val_metrics)
        return tr

    # ------------------------------------------------------------------ fit
    def fit(self, train_ds, val_ds=None, *, max_epochs: int, batch_size: int, ckpt_dir=None, save_top_k: int = 30,
            resume_ckpt=None, shuffle_seed: int = 0) -> List[dict]:
        """The Lightning loop of pose_trainer.py:233-256 without Lightning.

        Per epoch: the train set in a permutation drawn from
        RandomState(shuffle_seed * 1000003 + epoch) (a function of the epoch alone, so
        a resumed run draws the same batches), batches from `ds.get_batch`; then
        validation in dataset order, `checkpoint_epoch={e}-val_loss={v:.2f}.ckpt`
        under `ckpt_dir` (the `save_top_k` lowest val_loss stay; < 0 keeps all, 0
        writes none), then `train_ds.on_epoch_end(e)` (:174-177). Without `val_ds`
        val_loss is the epoch's mean train loss. `resume_ckpt` (epoch e) restores
        this trainer in place (weights, Adam state, steps, and `lr` / `hparams` /
        `regressor` from the file: see `_restore`), counts the checkpoints of epochs
        <= e already in `ckpt_dir` toward `save_top_k`, and continues at e + 1;
        `max_epochs` counts from epoch 0.
        Returns one {"epoch", "train/pose_mse", "val_loss", "ckpt"} per epoch run; with
        val_metrics and a validation set also "val/mpjpe", "val/pa_mpjpe", "val/mpjae".
        The checkpoints are ranked by val_loss either way."""
        start, kept = 0, []
        ckpt_dir = None if ckpt_dir is None else str(ckpt_dir)
        if resume_ckpt:
            ck = self._restore(resume_ckpt, self.device, smplx_models=self.smplx_models, kp_weight=self.kp_weight,
                               kp_joint_weight=None if self._kp_jw is None else self._kp_jw.cpu().numpy(),
                               val_metrics=self.val_metrics)
            e = int(ck["epoch"])
            train_ds.on_epoch_end(e)
            start = e + 1
            # the interrupted run's files count toward save_top_k: earlier epochs by the
            # val_loss in their names, the resume file by the exact value it stores
            if ckpt_dir and os.path.isdir(ckpt_dir):
                here = os.path.abspath(str(resume_ckpt))
                for f in sorted(os.listdir(ckpt_dir)):
                    m = _CKPT_NAME.match(f)
                    p = os.path.join(ckpt_dir, f)
                    if not m or int(m.group(1)) > e:
                        continue
                    exact = os.path.abspath(p) == here and "val_loss" in ck
                    kept.append((float(ck["val_loss"]) if exact else float(m.group(2)), int(m.group(1)), p))
        history = []
        for epoch in range(start, int(max_epochs)):
            n = len(train_ds)
            perm = np.random.RandomState(int(shuffle_seed) * 1000003 + epoch).permutation(n)
            losses = [self.training_step(train_ds.get_batch(perm[lo:lo + batch_size]), b)["loss"]
                      for b, lo in enumerate(range(0, n, batch_size))]
            if not losses:
                raise ValueError("fit: the training set is empty")
            train_loss = float(torch.stack(losses).mean())
            val_loss = train_loss
            metrics = {}
            if val_ds is not None and len(val_ds):
                val = self.validate(val_ds, batch_size)
                val_loss = float(val["val_loss"])
                metrics = {f"val/{k}": float(val["log"][f"val/{k}"]) for k in VAL_METRICS if f"val/{k}" in val["log"]}
            path = None
            if ckpt_dir and save_top_k != 0:
                path = self.save_checkpoint(os.path.join(ckpt_dir, f"checkpoint_epoch={epoch}-val_loss={val_loss:.2f}.ckpt"),
                                            epoch, val_loss=val_loss)
                kept.append((val_loss, epoch, path))
                if save_top_k > 0 and len(kept) > save_top_k:
                    kept.sort(key=lambda r: (r[0], r[1]))
                    for _, _, p in kept[save_top_k:]:
                        if os.path.exists(p):
                            os.remove(p)
                        if p == path:
                            path = None
                    kept = kept[:save_top_k]
            train_ds.on_epoch_end(epoch)
            history.append({"epoch": epoch, "train/pose_mse": train_loss, "val_loss": val_loss, "ckpt": path, **metrics})
        return history


def calc_mean_losses(outputs, loss_keys):
    """pose_trainer.py:27-39: per key, the mean over the outputs that have it; keys no
    output has are left out."""
    sums = {k: 0.0 for k in loss_keys}
    cnts = {k: 0 for k in loss_keys}
    for out in outputs:
        for k in loss_keys:
            if k in out:
                sums[k] = sums[k] + out[k]
                cnts[k] += 1
    return {k: sums[k] / cnts[k] for k in loss_keys if cnts[k] > 0}


# ---------------------------------------------------------------------- CLI
def _load_amass_path_list(csv_file):
    """pose_trainer.py:20-24: one sequence path per line."""
    with open(csv_file, "r") as fh:
        return [Path(ll.strip()) for ll in fh.readlines() if ll.strip()]


def build_parser() -> argparse.ArgumentParser:
    """The reference's training arguments and defaults (pose_trainer.py:204-230)."""
    p = argparse.ArgumentParser(prog="python -m temporal_inverse_kinematics_amd.trainer")
    p.add_argument("--amass", type=str, default="/media/F/datasets/amass", help="amass dir")
    p.add_argument("--data_dir", type=str, default="/media/F/datasets/amass/ik_model", help="data dir")
    p.add_argument("--n_workers", type=int, default=8, help="accepted and ignored (batches are built on the device)")
    p.add_argument("--max_epoch", type=int, default=200, help="max epoch")
    p.add_argument("--smpl_mean", type=str, default="/media/F/thesis/motion_capture/data/smpl/smpl_mean_params.npz",
                   help="accepted and ignored, as in the reference")
    p.add_argument("--n_train", type=int, default=-1, help="use the first n training sequences (-1: all)")
    p.add_argument("--n_valid", type=int, default=-1, help="use the first n validation sequences (-1: all)")
    p.add_argument("--resume_ckpt", type=str, default="", help="checkpoint to continue from")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--win_size", default=9, type=int, help="window size in frames")
    p.add_argument("--bs", default=256, type=int, help="batch size in terms of predicted frames")
    p.add_argument("--kps_channel", default=3, type=int, help="keypoint channel")
    p.add_argument("--graph_layout", default="coco", type=str, choices=["coco", "openpose"], help="skeleton graph layout")
    p.add_argument("--max_hop", default=2, type=int, help="graph max hop")
    p.add_argument("--dilation", default=1, type=int, help="conv dilation")
    p.add_argument("--keypoint_format", default="coco", type=str, help="input model keypoint format")
    p.add_argument("--n_out_joints", default=22, type=int, help="number of output joints")
    p.add_argument("--n_out_channels", default=3, type=int, help="number of output channels")
    p.add_argument("--synthetic_smplx", action="store_true",
                   help="use the seeded synthetic SMPL-X constants instead of <amass>/smplx (tests, dry runs)")
    return p


def build_train_parser() -> argparse.ArgumentParser:
    """build_parser() plus this project's own training options, which the reference does not have."""
    p = build_parser()
    p.add_argument("--kp_weight", type=float, default=0.0,
                   help="weight of the keypoint term rel(FK(pred)) vs rel(keypoints) in the loss (0: pose MSE alone)")
    p.add_argument("--val_metrics", action="store_true",
                   help="validation also reports mpjpe, pa_mpjpe (metres) and mpjae (radians) of the predicted poses")
    return p


def run_train(argv=None) -> int:
    """pose_trainer.py:233-256: train.csv / valid.csv under --data_dir, SMPL-X models
    from <amass>/smplx, the shape DB <amass>/smplx_shapes.npz for the training set
    only, checkpoints (top 30) under <data_dir>/model_ckps/."""
    from .smplx_fk import load_smplx_models
    from .training_data import AmassDataset
    hp = build_train_parser().parse_args(argv)
    kp_weight = hp.kp_weight
    val_metrics = hp.val_metrics
    del hp.kp_weight, hp.val_metrics    # not hyper-parameters of the model: the checkpoint's hparams keep their keys
    data_dir = Path(hp.data_dir)
    train_paths = _load_amass_path_list(data_dir / "train.csv")
    val_paths = _load_amass_path_list(data_dir / "valid.csv")
    if hp.n_train > 0:
        train_paths = train_paths[:hp.n_train]
    if hp.n_valid > 0:
        val_paths = val_paths[:hp.n_valid]
    shape_path = Path(hp.amass) / "smplx_shapes.npz"
    if not shape_path.exists():
        raise FileNotFoundError(f"smplx_shapes.npz is not found under {hp.amass}")
    kp_on = check_kp_args(kp_weight, 0 if kp_weight == 0 else 3) > 0.0 or val_metrics   # either needs FK in the trainer
    smplx = load_smplx_models(None if hp.synthetic_smplx else Path(hp.amass) / "smplx", "cuda", batch_size=1024)
    train_ds = AmassDataset(smplx_models=smplx, amass_paths=train_paths, window_size=hp.win_size,
                            keypoint_format=hp.keypoint_format, shape_db_path=shape_path, target_keypoints=kp_on)
    val_ds = AmassDataset(smplx_models=smplx, amass_paths=val_paths, window_size=hp.win_size,
                          keypoint_format=hp.keypoint_format, target_keypoints=kp_on)
    tr = GpuTrainer(IKPoseTrainer(hp), **({"smplx_models": smplx, "kp_weight": kp_weight, "val_metrics": val_metrics}
                                          if kp_on else {}))
    if hp.resume_ckpt:
        print(f"resume from checkpoint: {hp.resume_ckpt}")
    else:
        print("start new training with new model weights")
    history = tr.fit(train_ds, val_ds, max_epochs=hp.max_epoch, batch_size=hp.bs, ckpt_dir=data_dir / "model_ckps",
                     save_top_k=30, resume_ckpt=hp.resume_ckpt or None)
    for row in history:
        print(json.dumps(row))
    return 0


if __name__ == "__main__":
    sys.exit(run_train())
