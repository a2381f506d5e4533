"""ORACLE — CPU restatement of SMPL-X forward kinematics + LBS. TEST INFRASTRUCTURE ONLY.

The reference calls the third-party `smplx` package (vchoutas/smplx) at
common/smpl_util.py:13-18 (smplx.create(model_type='smplx', use_pca=False,
use_face_contour=True, batch_size=...)) and :67-69 (SMPLX.forward). smplx is
not vendored in /root/reference, not installed here, and its version is not
pinned (README.md:14 names a requirements.txt that does not exist), so this
restates its published algorithm (smplx/lbs.py: lbs, blend_shapes,
vertices2joints, batch_rodrigues, batch_rigid_transform, vertices2landmarks,
find_dynamic_lmk_idx_and_bcoords, rot_mat_to_euler; smplx/body_models.py:
SMPLX.forward, VertexJointSelector) in numpy float64.

PARITY UNPINNED for everything past the rotation step: no reference test,
fixture or model file pins the kinematic chain, LBS or landmarks (SURVEY.md
§8c). The axis-angle -> rotation step is pinned: smplx's batch_rodrigues
agrees with the reference's kornia copy (golden kornia.npz) to ~1.5e-6.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

NECK_IDX = 12


def batch_rodrigues(rot_vecs, dtype=np.float64):
    """smplx lbs.batch_rodrigues: angle = ||v + 1e-8||, K skew of v/angle,
    R = I + sin K + (1 - cos) K^2. Every operation in `dtype`."""
    dt = np.dtype(dtype).type
    v = np.asarray(rot_vecs, dtype=dt).reshape(-1, 3)
    angle = np.linalg.norm(v + dt(1e-8), axis=1, keepdims=True)
    d = v / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).reshape(-1, 3, 3)
    return np.eye(3, dtype=dt)[None] + s * K + (dt(1) - c) * (K @ K)


def rot_mat_to_euler(R):
    sy = np.sqrt(R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2)
    return np.arctan2(-R[:, 2, 0], sy)


def neck_kin_chain(parents):
    chain, i = [], NECK_IDX
    while i != -1:
        chain.append(i)
        i = int(parents[i])
    return chain


def _posed(c, pose, dt):
    """(B,55,3) pose in dt with the constants' pose_mean added, as SMPLX.forward does first."""
    pose = np.asarray(pose, dtype=dt).reshape(-1, 55, 3)
    if "pose_mean" in c:
        pose = pose + c["pose_mean"].astype(dt).reshape(1, 55, 3)
    return pose


def _yaw_deg(c, R):
    """find_dynamic_lmk_idx_and_bcoords up to the angle: the neck chain's relative
    rotation, its y Euler angle, negated, in degrees. R (B,55,3,3)."""
    dt = R.dtype.type
    rel_rot = np.broadcast_to(np.eye(3, dtype=dt), (R.shape[0], 3, 3)).copy()
    for j in neck_kin_chain(c["parents"].astype(np.int64)):
        rel_rot = R[:, j] @ rel_rot
    return -rot_mat_to_euler(rel_rot) * dt(180.0) / dt(np.pi)


def _bins_of_yaw(yaw):
    """The rest of it: clamp at 39, round, negative angles to bins 40..78."""
    y = np.round(np.minimum(yaw, yaw.dtype.type(39))).astype(np.int64)
    neg = (y < 0).astype(np.int64)
    mask = (y < -39).astype(np.int64)
    negv = mask * 78 + (1 - mask) * (39 - y)
    return neg * negv + (1 - neg) * y


def contour_yaw_deg(c, pose, dtype=np.float64):
    """The yaw (degrees, before clamp and rounding) the contour bin of each body is
    taken from: pose (B,55,3) as smplx_forward takes it, every operation in dtype."""
    dt = np.dtype(dtype).type
    p = _posed(c, pose, dt)
    return _yaw_deg(c, batch_rodrigues(p.reshape(-1, 3), dt).reshape(-1, 55, 3, 3))


def contour_bins(c, pose, dtype=np.float64):
    """The dynamic-contour bin (0..78) of each body, by smplx_forward's own logic."""
    return _bins_of_yaw(contour_yaw_deg(c, pose, dtype))


def smplx_forward(c: Dict[str, np.ndarray], full_pose, betas=None, expression=None, transl=None,
                  return_verts=True, dtype=np.float64):
    """SMPLX.forward for pose2rot, use_pca=False, use_face_contour=True.

    c: constants (synthetic.synthetic_smplx_constants layout, plus optional
    'pose_mean' (55,3), 'dynamic_lmk_faces_idx' (79,17), 'dynamic_lmk_bary_coords' (79,17,3)).
    full_pose: (B,55,3) [global, 21 body, jaw, leye, reye, 15 lhand, 15 rhand].
    dtype: every operation, constant and intermediate in it (float64: the
    reference; float32: the measure of float32's own rounding noise).
    Returns joints (B, 55+21+51[+17], 3) and vertices (B,V,3).
    """
    dt = np.dtype(dtype).type
    pose = _posed(c, full_pose, dt)
    B = pose.shape[0]
    nb = c["shapedirs"].shape[2]
    ne = c["exprdirs"].shape[2]
    beta = np.zeros((B, nb), dt) if betas is None else np.asarray(betas, dt)
    expr = np.zeros((B, ne), dt) if expression is None else np.asarray(expression, dt)
    shape_components = np.concatenate([beta, expr], 1)
    shapedirs = np.concatenate([c["shapedirs"], c["exprdirs"]], 2).astype(dt)
    # lbs()
    v_shaped = c["v_template"].astype(dt)[None] + np.einsum("bl,mkl->bmk", shape_components, shapedirs)
    J = np.einsum("bik,ji->bjk", v_shaped, c["J_regressor"].astype(dt))
    R = batch_rodrigues(pose.reshape(-1, 3), dt).reshape(B, 55, 3, 3)
    pose_feature = (R[:, 1:] - np.eye(3, dtype=dt)).reshape(B, -1)
    v_posed = v_shaped + (pose_feature @ c["posedirs"].astype(dt)).reshape(B, -1, 3)
    parents = c["parents"].astype(np.int64)
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    T = np.zeros((B, 55, 4, 4), dt)
    T[:, :, :3, :3] = R
    T[:, :, :3, 3] = rel
    T[:, :, 3, 3] = 1.0
    G = np.zeros_like(T)
    G[:, 0] = T[:, 0]
    for i in range(1, 55):
        G[:, i] = G[:, parents[i]] @ T[:, i]
    posed_joints = G[:, :, :3, 3].copy()
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("bjkl,bjl->bjk", G[:, :, :3, :3], J)
    W = c["lbs_weights"].astype(dt)
    Tv = np.einsum("vj,bjkl->bvkl", W, A)
    verts = np.einsum("bvkl,bvl->bvk", Tv[:, :, :3, :3], v_posed) + Tv[:, :, :3, 3]
    # landmarks (vertices2landmarks)
    faces = c["faces"].astype(np.int64)
    lf = np.broadcast_to(c["lmk_faces_idx"].astype(np.int64), (B, len(c["lmk_faces_idx"])))
    lb = np.broadcast_to(c["lmk_bary_coords"].astype(dt), (B,) + c["lmk_bary_coords"].shape)
    if "dynamic_lmk_faces_idx" in c:
        y = _bins_of_yaw(_yaw_deg(c, R))
        lf = np.concatenate([lf, c["dynamic_lmk_faces_idx"].astype(np.int64)[y]], 1)
        lb = np.concatenate([lb, c["dynamic_lmk_bary_coords"].astype(dt)[y]], 1)
    tri = verts[np.arange(B)[:, None, None], faces[lf]]            # (B, L, 3 verts, 3)
    landmarks = np.einsum("blfi,blf->bli", tri, lb)
    extra = verts[:, c["extra_verts"].astype(np.int64)]
    joints = np.concatenate([posed_joints, extra, landmarks], 1)
    if transl is not None:
        t = np.asarray(transl, dt)[:, None, :]
        joints = joints + t
        verts = verts + t
    return (joints, verts) if return_verts else joints
