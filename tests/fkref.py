"""Constants, inputs, references and the comparator of the SMPL-X FK oracle tests
(tests/test_gpu_fk_oracle.py on the GPU, tests/test_fk_oracle_host.py on the
host). Not a test module.

Everything here is numpy on the float64 oracle (oracle/smplx_lbs.py); nothing
imports the HIP library, so the host test of the comparator runs anywhere.

The bar of a case, per output group (vertices, chain joints 0..54, joints 55..143):

    unit = max(max|oracle_f32 - oracle_f64|, 2^-23 * max|oracle_f64|)
    max|got - oracle_f64|  <=  MARGIN * unit

on the case's own outputs, oracle_f32 being the same oracle with every operation
in float32. The bar is a property of the reference alone.

The contour bin is a rounding of the neck yaw, so a body whose yaw sits on a bin
edge has no single right answer. Every input set here meets the bin condition:
each body's float64 yaw is at least BIN_EDGE_DEG from an edge and its float32
and float64 bins agree. Random draws that miss it are replaced by the next
seed's draw of the same body; nothing is excluded.
"""
from __future__ import annotations

import functools

import numpy as np

import fwdblocks as fb
import memedge as me
from oracle import smplx_lbs as sl
from temporal_inverse_kinematics_amd import synthetic as syn

MARGIN = fb.MARGIN
EPS32 = fb.EPS32
TOL = 1e-4                  # the fixed bar of tests/test_gpu_fk.py, kept there; here only to document the gap
V_SMALL = 777               # three 256-vertex tiles, the last ragged; 3V = 2331 is no multiple of 128
V_FULL = 10475
TAU = 2.0 ** -30            # fk_fold.h: joints with W > TAU are live
BIN_EDGE_DEG = 1e-3
GROUPS = ("verts", "chain", "rest")

CONSTS = ("std", "blend_heavy", "bary_open", "nz8", "nz16", "nz17")
NZ_MAX = {"nz8": 7, "nz16": 12, "nz17": 17}             # live joints per vertex, at most
NZ_CLASS = {"std": (1, 4), "nz8": (5, 8), "nz16": (9, 16), "nz17": (17, 55)}   # where the maximum must land

YAW_K = np.arange(-45, 46)                               # yaw_sweep: joint 12 about y by (k + 0.25) degrees
ANGLES = (0.0, 1e-8, 1e-4, 1e-3, np.pi - 1e-3, np.pi, 2 * np.pi - 1e-3, 2 * np.pi + 0.1, 7.0)
ANGLE_DIR = np.array([1.0, 2.0, 2.0]) / 3.0
NECK_CHAIN = (0, 3, 6, 9, 12)
DEFAULT_B = {"yaw_sweep": len(YAW_K), "angles": len(ANGLES), "far": 9, "bare": 5}

KSTEP = 32                  # reorder: the blend's K in steps of 32 (a GEMM tile's K step), the last step first
TRANSPOSED_JOINT = 16      # fault: this joint's rotation transposed
WRONG_PARENT_JOINT = 7      # fault: this joint's bone offset taken from its grandparent


# ---------------------------------------------------------------- constants
def live_counts(c):
    return (c["lbs_weights"] > np.float32(TAU)).sum(axis=1)


def _nz_weights(V, nzmax):
    """The construction of tests/test_gpu_fk.py::test_fk_sparse_skinning: 1..nzmax live
    joints per vertex and a tail of 1e-13 below the threshold."""
    rng = np.random.default_rng(nzmax)
    w = np.zeros((V, 55))
    for v in range(V):
        k = rng.integers(1, nzmax + 1)
        w[v, rng.choice(55, size=k, replace=False)] = rng.uniform(0.05, 1.0, k)
    w /= w.sum(axis=1, keepdims=True)
    w[w == 0] = 1e-13
    return w.astype(np.float32)


@functools.lru_cache(maxsize=None)
def consts(name="std", V=V_SMALL):
    """A dict edit of synthetic_smplx_constants(seed=1, num_verts=V); read-only."""
    c = dict(syn.synthetic_smplx_constants(seed=1, num_verts=V))
    if name == "blend_heavy":   # the blend GEMM's products dominate the vertex, not the template row
        c["v_template"] = c["v_template"] * np.float32(0.01)
        c["posedirs"] = c["posedirs"] * np.float32(30)
        c["shapedirs"] = c["shapedirs"] * np.float32(10)
    elif name == "bary_open":   # barycentric triples that do not sum to 1
        rng = np.random.default_rng(777)
        for k in ("lmk_bary_coords", "dynamic_lmk_bary_coords"):
            f = rng.uniform(0.7, 1.3, c[k].shape[:-1] + (1,))
            c[k] = (c[k] * f).astype(np.float32)
    elif name in NZ_MAX:
        c["lbs_weights"] = _nz_weights(V, NZ_MAX[name])
    elif name != "std":
        raise ValueError(name)
    if name in NZ_CLASS:
        lo, hi = NZ_CLASS[name]
        assert lo <= int(live_counts(c).max()) <= hi, (name, int(live_counts(c).max()))
    for v in c.values():
        v.setflags(write=False)
    return c


# ---------------------------------------------------------------- the bin condition
BIN_EDGES = np.arange(-39, 39) + 0.5    # -38.5 .. 38.5: beyond them every yaw lands in bin 78 or 39


def bin_state(c, pose):
    """-> (float64 bins, float32 bins, degrees from each body's float64 yaw to the nearest bin edge)."""
    y64 = sl.contour_yaw_deg(c, pose, np.float64)
    return (sl.contour_bins(c, pose, np.float64), sl.contour_bins(c, pose, np.float32),
            np.abs(y64[:, None] - BIN_EDGES[None]).min(axis=1))


def bin_offenders(c, pose):
    b64, b32, dist = bin_state(c, pose)
    return np.nonzero((b64 != b32) | (dist < BIN_EDGE_DEG))[0]


def assert_bin_condition(c, pose):
    bad = bin_offenders(c, pose)
    assert bad.size == 0, ("bodies on a contour bin edge", bad.tolist())


# ---------------------------------------------------------------- inputs
def _random(B, transl_sigma=None, beta_scale=None):
    """memedge.fk_inputs(B); a body that misses the bin condition is replaced, in all
    four arrays, by the same body of the next seed's draw."""
    c = consts("std", V_SMALL)
    seed = 10 + B
    arrs = [np.array(a, copy=True) for a in me.fk_inputs(B, seed)]
    for _ in range(16):
        bad = bin_offenders(c, arrs[0])
        if bad.size == 0:
            break
        seed += 1
        for a, n in zip(arrs, me.fk_inputs(B, seed)):
            a[bad] = n[bad]
    pose, betas, expr, transl = arrs
    if transl_sigma is not None:
        transl = np.random.default_rng(4000 + B).normal(0.0, transl_sigma, (B, 3)).astype(np.float32)
    if beta_scale is not None:
        betas = betas * np.float32(beta_scale)
    return pose, betas, expr, transl


@functools.lru_cache(maxsize=None)
def inputs(kind, B=None):
    """(pose (B,55,3), betas, expression, transl), float32 and read-only; 'bare': the last three None."""
    B = DEFAULT_B.get(kind) if B is None else B
    if kind == "random":
        out = _random(B)
    elif kind == "far":           # metres of translation, as AMASS trans has, and strong shapes
        out = _random(B, transl_sigma=100.0, beta_scale=3.0)
    elif kind == "bare":
        out = (_random(B)[0], None, None, None)
    elif kind == "yaw_sweep":     # every contour bin, both clamps: the neck chain is joint 12 alone
        assert B == len(YAW_K)
        pose, betas, expr, transl = [np.array(a, copy=True) for a in me.fk_inputs(B)]
        pose[:, NECK_CHAIN[:-1]] = 0.0
        pose[:, 12] = 0.0
        pose[:, 12, 1] = np.deg2rad(YAW_K + 0.25).astype(np.float32)
        out = (pose, betas, expr, transl)
    elif kind == "angles":        # one body per rotation magnitude, joints 0..21 along (1,2,2)/3
        assert B == len(ANGLES)
        pose, betas, expr, transl = [np.array(a, copy=True) for a in me.fk_inputs(B)]
        for b, m in enumerate(ANGLES):
            pose[b, :22] = (m * ANGLE_DIR).astype(np.float32)
        # exactly zero on every joint, the hands included: the pose that cancels the pose mean
        pose[0] = -consts("std", V_SMALL)["pose_mean"]
        out = (pose, betas, expr, transl)
    else:
        raise ValueError(kind)
    for a in out:
        if a is not None:
            assert a.dtype == np.float32
            a.setflags(write=False)
    assert_bin_condition(consts("std", V_SMALL), out[0])
    return out


def pose_for(c, kind, inp):
    """'angles' cancels the pose mean of the constants it runs on (body 0 exactly zero)."""
    if kind != "angles":
        return inp
    pose = np.array(inp[0], copy=True)
    pose[0] = -c["pose_mean"]
    return (pose,) + tuple(inp[1:])


# ---------------------------------------------------------------- reference and comparator
@functools.lru_cache(maxsize=None)
def reference(cname, V, kind, B=None):
    """The float64 oracle and its float32 restatement on one case, computed once, read-only:
    {'inputs', 'j64', 'v64', 'unit': {group: float}}."""
    c = consts(cname, V)
    inp = pose_for(c, kind, inputs(kind, B))
    assert_bin_condition(c, inp[0])
    j64, v64 = sl.smplx_forward(c, *inp)
    j32, v32 = sl.smplx_forward(c, *inp, dtype=np.float32)
    assert j32.dtype == np.float32 and v32.dtype == np.float32
    g64, g32 = split(j64, v64), split(j32, v32)
    unit = {g: max(float(np.abs(g32[g].astype(np.float64) - g64[g]).max()), EPS32 * float(np.abs(g64[g]).max()))
            for g in GROUPS}
    for a in (j64, v64):
        a.setflags(write=False)
    return {"inputs": inp, "j64": j64, "v64": v64, "unit": unit}


def split(joints, verts):
    return {"verts": verts, "chain": joints[:, :55], "rest": joints[:, 55:]}


def compare(joints, verts, ref, margin=MARGIN):
    """-> (ok, {group: max|got - f64| / unit}). verts None (the mesh-free joints path):
    its group is left out. A non-finite value fails with an infinite ratio."""
    got = split(np.asarray(joints, np.float64), None if verts is None else np.asarray(verts, np.float64))
    want = split(ref["j64"], ref["v64"])
    ratios = {}
    for g in GROUPS:
        if got[g] is None:
            continue
        assert got[g].shape == want[g].shape, (g, got[g].shape, want[g].shape)
        d = np.abs(got[g] - want[g])
        ratios[g] = float(d.max() / ref["unit"][g]) if np.isfinite(got[g]).all() else float("inf")
    return all(r <= margin for r in ratios.values()), ratios


def max_abs_err(joints, verts, ref):
    """What the fixed bar TOL looks at."""
    with np.errstate(invalid="ignore"):
        e = max(float(np.abs(np.asarray(joints, np.float64) - ref["j64"]).max()),
                float(np.abs(np.asarray(verts, np.float64) - ref["v64"]).max()))
    return e if np.isfinite(e) else float("inf")


def fmt(ratios):
    return " ".join(f"{g}={r:.2f}" for g, r in ratios.items())


# ---------------------------------------------------------------- a second evaluation, with fault hooks
FAULTS = ("P_two_planes", "drop_p0q2", "drop_i_plus_j_2", "drop_p1q1", "drop_p2q0", "bin_40_minus_y", "no_clamp_39",
          "no_clamp_below", "no_pose_mean", "no_eps", "lmk_no_transl_correction", "lmk_transl_added_whole",
          "drop_last_live", "transposed_joint", "wrong_parent")


def planes(a):
    """The three bf16 planes of a float32 array, as the bf16x3 kernels split their operands."""
    a = np.asarray(a, np.float32)
    acc = [np.zeros_like(a)] + [fb.round_planes(a, k) for k in (1, 2, 3)]
    return [(acc[k + 1] - acc[k]).astype(np.float64) for k in range(3)]


def _rodrigues(v, dt, eps=True):
    v = np.asarray(v, dt).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        angle = np.linalg.norm(v + dt(1e-8) if eps else v, axis=1, keepdims=True)
        d = v / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).reshape(-1, 3, 3)
    return np.eye(3, dtype=dt)[None] + s * K + (dt(1) - c) * (K @ K)


def _faulty_bins(yaw, fault):
    hi = yaw if fault == "no_clamp_39" else np.minimum(yaw, yaw.dtype.type(39))
    y = np.round(hi).astype(np.int64)
    below = np.zeros_like(y, dtype=bool) if fault == "no_clamp_below" else y < -39
    negv = np.where(below, 78, (40 if fault == "bin_40_minus_y" else 39) - y)
    # a kernel would read past the 79-row table here; numpy wraps so that the fault stays a wrong row
    return np.where(y < 0, negv, y) % 79


def evaluate(c, inp, dtype=np.float64, fault=None, reorder=False):
    """SMPL-X FK restated a second time, every operation in dtype -> (joints, verts).

    reorder=False: the oracle's formulation (template + shape + pose blend, dense skinning,
    landmarks before the translation). reorder=True: what a kernel may legitimately do
    instead: one blend product [vec(R - I) | betas | expression | 1] . P accumulated over K
    in reversed order, the skinning a per-vertex sum over the live joints (W > 2^-30) in
    ascending order, the translation added to the vertices before the landmarks and
    corrected by t (1 - sum of the barycentric weights).
    fault: one of FAULTS, what a subtly wrong kernel would compute."""
    assert fault is None or fault in FAULTS, fault
    dt = np.dtype(dtype).type
    pose, betas, expr, transl = inp
    p = np.asarray(pose, dt).reshape(-1, 55, 3)
    B, V = p.shape[0], c["v_template"].shape[0]
    if fault != "no_pose_mean":
        p = p + c["pose_mean"].astype(dt)[None]
    R = _rodrigues(p.reshape(-1, 3), dt, eps=fault != "no_eps").reshape(B, 55, 3, 3)
    if fault == "transposed_joint":
        R = R.copy()
        R[:, TRANSPOSED_JOINT] = R[:, TRANSPOSED_JOINT].transpose(0, 2, 1)
    nb, ne = c["shapedirs"].shape[2], c["exprdirs"].shape[2]
    beta = np.zeros((B, nb), dt) if betas is None else np.asarray(betas, dt)
    ex = np.zeros((B, ne), dt) if expr is None else np.asarray(expr, dt)
    shape = np.concatenate([beta, ex], 1)
    sdirs = np.concatenate([c["shapedirs"], c["exprdirs"]], 2).astype(dt)
    v_shaped = c["v_template"].astype(dt)[None] + np.einsum("bl,mkl->bmk", shape, sdirs)
    J = np.einsum("bik,ji->bjk", v_shaped, c["J_regressor"].astype(dt))
    # ---- the blend
    feat = np.concatenate([(R[:, 1:] - np.eye(3, dtype=dt)).reshape(B, -1), shape, np.ones((B, 1), dt)], 1)
    P = np.concatenate([c["posedirs"].astype(dt), sdirs.reshape(3 * V, nb + ne).T, c["v_template"].astype(dt).reshape(1, -1)], 0)
    blend_fault = fault in ("P_two_planes", "drop_p0q2", "drop_i_plus_j_2", "drop_p1q1", "drop_p2q0")
    if blend_fault:
        assert dt is np.float64
        f32, P32 = feat.astype(np.float32), P.astype(np.float32)
        if fault == "P_two_planes":
            vp = f32.astype(np.float64) @ fb.round_planes(P32, 2).astype(np.float64)
        else:
            pf, qP = planes(f32), planes(P32)
            drop = {"drop_p0q2": [(0, 2)], "drop_p1q1": [(1, 1)], "drop_p2q0": [(2, 0)],
                    "drop_i_plus_j_2": [(0, 2), (1, 1), (2, 0)]}[fault]
            vp = f32.astype(np.float64) @ P32.astype(np.float64) - sum(pf[i] @ qP[j] for i, j in drop)
    elif reorder:
        vp = np.zeros((B, 3 * V), dt)
        for k in range((P.shape[0] - 1) // KSTEP * KSTEP, -1, -KSTEP):   # the last K step first
            vp += feat[:, k:k + KSTEP] @ P[k:k + KSTEP]
    else:
        vp = v_shaped.reshape(B, -1) + feat[:, :486] @ P[:486]
    v_posed = vp.reshape(B, V, 3)
    # ---- the chain
    parents = c["parents"].astype(np.int64)
    src = parents.copy()
    if fault == "wrong_parent":
        src[WRONG_PARENT_JOINT] = parents[parents[WRONG_PARENT_JOINT]]
    rel = J.copy()
    rel[:, 1:] -= J[:, src[1:]]
    T = np.zeros((B, 55, 4, 4), dt)
    T[:, :, :3, :3] = R
    T[:, :, :3, 3] = rel
    T[:, :, 3, 3] = 1.0
    G = np.zeros_like(T)
    G[:, 0] = T[:, 0]
    for i in range(1, 55):
        G[:, i] = G[:, parents[i]] @ T[:, i]
    A = G.copy()
    A[:, :, :3, 3] -= np.einsum("bjkl,bjl->bjk", G[:, :, :3, :3], J)
    # ---- the skinning
    W = c["lbs_weights"].astype(dt)
    if fault == "drop_last_live":   # the full vertices lose their last live joint (a loop one short)
        W = W.copy()
        live = c["lbs_weights"] > np.float32(TAU)
        n = live.sum(1)
        last = 54 - np.argmax(live[:, ::-1], axis=1)
        full = n == n.max()
        W[np.nonzero(full)[0], last[full]] = 0
    if reorder:
        live = c["lbs_weights"] > np.float32(TAU)
        Tv = np.zeros((B, V, 3, 4), dt)
        for j in range(55):
            Tv += np.where(live[:, j], W[:, j], dt(0))[None, :, None, None] * A[:, j, None, :3, :]
    else:
        Tv = np.einsum("vj,bjkl->bvkl", W, A)[:, :, :3, :]
    if reorder:
        verts = Tv[..., 0] * v_posed[..., 0:1] + Tv[..., 1] * v_posed[..., 1:2] + Tv[..., 2] * v_posed[..., 2:3] + Tv[..., 3]
    else:
        verts = np.einsum("bvkl,bvl->bvk", Tv[..., :3], v_posed) + Tv[..., 3]
    # ---- the landmarks
    t = np.zeros((B, 1, 3), dt) if transl is None else np.asarray(transl, dt)[:, None, :]
    faces = c["faces"].astype(np.int64)
    if fault in ("bin_40_minus_y", "no_clamp_39", "no_clamp_below"):
        bins = _faulty_bins(sl.contour_yaw_deg(c, pose, dt), fault)
    else:
        bins = sl.contour_bins(c, pose, dt)
    lf = np.concatenate([np.broadcast_to(c["lmk_faces_idx"].astype(np.int64), (B, len(c["lmk_faces_idx"]))),
                         c["dynamic_lmk_faces_idx"].astype(np.int64)[bins]], 1)
    lb = np.concatenate([np.broadcast_to(c["lmk_bary_coords"].astype(dt), (B,) + c["lmk_bary_coords"].shape),
                         c["dynamic_lmk_bary_coords"].astype(dt)[bins]], 1)
    translated_first = reorder or fault in ("lmk_no_transl_correction", "lmk_transl_added_whole")
    if translated_first:
        verts = verts + t
        tri = verts[np.arange(B)[:, None, None], faces[lf]]
        s = tri[:, :, 0] * lb[:, :, 0:1]
        for i in (1, 2):
            s = s + tri[:, :, i] * lb[:, :, i:i + 1]
        if fault == "lmk_no_transl_correction":
            lmk = s
        elif fault == "lmk_transl_added_whole":
            lmk = s + t
        else:
            lmk = s + t * (dt(1) - (lb[:, :, 0:1] + lb[:, :, 1:2] + lb[:, :, 2:3]))
        joints = np.concatenate([G[:, :, :3, 3] + t, verts[:, c["extra_verts"].astype(np.int64)], lmk], 1)
    else:
        tri = verts[np.arange(B)[:, None, None], faces[lf]]
        lmk = np.einsum("blfi,blf->bli", tri, lb)
        joints = np.concatenate([G[:, :, :3, 3], verts[:, c["extra_verts"].astype(np.int64)], lmk], 1) + t
        verts = verts + t
    return joints, verts
