"""Host test of the SMPL-X FK comparator (tests/fkref.py) and of the oracle's dtype
argument, on the oracle's own arrays: the per-group bar of
tests/test_gpu_fk_oracle.py passes what is right and fails what is subtly wrong.

1. oracle/smplx_lbs.py at its default dtype is bit for bit what it was before it
   took one (the earlier code is kept below, verbatim); in float32 every array it
   makes is float32; contour_bins is the bin logic tests/test_gpu_fk_joints.py
   restated.
2. The constants sets land in their skinning classes (at most 4, 8, 16 and more
   than 16 live joints per vertex); yaw_sweep hits all 79 bins, both clamps
   included, float32 and float64 bins agree and no body is nearer than 0.2499
   degrees to a bin edge; every input set of the GPU test meets the bin condition.
3. A second float32 evaluation in another order (fkref.evaluate(reorder=True):
   the blend as one product accumulated over K in steps of 32 from the last step
   to the first, the skinning a per-vertex sum over ascending live joints, the
   translation added before the landmarks and corrected by t (1 - sum of the
   barycentric weights)) passes every case of the GPU test at V = 777.
4. Every fault, injected in numpy into the float64 evaluation, fails its named case
   with a ratio of at least 2 MARGIN; whether the fixed bar TOL = 1e-4 of
   tests/test_gpu_fk.py would have passed it is asserted beside it.

Measured at V = 777 (error over the float32 oracle's noise, the unit of MARGIN = 4;
the worst of the three groups):
3. at most 1.82 (nz17, B = 37, joints 55..143).
4. fault: ratio on its named case, and its verdict under TOL on the same case
   P at two bf16 planes            16.96  std random B=37         passes TOL (5.5e-6)
   p0(feat).q2(P) dropped          16.96  std random B=37         passes TOL (5.5e-6)
   all i + j = 2 products dropped  16.87  std random B=37         passes TOL (5.4e-6)
   p1.q1 dropped                   19.94  blend_heavy random B=37 passes TOL (8.9e-6)
   p2.q0 dropped                   12.12  blend_heavy random B=37 passes TOL (4.8e-6)
   bin 39 - y written 40 - y       3.7e6  std yaw_sweep           fails TOL
   clamp at 39 removed             3.3e6  std yaw_sweep           fails TOL
   clamp below -39 removed         3.6e6  std yaw_sweep           fails TOL
   pose_mean omitted               1.7e6  std yaw_sweep           fails TOL
   1e-8 omitted                    inf    std angles (NaN)        fails TOL
   landmark translation without its (1 - sb) correction
                                   2.5e6  bary_open far           fails TOL (46 m); on std far
                                          it measures 0.29 and passes both bars: with normalised
                                          tables the term is dead code
   landmark translation added whole on top of the translated vertices
                                   1.1e7  bary_open far           fails TOL
   last live weight dropped        4.6e5  nz16 random B=37        fails TOL
   one joint's rotation transposed 3.9e6  std random B=37         fails TOL
   bone offset from the grandparent 5.7e5 std random B=37         fails TOL
   Measured only (below 2 MARGIN, not asserted to fail): p1.q1 dropped 2.45 (std),
   2.51 (bary_open), 2.85 (nz8), 3.19 (nz16), 2.93 (nz17); p2.q0 dropped 1.76 (std),
   1.81 (bary_open), 2.03 (nz8), 1.79 (nz16), 1.77 (nz17), all on random B=37.
   Both reach 2 MARGIN on blend_heavy only, where they are asserted.
"""
import numpy as np
import pytest

import fkref as fr
import memedge as me
from oracle import smplx_lbs as sl

# the cases of tests/test_gpu_fk_oracle.py at V = 777
BATCHES = (1, 3, 4, 5, 9, 127, 128, 129)
JOINT_BATCHES = (1, 63, 64, 65, 193)
CASES = ([(cn, "random", B) for cn in ("std", "blend_heavy") for B in sorted(set(BATCHES + JOINT_BATCHES))] +
         [(cn, k, None) for cn in ("std", "blend_heavy") for k in ("yaw_sweep", "angles")] +
         [("std", "far", None), ("std", "bare", None), ("bary_open", "far", None)] +
         [(cn, "random", B) for cn in ("nz8", "nz16", "nz17") for B in (5, 37)])
IDS = ["-".join(map(str, c)) for c in CASES]

# fault -> (constants, inputs, B, does the fixed bar TOL pass it on that case)
FAULT_CASES = {
    "P_two_planes": ("std", "random", 37, True),
    "drop_p0q2": ("std", "random", 37, True),
    "drop_i_plus_j_2": ("std", "random", 37, True),
    "drop_p1q1": ("blend_heavy", "random", 37, True),
    "drop_p2q0": ("blend_heavy", "random", 37, True),
    "bin_40_minus_y": ("std", "yaw_sweep", None, False),
    "no_clamp_39": ("std", "yaw_sweep", None, False),
    "no_clamp_below": ("std", "yaw_sweep", None, False),
    "no_pose_mean": ("std", "yaw_sweep", None, False),
    "no_eps": ("std", "angles", None, False),
    "lmk_no_transl_correction": ("bary_open", "far", None, False),
    "lmk_transl_added_whole": ("bary_open", "far", None, False),
    "drop_last_live": ("nz16", "random", 37, False),
    "transposed_joint": ("std", "random", 37, False),
    "wrong_parent": ("std", "random", 37, False),
}


# ---------------------------------------------------------------- 1. the oracle's dtype argument
def _rodrigues_before(rot_vecs):
    """oracle/smplx_lbs.py batch_rodrigues as it stood before the dtype argument."""
    v = np.asarray(rot_vecs, dtype=np.float64).reshape(-1, 3)
    angle = np.linalg.norm(v + 1e-8, axis=1, keepdims=True)
    d = v / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = np.zeros_like(rx)
    K = np.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).reshape(-1, 3, 3)
    return np.eye(3)[None] + s * K + (1 - c) * (K @ K)


def _forward_before(c, full_pose, betas=None, expression=None, transl=None):
    """oracle/smplx_lbs.py smplx_forward as it stood before the dtype argument -> (joints, verts, bins)."""
    pose = np.asarray(full_pose, dtype=np.float64).reshape(-1, 55, 3)
    B = pose.shape[0]
    if "pose_mean" in c:
        pose = pose + c["pose_mean"].astype(np.float64).reshape(1, 55, 3)
    nb = c["shapedirs"].shape[2]
    ne = c["exprdirs"].shape[2]
    beta = np.zeros((B, nb)) if betas is None else np.asarray(betas, np.float64)
    expr = np.zeros((B, ne)) if expression is None else np.asarray(expression, np.float64)
    shape_components = np.concatenate([beta, expr], 1)
    shapedirs = np.concatenate([c["shapedirs"], c["exprdirs"]], 2).astype(np.float64)
    v_shaped = c["v_template"].astype(np.float64)[None] + np.einsum("bl,mkl->bmk", shape_components, shapedirs)
    J = np.einsum("bik,ji->bjk", v_shaped, c["J_regressor"].astype(np.float64))
    R = _rodrigues_before(pose.reshape(-1, 3)).reshape(B, 55, 3, 3)
    pose_feature = (R[:, 1:] - np.eye(3)).reshape(B, -1)
    v_posed = v_shaped + (pose_feature @ c["posedirs"].astype(np.float64)).reshape(B, -1, 3)
    parents = c["parents"].astype(np.int64)
    rel = J.copy()
    rel[:, 1:] -= J[:, parents[1:]]
    T = np.zeros((B, 55, 4, 4))
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
    W = c["lbs_weights"].astype(np.float64)
    Tv = np.einsum("vj,bjkl->bvkl", W, A)
    verts = np.einsum("bvkl,bvl->bvk", Tv[:, :, :3, :3], v_posed) + Tv[:, :, :3, 3]
    faces = c["faces"].astype(np.int64)
    lf = np.broadcast_to(c["lmk_faces_idx"].astype(np.int64), (B, len(c["lmk_faces_idx"])))
    lb = np.broadcast_to(c["lmk_bary_coords"].astype(np.float64), (B,) + c["lmk_bary_coords"].shape)
    chain, i = [], 12
    while i != -1:
        chain.append(i)
        i = int(parents[i])
    rel_rot = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
    for j in chain:
        rel_rot = R[:, j] @ rel_rot
    sy = np.sqrt(rel_rot[:, 0, 0] ** 2 + rel_rot[:, 1, 0] ** 2)
    y = np.round(np.minimum(-np.arctan2(-rel_rot[:, 2, 0], sy) * 180.0 / np.pi, 39)).astype(np.int64)
    neg = (y < 0).astype(np.int64)
    mask = (y < -39).astype(np.int64)
    negv = mask * 78 + (1 - mask) * (39 - y)
    y = neg * negv + (1 - neg) * y
    lf = np.concatenate([lf, c["dynamic_lmk_faces_idx"].astype(np.int64)[y]], 1)
    lb = np.concatenate([lb, c["dynamic_lmk_bary_coords"].astype(np.float64)[y]], 1)
    tri = verts[np.arange(B)[:, None, None], faces[lf]]
    landmarks = np.einsum("blfi,blf->bli", tri, lb)
    extra = verts[:, c["extra_verts"].astype(np.int64)]
    joints = np.concatenate([posed_joints, extra, landmarks], 1)
    if transl is not None:
        t = np.asarray(transl, np.float64)[:, None, :]
        joints = joints + t
        verts = verts + t
    return joints, verts, y


@pytest.mark.parametrize("cname,kind", [("std", "random"), ("std", "angles"), ("std", "yaw_sweep"), ("bary_open", "far"),
                                        ("nz17", "bare")])
def test_default_dtype_is_bit_identical(cname, kind):
    c = fr.consts(cname)
    inp = fr.pose_for(c, kind, fr.inputs(kind, 9 if kind == "random" else None))
    jb, vb, bins = _forward_before(c, *inp)
    j, v = sl.smplx_forward(c, *inp)
    assert j.dtype == np.float64 and v.dtype == np.float64
    assert np.array_equal(j, jb) and np.array_equal(v, vb)
    assert np.array_equal(sl.smplx_forward(c, *inp, return_verts=False), jb)
    assert np.array_equal(sl.contour_bins(c, inp[0]), bins)          # the export is the forward's own bin
    assert np.array_equal(sl.contour_bins(c, inp[0], np.float64), bins)
    assert np.array_equal(sl.batch_rodrigues(inp[0]), _rodrigues_before(inp[0]))
    assert np.array_equal(sl.batch_rodrigues(inp[0], dtype=np.float64), _rodrigues_before(inp[0]))


def test_float32_is_float32_throughout():
    """A float64 constant, identity or zero tensor anywhere would promote the result."""
    c = fr.consts("std")
    inp = fr.inputs("random", 9)
    j, v = sl.smplx_forward(c, *inp, dtype=np.float32)
    assert j.dtype == np.float32 and v.dtype == np.float32
    assert sl.smplx_forward(c, inp[0], dtype=np.float32)[0].dtype == np.float32       # the defaulted inputs
    assert sl.batch_rodrigues(inp[0], dtype=np.float32).dtype == np.float32
    assert sl.contour_yaw_deg(c, inp[0], np.float32).dtype == np.float32
    assert sl.contour_yaw_deg(c, inp[0]).dtype == np.float64
    j64, v64 = sl.smplx_forward(c, *inp)
    for a, b in ((j, j64), (v, v64)):
        e = np.abs(a.astype(np.float64) - b).max()
        assert 1e-8 < e < 2e-6, e          # float32 noise on outputs of O(1): neither float64 nor worse


# ---------------------------------------------------------------- 2. constants and inputs
def test_constants_sets():
    for V in (fr.V_SMALL, fr.V_FULL):
        std = fr.consts("std", V)
        assert std["v_template"].shape == (V, 3)
        for name, (lo, hi) in fr.NZ_CLASS.items():
            c = fr.consts(name, V)
            n = fr.live_counts(c)
            assert lo <= n.max() <= hi and n.min() >= 1, (name, V, int(n.max()))
            if name != "std":
                assert n.max() == fr.NZ_MAX[name]
                assert (c["lbs_weights"] > 0).all() and (c["lbs_weights"] < fr.TAU).any()    # the sub-threshold tail
        with pytest.raises(ValueError):
            std["v_template"][0, 0] = 1.0                                                    # read-only
        bo = fr.consts("bary_open", V)
        for k in ("lmk_bary_coords", "dynamic_lmk_bary_coords"):
            s, s0 = bo[k].sum(-1), std[k].sum(-1)
            assert np.abs(s0 - 1).max() < 2e-7 and 0.69 < s.min() < 0.8 and 1.2 < s.max() < 1.31
            assert np.abs(s - 1).min() > 1e-4
    ref = fr.reference("blend_heavy", fr.V_SMALL, "random", 37)
    assert np.abs(ref["v64"]).max() < 10 and ref["unit"]["verts"] < 1e-6
    # the blend products, not the template, make the blend_heavy vertex
    c = fr.consts("blend_heavy")
    assert np.abs(c["v_template"]).max() < 0.02


def test_yaw_sweep_covers_every_bin():
    pose = fr.inputs("yaw_sweep")[0]
    assert pose.shape == (91, 55, 3)
    for cn, V in (("std", fr.V_SMALL), ("std", fr.V_FULL), ("blend_heavy", fr.V_SMALL)):
        b64, b32, dist = fr.bin_state(fr.consts(cn, V), pose)
        assert sorted(set(b64.tolist())) == list(range(79))
        assert np.array_equal(b64, b32)
        assert dist.min() >= 0.2499, dist.min()
        assert (b64 == 39).sum() >= 2 and (b64 == 78).sum() >= 2      # bodies past both clamps
    yaw = sl.contour_yaw_deg(fr.consts(), pose)
    assert yaw.max() > 44 and yaw.min() < -45


def test_every_input_set_meets_the_bin_condition():
    sets = [("random", B) for B in sorted(set(BATCHES + JOINT_BATCHES + (37,)))]
    sets += [(k, None) for k in ("yaw_sweep", "angles", "far", "bare")]
    for cn, V in (("std", fr.V_SMALL), ("std", fr.V_FULL), ("blend_heavy", fr.V_SMALL)):
        c = fr.consts(cn, V)
        for kind, B in sets:
            inp = fr.pose_for(c, kind, fr.inputs(kind, B))
            assert inp[0].dtype == np.float32 and inp[0].shape[1:] == (55, 3)
            b64, b32, dist = fr.bin_state(c, inp[0])
            assert np.array_equal(b64, b32) and dist.min() >= fr.BIN_EDGE_DEG, (cn, V, kind, B, dist.min())
    assert all(a is None for a in fr.inputs("bare")[1:])
    far = fr.inputs("far")
    assert np.abs(far[3]).max() > 100 and np.abs(far[1]).max() > 3


def test_a_body_on_a_bin_edge_is_replaced(monkeypatch):
    """The builder's replacement, driven by a threshold no draw of 64 bodies meets: with
    the edge distance raised to 0.05 degrees the offenders are redrawn and the rest stay."""
    raw = me.fk_inputs(64)
    monkeypatch.setattr(fr, "BIN_EDGE_DEG", 0.05)
    bad = fr.bin_offenders(fr.consts(), raw[0])
    assert bad.size > 0
    got = fr._random(64)
    assert fr.bin_offenders(fr.consts(), got[0]).size == 0
    keep = np.setdiff1d(np.arange(64), bad)
    for a, b in zip(got, raw):
        assert np.array_equal(a[keep], b[keep]) and not np.array_equal(a[bad], b[bad])
    again = fr._random(64)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))     # deterministic


def test_angles_are_what_they_say():
    c = fr.consts("std")
    pose = fr.pose_for(c, "angles", fr.inputs("angles"))[0]
    assert np.all(pose[0] + c["pose_mean"] == 0)                      # exactly zero after the pose mean
    n = np.linalg.norm(pose[:, :22].astype(np.float64), axis=2)
    assert np.allclose(n, np.array(fr.ANGLES)[:, None], rtol=1e-6, atol=1e-15)
    assert np.isfinite(fr.reference("std", fr.V_SMALL, "angles")["v64"]).all()


# ---------------------------------------------------------------- the comparator
def test_compare_groups_and_non_finite():
    ref = fr.reference("std", fr.V_SMALL, "random", 5)
    j, v = ref["j64"], ref["v64"]
    ok, r = fr.compare(j, v, ref)
    assert ok and r == {"verts": 0.0, "chain": 0.0, "rest": 0.0}
    ok, r = fr.compare(j, None, ref)                                  # the mesh-free joints path
    assert ok and sorted(r) == ["chain", "rest"]
    for g, sl_ in (("chain", (2, 54, 1)), ("rest", (2, 143, 1))):
        got = j.copy()
        got[sl_] += 5 * ref["unit"][g]
        ok, r = fr.compare(got, v, ref)
        assert not ok and 4.9 < r[g] < 5.1 and all(r[h] == 0 for h in r if h != g)
        got[sl_] = j[sl_] + 3 * ref["unit"][g]
        assert fr.compare(got, v, ref)[0]
    got = v.copy()
    got[4, 776, 2] += 5 * ref["unit"]["verts"]                        # the last vertex of the ragged tile
    ok, r = fr.compare(j, got, ref)
    assert not ok and 4.9 < r["verts"] < 5.1
    for bad in (np.nan, np.inf):
        got = v.copy()
        got[0, 0, 0] = bad
        ok, r = fr.compare(j, got, ref)
        assert not ok and r["verts"] == float("inf")
    for g in fr.GROUPS:   # the unit is float32 noise of an O(1) output, and never below one ulp of the largest value
        assert fr.EPS32 * np.abs(fr.split(j, v)[g]).max() <= ref["unit"][g] < 1e-6


def test_evaluate_is_the_oracle_in_float64():
    for cn, kind, B in (("std", "random", 9), ("bary_open", "far", None), ("nz17", "random", 5), ("std", "bare", None)):
        ref = fr.reference(cn, fr.V_SMALL, kind, B)
        j, v = fr.evaluate(fr.consts(cn), ref["inputs"])
        assert np.array_equal(j, ref["j64"]) and np.array_equal(v, ref["v64"])
        j, v = fr.evaluate(fr.consts(cn), ref["inputs"], reorder=True)
        # the dropped tail weights (up to 54 of 1e-13 per vertex) are the largest difference
        bound = 1e-10 * max(1.0, np.abs(ref["v64"]).max())
        assert np.abs(j - ref["j64"]).max() < bound and np.abs(v - ref["v64"]).max() < bound


# ---------------------------------------------------------------- 3. a legitimate reordering passes
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reordered_float32_passes(case):
    cn, kind, B = case
    ref = fr.reference(cn, fr.V_SMALL, kind, B)
    j, v = fr.evaluate(fr.consts(cn), ref["inputs"], np.float32, reorder=True)
    assert j.dtype == np.float32 and v.dtype == np.float32
    ok, r = fr.compare(j, v, ref)
    print(f"FK-HOST reordered f32 {case}: {fr.fmt(r)}")
    assert ok, (case, r)
    assert fr.compare(j, None, ref)[0]


# ---------------------------------------------------------------- 4. faults fail
@pytest.mark.parametrize("fault", list(FAULT_CASES))
def test_fault_fails(fault):
    cn, kind, B, tol_passes = FAULT_CASES[fault]
    ref = fr.reference(cn, fr.V_SMALL, kind, B)
    j, v = fr.evaluate(fr.consts(cn), ref["inputs"], fault=fault)
    ok, r = fr.compare(j, v, ref)
    e = fr.max_abs_err(j, v, ref)
    print(f"FK-HOST fault {fault} on {cn}/{kind}/{B}: {fr.fmt(r)}; max abs err {e:.3g}, TOL {'passes' if e < fr.TOL else 'fails'}")
    assert not ok and max(r.values()) >= 2 * fr.MARGIN, (fault, r)
    assert (e < fr.TOL) == tol_passes, (fault, e)


def test_p0q2_fault_in_place_of_the_kernel_output_fails():
    """What the GPU test would see if a kernel returned the float64 oracle with p0(feat).q2(P)
    left out of the blend, and nothing else wrong, cast to the kernel's float32."""
    ref = fr.reference("std", fr.V_SMALL, "random", 37)
    j, v = fr.evaluate(fr.consts("std"), ref["inputs"], fault="drop_p0q2")
    ok, r = fr.compare(j.astype(np.float32), v.astype(np.float32), ref)
    assert not ok and r["verts"] >= 2 * fr.MARGIN and r["rest"] >= 2 * fr.MARGIN and r["chain"] <= 1.0, r
    assert fr.max_abs_err(j, v, ref) < fr.TOL / 10      # an order of magnitude inside the fixed bar
    ok, r = fr.compare(j.astype(np.float32), None, ref)             # and on the joints path's two groups
    assert not ok


def test_translation_correction_is_dead_code_on_normalised_tables():
    ref = fr.reference("std", fr.V_SMALL, "far")
    j, v = fr.evaluate(fr.consts("std"), ref["inputs"], fault="lmk_no_transl_correction")
    ok, r = fr.compare(j, v, ref)
    print(f"FK-HOST lmk_no_transl_correction on std/far: {fr.fmt(r)}")
    assert ok and fr.max_abs_err(j, v, ref) < fr.TOL


@pytest.mark.parametrize("cname", fr.CONSTS)
def test_single_middle_product_dropped(cname):
    """p1.q1 and p2.q0 dropped: measured on every constants set, asserted to fail where they
    reach 2 MARGIN (blend_heavy), listed in the docstring elsewhere."""
    kind, B = "random", 37
    ref = fr.reference(cname, fr.V_SMALL, kind, B)
    for fault in ("drop_p1q1", "drop_p2q0"):
        j, v = fr.evaluate(fr.consts(cname), ref["inputs"], fault=fault)
        ok, r = fr.compare(j, v, ref)
        print(f"FK-HOST {fault} on {cname}/{kind}: {fr.fmt(r)}")
        assert fr.max_abs_err(j, v, ref) < fr.TOL
        assert r["chain"] == 0.0                                      # the chain joints do not read the blend
        if cname == "blend_heavy":
            assert not ok and max(r.values()) >= 2 * fr.MARGIN, (fault, r)
        else:
            assert max(r.values()) < 2 * fr.MARGIN, (fault, r)        # measured only: below the asserted level
