"""GPU parity of the SMPL-X FK check (tik_fk_*) against the numpy oracle
(oracle/smplx_lbs.py). Parity UNPINNED by the reference past the rotation
step (smplx is third-party and absent; no model files): the oracle restates
the public smplx algorithm. Tolerance 1e-4 abs on joints/vertices of O(1)."""
import numpy as np
import pytest

import torch

from oracle import smplx_lbs as sl

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def consts():
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    _build.build()
    return syn.synthetic_smplx_constants(seed=1)


@pytest.fixture(scope="module", params=["bf16x3", "fp32"])
def model(consts, request):
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    return SMPLX(consts, batch_size=9, precision=request.param)


def _inputs(B, seed):
    from temporal_inverse_kinematics_amd import synthetic as syn
    pose, betas = syn.synthetic_fk_inputs(B, seed=seed)
    rng = np.random.default_rng(seed)
    expr = rng.normal(0, 0.5, (B, 10)).astype(np.float32)
    transl = rng.normal(0, 0.5, (B, 3)).astype(np.float32)
    return pose, betas, expr, transl


@pytest.mark.parametrize("B", [1, 3, 8, 37])
def test_fk_vs_oracle(consts, model, B):
    pose, betas, expr, transl = _inputs(B, 10 + B)
    cu = lambda a: torch.from_numpy(a).cuda()
    j, v = model.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
    jr, vr = sl.smplx_forward(consts, pose, betas, expr, transl)
    assert j.shape == (B, 144, 3) and v.shape == (B, 10475, 3)
    assert np.abs(v.cpu().numpy() - vr).max() < TOL
    assert np.abs(j.cpu().numpy() - jr).max() < TOL


def test_fk_defaults_and_joints_only(consts, model):
    pose, _, _, _ = _inputs(5, 99)
    j, v = model.full_forward(torch.from_numpy(pose).cuda(), return_verts=False)
    assert v is None
    jr = sl.smplx_forward(consts, pose, return_verts=False)
    assert np.abs(j.cpu().numpy() - jr).max() < TOL


def test_fk_batch_independent_large(consts, model):
    pose, betas, expr, transl = _inputs(300, 5)
    cu = lambda a: torch.from_numpy(a).cuda()
    j, v = model.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
    j1, v1 = model.full_forward(cu(pose[123:124]), cu(betas[123:124]), cu(expr[123:124]), cu(transl[123:124]))
    assert torch.equal(v[123:124], v1) and torch.equal(j[123:124], j1)
    jr, vr = sl.smplx_forward(consts, pose[[0, 150, 299]], betas[[0, 150, 299]], expr[[0, 150, 299]],
                              transl[[0, 150, 299]])
    assert np.abs(v.cpu().numpy()[[0, 150, 299]] - vr).max() < TOL


def test_fk_rotation_step_pinned_to_kornia(model):
    """drive the HIP FK chain. Body i is the rest pose with
    only joint 18 (left elbow) rotated by the golden kornia axis-angle aa_i
    (kornia_geometry_conversion.py:125-201 fixture, incl. the small-angle
    Taylor branch). Its child joint 20 must move rigidly: J20 - J18 =
    R_kornia(aa_i) (J20 - J18)_rest, on the FK's own posed joints."""
    from conftest import golden
    k = golden("kornia.npz")
    aa, R = k["aa"].astype(np.float32), k["R"].astype(np.float64)
    B = aa.shape[0]
    pose = np.zeros((B + 1, 55, 3), np.float32)
    pose[1:, 18] = aa                                  # body 0: the rest pose
    j, _ = model.full_forward(torch.from_numpy(pose).cuda(), return_verts=False)
    j = j.double().cpu().numpy()
    rest = j[0, 20] - j[0, 18]
    bones = j[1:, 20] - j[1:, 18]
    want = R @ rest
    # smplx's Rodrigues (angle = |aa + 1e-8|) agrees with kornia's to ~1.5e-6
    assert np.abs(bones - want).max() < 2e-5 * max(1.0, np.abs(rest).max())
    # joints off the rotated chain do not move
    assert np.abs(j[1:, :18] - j[0:1, :18]).max() < 1e-6


def test_fk_config4_full_batch(consts, model):
    """BASELINE config #4 at its size (B=4096 bodies, verts (4096,10475,3)):
    rows 0, 2047, 4095 against the oracle; batch independence (a solo body
    equals its row, bit for bit); finite everywhere."""
    B = 4096
    pose, betas, expr, transl = _inputs(B, 44)
    cu = lambda a: torch.from_numpy(a).cuda()
    j, v = model.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
    assert j.shape == (B, 144, 3) and v.shape == (B, 10475, 3)
    assert torch.isfinite(v).all() and torch.isfinite(j).all()
    pick = [0, 2047, 4095]
    jr, vr = sl.smplx_forward(consts, pose[pick], betas[pick], expr[pick], transl[pick])
    assert np.abs(v[pick].cpu().numpy() - vr).max() < TOL
    assert np.abs(j[pick].cpu().numpy() - jr).max() < TOL
    for i in (2047, 4095):
        j1, v1 = model.full_forward(cu(pose[i:i + 1]), cu(betas[i:i + 1]), cu(expr[i:i + 1]), cu(transl[i:i + 1]))
        assert torch.equal(v[i:i + 1], v1) and torch.equal(j[i:i + 1], j1)


@pytest.mark.parametrize("nzmax", [4, 7, 12])
def test_fk_sparse_skinning(consts, monkeypatch, nzmax):
    """Skinning on the sparse weights (fk.hip, the default: per vertex the
    joints with W > 2^-30, fp32 FMAs in ascending joint order) against the
    dense skinning GEMM (TIK_FK_SKIN=dense) and the oracle, on weight
    matrices with up to nzmax live joints per vertex (the 4, 8 and 16-entry
    kernels) plus a tail of tiny nonzero weights below the threshold, at a
    batch that ends mid body tile; and batch independence."""
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    c = dict(consts)
    rng = np.random.default_rng(nzmax)
    V = c["v_template"].shape[0]
    w = np.zeros((V, 55))
    for v in range(V):
        k = rng.integers(1, nzmax + 1)
        idx = rng.choice(55, size=k, replace=False)
        w[v, idx] = rng.uniform(0.05, 1.0, k)
    w /= w.sum(axis=1, keepdims=True)
    w[w == 0] = 1e-13   # below the threshold: dropped by the sparse kernels
    c["lbs_weights"] = w.astype(np.float32)
    B = 37
    pose, betas, expr, transl = _inputs(B, 500 + nzmax)
    cu = lambda a: torch.from_numpy(a).cuda()
    outs = []
    for flag in ("sparse", "dense"):
        monkeypatch.setenv("TIK_FK_SKIN", flag)
        m = SMPLX(c, batch_size=9, precision="bf16x3")
        outs.append(m.full_forward(cu(pose), cu(betas), cu(expr), cu(transl)))
    (jf, vf), (jd, vd) = outs
    assert torch.isfinite(vf).all()
    assert float((vf - vd).abs().max()) < 1e-5
    assert float((jf - jd).abs().max()) < 1e-5
    _, vr = sl.smplx_forward(c, pose[[0, 36]], betas[[0, 36]], expr[[0, 36]], transl[[0, 36]])
    assert np.abs(vf[[0, 36]].cpu().numpy() - vr).max() < TOL
    monkeypatch.setenv("TIK_FK_SKIN", "sparse")
    m = SMPLX(c, batch_size=9, precision="bf16x3")
    _, v1 = m.full_forward(cu(pose[36:37]), cu(betas[36:37]), cu(expr[36:37]), cu(transl[36:37]))
    assert torch.equal(v1, vf[36:37])


@pytest.mark.parametrize("B", [1, 1025, 2500, 4096])
def test_fk_chunk_pipeline_batch_invariant(consts, B):
    """Batches of more than one 2048-body chunk (fk_model.h) run blend + skinning
    per chunk, the chunks alternating between two HIP streams (fk_forward.cpp):
    every body's vertices and joints are bit-identical to the same body solved
    alone (the chunking only partitions rows), at one body, half a chunk plus
    one (one chunk), a ragged second chunk and config #4's two full chunks; the
    sampled bodies include both sides of the chunk boundary (2047, 2048); the
    last body against the oracle. Three chunks, the third on the first chunk's
    buffer: tests/test_gpu_fk_oracle.py with TIK_FK_CHUNK=4."""
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    pose, betas, expr, transl = _inputs(B, 900 + B)
    cu = lambda a: torch.from_numpy(a).cuda()
    m = SMPLX(consts, batch_size=9, precision="bf16x3")
    j, v = m.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
    torch.cuda.synchronize()
    assert torch.isfinite(v).all()
    for i in sorted({0, min(1023, B - 1), min(1024, B - 1), min(2047, B - 1), min(2048, B - 1), B - 1}):
        j1, v1 = m.full_forward(cu(pose[i:i + 1]), cu(betas[i:i + 1]), cu(expr[i:i + 1]), cu(transl[i:i + 1]))
        assert torch.equal(v[i:i + 1], v1) and torch.equal(j[i:i + 1], j1), i
    _, vr = sl.smplx_forward(consts, pose[-1:], betas[-1:], expr[-1:], transl[-1:])
    assert np.abs(v[-1:].cpu().numpy() - vr).max() < TOL


def _write_smplx_npz(path, c, components=400):
    """The constants in the SMPL-X model-file layout (the keys and shapes of
    SMPLX_{MALE,FEMALE,NEUTRAL}.npz as smplx.body_models.SMPLX reads them):
    shapedirs (V,3,400) with the expression basis at 300:, or the
    20-component layout (V,3,20) with it at 10:20. The unused components are
    filled with a marker value, so a loader reading the wrong columns fails."""
    V = c["v_template"].shape[0]
    shapedirs = np.full((V, 3, components), 7.0, np.float32)
    e0 = 300 if components >= 400 else 10
    shapedirs[:, :, :10] = c["shapedirs"]
    shapedirs[:, :, e0:e0 + 10] = c["exprdirs"]
    kin = np.zeros((2, 55), np.uint32)
    kin[0] = c["parents"].astype(np.int64) % (1 << 32)
    kin[1] = np.arange(55)
    np.savez(path, v_template=c["v_template"], shapedirs=shapedirs,
             posedirs=c["posedirs"].T.reshape(V, 3, 486), J_regressor=c["J_regressor"],
             weights=c["lbs_weights"], kintree_table=kin, f=c["faces"].astype(np.uint32),
             hands_meanl=c["pose_mean"][25:40].reshape(45), hands_meanr=c["pose_mean"][40:55].reshape(45),
             lmk_faces_idx=c["lmk_faces_idx"], lmk_bary_coords=c["lmk_bary_coords"],
             dynamic_lmk_faces_idx=c["dynamic_lmk_faces_idx"],
             dynamic_lmk_bary_coords=c["dynamic_lmk_bary_coords"])


def test_smplx_model_file_loader(tmp_path):
    """SMPLX_{MALE,FEMALE,NEUTRAL}.npz in the model-file
    layout (shapedirs (V,3,400) with the expression basis at 300:, posedirs
    (V,3,486), kintree_table, weights, f, hands_mean{l,r}, landmark and
    dynamic-landmark tables) -> load_smplx_models(dir) (smpl_util.py:8-19) ->
    HIP FK against the oracle on the constants the files were written from."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.smplx_fk import load_smplx_models
    src = {}
    for gender, seed in (("male", 11), ("female", 12), ("neutral", 13)):
        src[gender] = syn.synthetic_smplx_constants(seed=seed)
        src[gender]["extra_verts"] = syn.SMPLX_EXTRA_VERTS.copy()   # the loader's fixed vertex picks
        _write_smplx_npz(tmp_path / f"SMPLX_{gender.upper()}.npz", src[gender])
    models = load_smplx_models(str(tmp_path), "cuda", 9)
    pose, betas, expr, transl = _inputs(6, 77)
    cu = lambda a: torch.from_numpy(a).cuda()
    for gender, m in models.items():
        j, v = m.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
        jr, vr = sl.smplx_forward(src[gender], pose, betas, expr, transl)
        assert np.abs(v.cpu().numpy() - vr).max() < TOL, gender
        assert np.abs(j.cpu().numpy() - jr).max() < TOL, gender


def test_run_smpl_inference_api(consts):
    from temporal_inverse_kinematics_amd.smplx_fk import load_smplx_models, run_smpl_inference
    models = load_smplx_models(None, "cuda", 9)
    rng = np.random.default_rng(0)
    F = 20
    poses = rng.normal(0, 0.3, (F, 156)).astype(np.float32)
    data = {"poses": poses, "gender": "male", "trans": rng.normal(0, 1, (F, 3)), "betas": rng.normal(0, 1, 16)}
    j, v = run_smpl_inference(data, models, "cuda", apply_trans=False, apply_shape=False, return_mesh=True)
    # meshes keep the reference's padding to whole batches of 9 (smpl_util.py:76-77): 27 for 20 frames
    assert j.shape == (F, 144, 3) and v.shape == (27, 10475, 3)
    full = np.zeros((27, 55, 3), np.float32)
    full[:F, 0] = poses[:, :3]
    full[:F, 1:22] = poses[:, 3:66].reshape(F, 21, 3)
    full[:F, 25:40] = poses[:, 66:111].reshape(F, 15, 3)
    full[:F, 40:55] = poses[:, 111:156].reshape(F, 15, 3)
    from temporal_inverse_kinematics_amd import synthetic as syn
    jr, vr = sl.smplx_forward(syn.synthetic_smplx_constants(seed=1), full)
    assert np.abs(j - jr[:F]).max() < TOL and np.abs(v - vr).max() < TOL
    full = full[:F]
    jt = run_smpl_inference(data, models, "cuda", apply_trans=True, apply_shape=True, apply_root_rot=False)
    full[:, 0] = 0
    b = np.tile(np.asarray(data["betas"], np.float32)[:10][None], (F, 1))
    jr2 = sl.smplx_forward(syn.synthetic_smplx_constants(seed=1), full, b, transl=data["trans"], return_verts=False)
    assert np.abs(jt - jr2).max() < TOL


def test_fk_out_buffers(consts, model):
    """full_forward(out=(joints, vertices)) writes the same values into the
    caller's buffers (the FK bench's serving-loop form) and returns them; wrong
    shapes are refused."""
    pose, betas, expr, transl = _inputs(6, 321)
    cu = lambda a: torch.from_numpy(a).cuda()
    j, v = model.full_forward(cu(pose), cu(betas), cu(expr), cu(transl))
    oj, ov = torch.full_like(j, 7.0), torch.full_like(v, 7.0)
    j2, v2 = model.full_forward(cu(pose), cu(betas), cu(expr), cu(transl), out=(oj, ov))
    assert j2.data_ptr() == oj.data_ptr() and v2.data_ptr() == ov.data_ptr()
    assert torch.equal(oj, j) and torch.equal(ov, v)
    with pytest.raises(ValueError):
        model.full_forward(cu(pose), out=(oj[:5], ov))
