"""tik_fk_refine_robust / SMPLX.refine_frames(robust_sigma=, skip_nonfinite=) (csrc/lm_refine.hip): the Geman-McClure
data term and non-finite keypoints as missing, against the float64 reference of tests/lm_robust_ref.py and bit for bit
against itself. The body is the 77-vertex one of tests/lm_refine_ref.py.

Bounds: cost column 0 within 1e-4 of the float64 formula on the oracle's residual (the bound
test_gpu_lm_refine.check_against_reference uses for cost[0]); the IRLS weights within 1e-5 relative of the formula in
float64 on the same launch's dbg_r (a handful of fp32 roundings on both sides; against the oracle's r its 1e-4 would
swamp the comparison near s = sigma^2); the outlier scenario's final cost within 1.5 x + 1e-8 of the reference (the
bound refine_poses carries) and its worst keypoint distance to the clean truth at most 1/4 of the GPU's own plain run
(the reference's ratio is <= 0.082: a margin of 3). Everything else is bit for bit.

Each case prints its own figures.
"""
import numpy as np
import pytest
import torch

import fk_jacobian_ref as R
import lm_refine_ref as L
import lm_robust_ref as RR
import memedge as me

pytestmark = pytest.mark.gpu
CHECKED = [0, 63, 64]


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def new_model(skin):
    me.lib()
    with me.env(TIK_FK_SKIN=skin):
        return R.SMPLX(L.consts(), batch_size=9)


@pytest.fixture(scope="module")
def model():
    return new_model("sparse")


@pytest.fixture(scope="module")
def inputs65():
    """tests/test_gpu_lm_refine.py's: theta (65,66), betas (65,10), keypoints N(0, 0.3^2) (65,17,3)."""
    pose, betas, _, _ = R.inputs65()
    th = np.ascontiguousarray(pose[:, :22].reshape(65, 66), dtype=np.float32)
    kps = np.random.default_rng(65).normal(0, 0.3, (65, 17, 3)).astype(np.float32)
    return th, np.ascontiguousarray(betas, dtype=np.float32), kps


def c_refine(model, robust, t, k, b, iters, tail=()):
    """The C entry points, called positionally as the existing tests call tik_fk_refine -> (rc, poses, cost)."""
    from temporal_inverse_kinematics_amd import _lib
    lib = _lib.load()
    B = t.shape[0]
    out, cost = torch.full((B, 66), -7.0, device="cuda"), torch.full((B, iters + 1), -7.0, device="cuda")
    head = (model._h, t.data_ptr(), 0, 0, k.data_ptr(), b.data_ptr(), b.shape[1], 0, 0, None, iters, L.MU, 0.0, L.LAM0, B,
            out.data_ptr(), cost.data_ptr(), 0, 0)
    rc = lib.tik_fk_refine_robust(*head, *tail, 0) if robust else lib.tik_fk_refine(*head, 0)
    torch.cuda.synchronize()
    return rc, out, cost


# ---------------------------------------------------------------- 1. off is off
@pytest.mark.parametrize("skin", ["sparse", "dense"])
def test_off_is_off(inputs65, skin):
    from temporal_inverse_kinematics_amd import _lib
    th, betas, kps = inputs65
    m = new_model(skin)
    t, k, b = cu(th), cu(kps), cu(betas)
    poses, cost = m.refine_frames(t, k, betas=b, iters=3, mu=L.MU, lam0=L.LAM0)
    off, c_off = m.refine_frames(t, k, betas=b, iters=3, mu=L.MU, lam0=L.LAM0, robust_sigma=0.0, skip_nonfinite=False)
    assert torch.isfinite(poses).all() and torch.equal(off, poses) and torch.equal(c_off, cost)
    rc0, p0, c0 = c_refine(m, False, t, k, b, 3)
    rc1, p1, c1 = c_refine(m, True, t, k, b, 3, (0.0, 0, 0))
    assert rc0 == rc1 == _lib.TIK_OK
    assert torch.equal(p0, poses) and torch.equal(c0, cost) and torch.equal(p1, poses) and torch.equal(c1, cost)
    out = m.refine_frames(t[:2], k[:2], iters=0, debug=True)
    assert len(out) == 4                                     # no weights without a robust term


# ---------------------------------------------------------------- 2. rho and omega
def test_rho_and_omega(model, inputs65):
    th, betas, kps = inputs65
    s2 = RR.SIGMA ** 2
    w = np.random.default_rng(17).uniform(0.5, 2.0, 17).astype(np.float32)
    for jw in (None, w):
        poses, cost, jac, r, om = model.refine_frames(cu(th), cu(kps), betas=cu(betas), joint_weight=cu(jw), iters=1, mu=L.MU,
                                                      lam0=L.LAM0, robust_sigma=RR.SIGMA, debug=True)
        assert om.shape == (65, 17) and r.shape == (65, 51)
        w64 = np.ones(17) if jw is None else jw.astype(np.float64)
        full = np.zeros((65, 55, 3))
        full[:, :22] = th.reshape(65, 22, 3)
        joints = R.sl.smplx_forward(L.consts(), full, betas.astype(np.float64), return_verts=False)[:, R.COCO]
        s_ref = ((L.rel(joints) - L.rel(kps.astype(np.float64))) ** 2).sum(2)
        cost_ref = 0.5 * (w64 * s2 * s_ref / (s2 + s_ref)).sum(1)
        ec = np.abs(cost[:, 0].cpu().numpy() - cost_ref).max()
        s_gpu = (r.cpu().numpy().astype(np.float64).reshape(65, 17, 3) ** 2).sum(2)
        om_ref = w64 * (s2 / (s2 + s_gpu)) ** 2
        eo = (np.abs(om.cpu().numpy() - om_ref) / om_ref).max()
        print(f"weights={'ones' if jw is None else 'random'}: max |cost0 - float64| = {ec:.3e}, "
              f"max relative |omega - float64 on dbg_r| = {eo:.3e}")
        assert ec < 1e-4
        assert eo < 1e-5
        c = cost.cpu().numpy()
        assert np.isfinite(c).all() and (np.diff(c, axis=1) <= 0).all()


# ---------------------------------------------------------------- 3. the outlier scenario
def test_outlier_scenario(model):
    c = RR.case_outlier()
    assert (c["d_plain"] >= 0.3).all() and (c["d_robust"] <= 0.25 * c["d_plain"]).all()      # on the CPU first
    kw = dict(iters=c["iters"], mu=L.MU, lam0=L.LAM0)
    plain, _ = model.refine_frames(cu(c["th0"]), cu(c["kps"]), **kw)
    poses, cost = model.refine_frames(cu(c["th0"]), cu(c["kps"]), robust_sigma=RR.SIGMA, **kw)
    cost = cost.cpu().numpy().T
    assert np.isfinite(cost).all() and torch.isfinite(poses).all()
    assert (np.diff(cost, axis=0) <= 0).all(), cost
    assert np.abs(cost[0] - c["hist"][0]).max() < 1e-4
    print(f"final robust cost per frame: GPU {cost[-1]}, reference {c['hist'][-1]}")
    d_plain = RR.worst_distance(plain.cpu().numpy(), c["kps_clean"])
    d_rob = RR.worst_distance(poses.cpu().numpy(), c["kps_clean"])
    print(f"worst keypoint distance to the clean truth per frame: GPU plain {d_plain}, GPU sigma={RR.SIGMA} {d_rob}, "
          f"ratio {d_rob / d_plain} (reference {c['d_robust'] / c['d_plain']})")
    assert (cost[-1] <= 1.5 * c["hist"][-1] + 1e-8).all(), (cost[-1], c["hist"][-1])
    assert (d_rob <= 0.25 * d_plain).all()
    from temporal_inverse_kinematics_amd.refine import refine_poses
    out = refine_poses(c["th0"], c["kps"], model, iters=c["iters"], prior_weight=L.MU, lam0=L.LAM0, fused=True,
                       robust_sigma=RR.SIGMA)
    assert np.array_equal(out["poses"], poses.cpu().numpy()) and np.array_equal(out["cost"], cost)


# ---------------------------------------------------------------- 4. the missing scenario
def test_missing_scenario(model):
    c = RR.case_missing()
    assert np.array_equal(c["th"], c["th_w"])                                                  # on the CPU first
    kw = dict(iters=c["iters"], mu=L.MU, lam0=L.LAM0)
    t = cu(c["th0"])
    for sigma in (0.0, RR.SIGMA):
        poses, cost = model.refine_frames(t, cu(c["kps"]), skip_nonfinite=True, robust_sigma=sigma, **kw)
        want, cost_w = model.refine_frames(t, cu(c["filled"]), joint_weight=cu(c["w"]), robust_sigma=sigma, **kw)
        assert torch.isfinite(poses).all() and torch.isfinite(cost).all()
        assert torch.equal(poses, want) and torch.equal(cost, cost_w), sigma
        assert torch.equal(poses[4], t[4]) and (cost[4] == 0).all()
        assert (cost[:, -1] < cost[:, 0])[[0, 1, 2, 3, 5]].all()
        if sigma == 0.0:
            cc = cost.cpu().numpy().T
            print(f"final cost per frame: GPU {cc[-1]}, reference {c['hist'][-1]}")
            assert np.abs(cc[0] - c["hist"][0]).max() < 1e-4
            assert (cc[-1] <= 1.5 * c["hist"][-1] + 1e-8).all()
    # the flag off: every frame holds a NaN keypoint, and behaves as today
    poses, cost = model.refine_frames(t, cu(c["kps"]), **kw)
    assert torch.equal(poses, t) and torch.isnan(cost).all()
    from temporal_inverse_kinematics_amd.refine import refine_poses
    out = refine_poses(c["th0"], c["kps"], model, iters=c["iters"], prior_weight=L.MU, lam0=L.LAM0, fused=True, skip_nonfinite=True)
    want, _ = model.refine_frames(t, cu(c["kps"]), skip_nonfinite=True, **kw)
    assert np.array_equal(out["poses"], want.cpu().numpy())


# ---------------------------------------------------------------- 5. bits
def test_bits(model, inputs65):
    th, betas, kps = inputs65
    kps = kps.copy()
    kps[0, 3, 1] = np.nan          # a missing keypoint in a checked row
    kps[63, 12] = np.inf           # a missing hip: the whole frame
    kps[5, 0, 0] = np.nan
    t, k, b = cu(th), cu(kps), cu(betas)
    kw = dict(iters=3, mu=L.MU, lam0=L.LAM0, robust_sigma=RR.SIGMA, skip_nonfinite=True)
    poses, cost, _, _, om = model.refine_frames(t, k, betas=b, debug=True, **kw)
    assert torch.isfinite(poses).all() and torch.isfinite(cost).all() and torch.isfinite(om).all()
    assert om[0, 3] == 0 and (om[63] == 0).all() and (om[64] > 0).all() and torch.equal(poses[63], t[63])
    nodbg, c_nodbg = model.refine_frames(t, k, betas=b, **kw)
    assert torch.equal(nodbg, poses) and torch.equal(c_nodbg, cost)
    for i in CHECKED:
        p1, c1 = model.refine_frames(t[i:i + 1], k[i:i + 1], betas=b[i:i + 1], **kw)
        assert torch.equal(p1[0], poses[i]) and torch.equal(c1[0], cost[i]), i
    same, c0 = model.refine_frames(t, k, betas=b, iters=0, robust_sigma=RR.SIGMA, skip_nonfinite=True)
    assert torch.equal(same, t) and torch.equal(c0[:, 0], cost[:, 0])


# ---------------------------------------------------------------- 6. refusals
def test_refusals(model, inputs65):
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.refine import refine_poses
    th, betas, kps = inputs65
    t, k, b = cu(th[:3]), cu(kps[:3]), cu(betas[:3])
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            model.refine_frames(t, k, robust_sigma=bad)
        with pytest.raises(ValueError):
            refine_poses(th[:3], kps[:3], model, fused=True, robust_sigma=bad)
    with pytest.raises(ValueError):
        refine_poses(th[:3], kps[:3], model, robust_sigma=0.1)
    with pytest.raises(ValueError):
        refine_poses(th[:3], kps[:3], model, skip_nonfinite=True)
    # the C entry point itself: refused before any device work, the outputs keep their fill
    for tail in ((-0.1, 0, 0), (float("nan"), 0, 0), (0.1, 2, 0), (0.1, 1 | 4, 0), (0.0, -1, 0)):
        rc, out, cost = c_refine(model, True, t, k, b, 1, tail)
        assert rc == _lib.TIK_E_INVALID and "tik_fk_refine_robust" in _lib.last_error(), tail
        assert (out == -7).all() and (cost == -7).all()
    lib = _lib.load()
    assert lib.tik_fk_refine_robust(model._h, t.data_ptr(), 0, 0, k.data_ptr(), 0, 0, 0, 0, None, 1, L.MU, 0.0, L.LAM0, 0,
                                    t.data_ptr(), 0, 0, 0, 0.1, 1, 0, 0) == _lib.TIK_E_INVALID          # B = 0, as tik_fk_refine
    rc, out, cost = c_refine(model, True, t, k, b, 1, (0.1, 1, 0))
    assert rc == _lib.TIK_OK and torch.isfinite(out).all() and torch.isfinite(cost).all()
