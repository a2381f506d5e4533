"""The CPU side of the fused refinement's tests (no GPU, no library): the float64 reference
(tests/lm_refine_ref.py) meets the conditions the GPU tests lean on, and the Python argument checks of
SMPLX.refine_frames and of a refining OnlineIK raise before anything is asked of the library.

Measured on the reference: the data term of case_refine falls from 1.267 to 7.60e-4; the causal track's mean
second difference is 0.119 without the tie and 0.0084 with smooth = 0.1 (theta0's own: 0.198).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lm_refine_ref as L
from temporal_inverse_kinematics_amd import smplx_fk


def test_reference_refine_converges():
    c = L.case_refine()
    print(f"reference LM: data term {c['data0']:.3e} -> {c['data1']:.3e}, final cost per frame {c['hist'][-1]}")
    assert c["data1"] * 10 <= c["data0"]
    assert np.isfinite(c["hist"]).all() and (np.diff(c["hist"], axis=0) <= 0).all()


def test_reference_causal_tie_smooths_the_track():
    th0, _ = L.track_inputs()
    free, tied = L.case_track(0.0), L.case_track(L.TRACK_S)
    print(f"second difference: theta0 {L.second_difference(th0):.4f}, s=0 {free['d2']:.4f}, s={L.TRACK_S} {tied['d2']:.4f}")
    for c in (free, tied):
        assert np.isfinite(c["hist"]).all() and (np.diff(c["hist"], axis=1) <= 0).all()
    assert tied["d2"] < 0.5 * free["d2"]


def test_closed_form_of_the_two_priors():
    """With every keypoint weight 0 the cost is quadratic and its minimiser is (mu th0 + s thp) / (mu + s): the
    reference reaches it, which pins the scaling of both prior terms in the reference itself."""
    rng = np.random.default_rng(5)
    th0, thp = rng.uniform(-0.3, 0.3, (2, 1, 66))
    kps = L.coco_of(th0)
    o = L.lm(th0, kps, 10, smooth=0.1, prev=thp, weights=np.zeros(17))
    assert np.abs(o["th"] - (L.MU * th0 + 0.1 * thp) / (L.MU + 0.1)).max() < 1e-9


# ---------------------------------------------------------------- argument checks that need no library
@pytest.mark.parametrize("kw", [dict(mu=0.0), dict(mu=-1.0), dict(mu=float("nan")), dict(smooth=-0.1), dict(lam0=0.0),
                                dict(iters=-1), dict(iters=1.5)])
def test_bad_scalars(kw):
    args = dict(iters=3, mu=1e-2, smooth=0.0, lam0=1e-2)
    args.update(kw)
    with pytest.raises(ValueError):
        smplx_fk.check_refine_scalars(**args)
    assert smplx_fk.check_refine_scalars(3, 1e-2, 0.0, 1e-2) == (3, 1e-2, 0.0, 1e-2)


def test_selection_of_refine_frames():
    assert smplx_fk.resolve_refine_select("coco", 77) == L.R.COCO
    with pytest.raises(ValueError, match="three vertices"):
        smplx_fk.resolve_refine_select(L.R.COCO[:16] + [55 + 21], 144)      # the first static landmark
    with pytest.raises(ValueError):
        smplx_fk.resolve_refine_select(L.R.COCO[:16], 144)
    with pytest.raises(ValueError):
        smplx_fk.resolve_refine_select(None, 144)


def test_refine_frames_refuses_before_the_device():
    """Wrong shapes and a non-contiguous tensor are ValueErrors (CPU tensors here: a call that passed the checks
    would raise the RuntimeError of _lib.require_gpu instead)."""
    me = SimpleNamespace(num_joints=77, num_betas=10, _h=None)
    call = smplx_fk.SMPLX.refine_frames
    poses, kps = torch.zeros(4, 66), torch.zeros(4, 17, 3)
    bad = [dict(poses=torch.zeros(4, 65)), dict(poses=torch.zeros(66)), dict(kps=torch.zeros(4, 51)), dict(kps=torch.zeros(3, 17, 3)),
           dict(prior=torch.zeros(3, 66)), dict(prev=torch.zeros(4, 65)), dict(betas=torch.zeros(9)), dict(betas=torch.zeros(3, 10)),
           dict(joint_weight=torch.zeros(16)), dict(joint_weight=torch.zeros(4, 17, 1)), dict(poses=torch.zeros(66, 4).t()),
           dict(kps=torch.zeros(4, 17, 3, dtype=torch.float64)), dict(mu=0.0), dict(smooth=-1.0),
           dict(select=L.R.COCO[:16] + [55 + 21])]
    for kw in bad:
        args = dict(poses=poses, kps=kps)
        args.update(kw)
        with pytest.raises(ValueError):
            call(me, **args)
    with pytest.raises(RuntimeError):           # everything in order: only now is the device asked for
        call(me, poses, kps)


def test_online_refine_arguments():
    from temporal_inverse_kinematics_amd.streaming import OnlineIK, check_refine_args
    body = SimpleNamespace(_h=1, num_betas=10)
    assert check_refine_args(0, None, None, 1e-2, 0.0, 1e-2, None)[0] == 0
    it, mu, s, lam0, b, w = check_refine_args(2, body, np.zeros(10), 1e-2, 0.1, 1e-2, np.ones(17))
    assert (it, mu, s, lam0) == (2, 1e-2, 0.1, 1e-2) and b.dtype == np.float32 and w.shape == (17,)
    with pytest.raises(ValueError, match="smplx_model"):
        check_refine_args(2, None, None, 1e-2, 0.0, 1e-2, None)
    for kw in (dict(prior_weight=0.0), dict(smooth_weight=-0.1), dict(lam0=0.0), dict(joint_weight=-np.ones(17)),
               dict(joint_weight=np.ones(16)), dict(betas=np.zeros(9)), dict(refine=-1)):
        args = dict(refine=2, smplx_model=body, betas=None, prior_weight=1e-2, smooth_weight=0.0, lam0=1e-2, joint_weight=None)
        args.update(kw)
        with pytest.raises(ValueError):
            check_refine_args(**args)
    # the constructor checks first: no model handle, no library needed to be refused
    with pytest.raises(ValueError, match="smplx_model"):
        OnlineIK(object(), win_size=9, refine=2)
    with pytest.raises(ValueError):
        OnlineIK(object(), win_size=9, refine=2, smplx_model=body, prior_weight=0.0)
