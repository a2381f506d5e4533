"""Host side of the FK shape Jacobian / sequence solve: the ValueError paths of
SMPLX.joints_shape_jacobian, lm_accumulate, lm_solve_sum, fit_shape and
refine_sequence (reached without loading the library), the --fit-shape
argument, and the C ABI's three new entry points (declared, exported, refusing
bad arguments before any device call). No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from temporal_inverse_kinematics_amd.smplx_fk import LM_RUN, lm_accumulate, lm_solve_sum   # noqa: F401  (the feature)


@pytest.fixture
def no_library(monkeypatch):
    from temporal_inverse_kinematics_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the validators must not touch the library")
    monkeypatch.setattr(_lib, "load", refuse)


def _bare_model():
    """An SMPLX object without a handle: what the validators read, nothing else."""
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    m = object.__new__(SMPLX)
    m.num_joints, m.num_static_joints, m.num_betas, m.device = 144, 127, 10, torch.device("cpu")
    return m


def test_joints_shape_jacobian_validates_before_the_library(no_library):
    m = _bare_model()
    pose = torch.zeros((2, 55, 3))
    for kw in ({"select": None}, {"select": "body25"}, {"select": [144]}, {"select": [-1]}, {"select": []},
               {"select": [0] * 257}, {"select": [0, 127]}, {"select": [143]}):
        with pytest.raises(ValueError):
            m.joints_shape_jacobian(pose, **kw)
    with pytest.raises(ValueError, match="contour"):
        m.joints_shape_jacobian(pose, select=[130])
    with pytest.raises(RuntimeError, match="GPU"):   # a valid selection on the CPU: refused, no fallback
        m.joints_shape_jacobian(pose, select="coco")


def test_lm_accumulate_validates_before_the_library(no_library):
    from temporal_inverse_kinematics_amd.smplx_fk import LM_MAX_N, LM_RUN, lm_accumulate
    assert LM_RUN == 32 and LM_MAX_N == 165
    J, r = torch.zeros((2, 5, 4)), torch.zeros((2, 5))
    bad = [dict(jac=J[0]), dict(r=r[:, :4]), dict(r=r[0]), dict(row_weight=torch.zeros(4)), dict(jac=torch.zeros((2, 5, 166))),
           dict(jac=torch.zeros((2, 769, 4)), r=torch.zeros((2, 769))), dict(jac=torch.zeros((0, 5, 4))),
           dict(jac=J.double()), dict(r=r.double()), dict(jac=torch.zeros((2, 5, 8))[:, :, ::2]),
           dict(out=torch.zeros((2, 14))), dict(out=torch.zeros((1, 13))), dict(out=torch.zeros((1, 14), dtype=torch.float64))]
    for kw in bad:
        a = dict(jac=J, r=r)
        a.update(kw)
        with pytest.raises(ValueError):
            lm_accumulate(**a)
    with pytest.raises(RuntimeError, match="GPU"):
        lm_accumulate(J, r)


def test_lm_solve_sum_validates_before_the_library(no_library):
    from temporal_inverse_kinematics_amd.smplx_fk import lm_solve_sum
    part = torch.zeros((3, 14))                      # n = 4: 10 + 4
    bad = [dict(partial=part[0]), dict(partial=torch.zeros((0, 14))), dict(partial=torch.zeros((3, 13))), dict(n=3), dict(n=0),
           dict(partial=torch.zeros((1, 166 * 167 // 2 + 166))), dict(mu=-0.5), dict(mu=float("nan")), dict(lam=-1e-3),
           dict(lam=float("nan")), dict(prior=torch.zeros(5)), dict(prior=torch.zeros((1, 4))), dict(partial=part.double()),
           dict(prior=torch.zeros(4, dtype=torch.float64))]
    for kw in bad:
        a = dict(partial=part)
        a.update(kw)
        with pytest.raises(ValueError):
            lm_solve_sum(**a)
    with pytest.raises(RuntimeError, match="GPU"):
        lm_solve_sum(part, mu=0.1, n=4)


def test_fit_shape_and_refine_sequence_validate_before_the_library(no_library):
    from temporal_inverse_kinematics_amd.refine import fit_shape, refine_poses, refine_sequence
    m = _bare_model()
    poses, kps = np.zeros((3, 66), np.float32), np.zeros((3, 17, 3), np.float32)
    for kw in (dict(shape_weight=0), dict(shape_weight=0.0), dict(shape_weight=-1e-3), dict(shape_weight=float("nan")),
               dict(joint_weight=np.ones(16)), dict(joint_weight=-np.ones(17)), dict(joint_weight=np.ones((3, 17))),
               dict(joint_weight=np.full(17, np.nan)), dict(betas=np.zeros(9)),
               dict(betas=np.zeros((1, 10))), dict(betas=np.full(10, np.nan))):
        with pytest.raises(ValueError):
            fit_shape(poses, kps, m, **kw)
        with pytest.raises(ValueError):
            refine_sequence(poses, kps, m, **kw)
    with pytest.raises(ValueError, match="short or static sequence"):
        fit_shape(poses, kps, m, shape_weight=0)
    for kw in (dict(rounds=-1), dict(iters=-1), dict(prior_weight=0), dict(prior_weight=float("nan")), dict(lam0=0.0)):
        with pytest.raises(ValueError):
            refine_sequence(poses, kps, m, **kw)
    for fn in (fit_shape, refine_sequence):
        with pytest.raises(ValueError):
            fn(poses[:, :60], kps, m)
        with pytest.raises(ValueError):
            fn(poses, kps[:2], m)
        with pytest.raises(ValueError):
            fn(poses[0], kps, m)
    for bad in (poses[:2], poses[:, :60], poses[0]):
        with pytest.raises(ValueError, match="prior_poses"):
            refine_poses(poses, kps, m, prior_poses=bad)


def test_fit_shape_argument_parses(no_library):
    from temporal_inverse_kinematics_amd import inference
    p = inference.build_parser()
    a = p.parse_args(["seq.npz", "synthetic", "--refine", "5", "--fit-shape", "3", "--check"])
    assert a.fit_shape == 3 and a.refine == 5 and a.check and a.smplx_dir == "synthetic"
    assert p.parse_args(["seq.npz"]).fit_shape == 0
    assert p.parse_args(["seq.npz", "synthetic", "--refine", "5"]).fit_shape == 0
    with pytest.raises(SystemExit):
        p.parse_args(["seq.npz", "--fit-shape", "many"])
    for argv in (["seq.npz", "--refine", "2", "--fit-shape", "2"],              # no SMPL-X dir
                 ["seq.npz", "synthetic", "--fit-shape", "2"],                  # no pose iterations
                 ["seq.npz", "synthetic", "--refine", "0", "--fit-shape", "2"],
                 ["seq.npz", "synthetic", "--refine", "2", "--fit-shape", "-1"]):
        with pytest.raises(SystemExit):
            inference.main(argv)
    with pytest.raises(ValueError):
        inference.run_test("seq.npz", None, refine=2, fit_shape=2)
    with pytest.raises(ValueError):
        inference.run_test("seq.npz", "synthetic", refine=0, fit_shape=2)
    with pytest.raises(ValueError):
        inference.run_test("seq.npz", "synthetic", refine=2, fit_shape=-1)
    assert inference._betas_path("out/poses.npy") == "out/poses.betas.npy"
    assert inference._betas_path("poses") == "poses.betas.npy"


def test_header_declares_and_library_exports_the_entry_points():
    from temporal_inverse_kinematics_amd import _build, _lib
    txt = open(os.path.join(REPO, "include", "tik.h")).read()
    for name in ("tik_fk_joints_shape_jacobian", "tik_lm_accumulate", "tik_lm_solve_sum"):
        assert re.search(rf"^int {name}\(", txt, re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r"^#define TIK_LM_RUN 32\b", txt, re.M)
    assert "1337 + 165 nb" in txt                    # the workspace budget is written down beside tik_fk_joints'
    _build.build()
    lib = _lib.load()
    for name in ("tik_fk_joints_shape_jacobian", "tik_lm_accumulate", "tik_lm_solve_sum"):
        assert hasattr(lib, name), name
    # refused on the host, before any device call
    assert lib.tik_fk_joints_shape_jacobian(None, None, None, None, None, 1, None, 0, None, None, None) == _lib.TIK_E_INVALID
    assert "tik_fk_joints_shape_jacobian" in _lib.last_error()
    one = (_lib.ctypes.c_float * 4)()
    p = _lib.ctypes.addressof(one)
    for j, r, o in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.tik_lm_accumulate(j, r, None, 1, 1, 1, o, None) == _lib.TIK_E_INVALID
        assert "tik_lm_accumulate" in _lib.last_error()
    for B, m, n in ((0, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 769, 1), (1, 1, 0), (1, 1, 166)):
        assert lib.tik_lm_accumulate(p, p, None, B, m, n, p, None) == _lib.TIK_E_INVALID, (B, m, n)
        assert "tik_lm_accumulate" in _lib.last_error()
    assert lib.tik_lm_solve_sum(None, 1, None, 0.0, 0.0, 1, p, None) == _lib.TIK_E_INVALID
    assert lib.tik_lm_solve_sum(p, 1, None, 0.0, 0.0, 1, None, None) == _lib.TIK_E_INVALID
    for n_part, mu, lam, n in ((0, 0.0, 0.0, 1), (1, -1.0, 0.0, 1), (1, float("nan"), 0.0, 1), (1, 0.0, -1.0, 1),
                               (1, 0.0, float("nan"), 1), (1, 0.0, 0.0, 0), (1, 0.0, 0.0, 166)):
        assert lib.tik_lm_solve_sum(p, n_part, None, mu, lam, n, p, None) == _lib.TIK_E_INVALID, (n_part, mu, lam, n)
        assert "tik_lm_solve_sum" in _lib.last_error()
