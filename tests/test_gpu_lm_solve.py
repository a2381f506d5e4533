"""tik_lm_solve / smplx_fk.lm_solve: (J^T W J + (mu + lambda_b) I) delta = -(J^T W r + mu prior).

The reference is numpy.linalg.solve in float64 on the same fp32 inputs. The
allowed error is measured, not fixed: 4 x the error of a float32
numpy.linalg.solve of the same systems (normal matrix and right-hand side
formed in float32 too) against that float64 solution, plus 1e-6; the factor
covers a different but equally valid summation order. Each case prints its
ratio (kernel error / float32 numpy error). Measured on the MI355X: 0.84 ..
2.68 over the 20 cases; the largest (1.9 .. 2.7) are the (768,165) cases, the
(51,66) ones 0.84 .. 1.94; DESIGN.md "LM solve".
"""
import numpy as np
import pytest
import torch

import fk_jacobian_ref as R   # noqa: F401  (the module fails to import where the feature is absent)
import memedge as me
from temporal_inverse_kinematics_amd.smplx_fk import lm_solve

pytestmark = pytest.mark.gpu
SHAPES = [(51, 66), (1, 1), (3, 165), (768, 165), (51, 7)]


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def system(B, m, n, seed, prior=True, row_w=True):
    """Random fp32 inputs whose damped normal matrix has a float64 condition number below 1e4."""
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 1, (B, m, n)).astype(np.float32)
    r = rng.normal(0, 1, (B, m)).astype(np.float32)
    p = rng.normal(0, 1, (B, n)).astype(np.float32) if prior else None
    w = rng.uniform(0.2, 2.0, m).astype(np.float32) if row_w else None
    if row_w:
        w[m // 2] = 0.0   # a zero row weight
    mu = np.float32(0.25)
    # lambda: the largest eigenvalue of J^T W J is at most |W| |J|_F^2; (top + d) / d < 1e4 with room to spare
    W = np.ones(m) if w is None else w.astype(np.float64)
    top = np.array([np.linalg.eigvalsh((J[b].astype(np.float64).T * W) @ J[b].astype(np.float64))[-1] for b in range(B)])
    lam = (top / 2e3 + rng.uniform(0.01, 0.1, B)).astype(np.float32)
    return J, r, p, w, lam, mu


def solve_np(J, r, p, w, lam, mu, dt):
    B, m, n = J.shape
    out = np.empty((B, n), dt)
    conds = []
    W = np.ones(m, dt) if w is None else w.astype(dt)
    for b in range(B):
        Jb = J[b].astype(dt)
        N = (Jb.T * W) @ Jb + (dt(mu) + dt(lam[b])) * np.eye(n, dtype=dt)
        g = (Jb.T * W) @ r[b].astype(dt) + (dt(mu) * p[b].astype(dt) if p is not None else 0)
        out[b] = np.linalg.solve(N, -g)
        conds.append(np.linalg.cond(N.astype(np.float64)))
    return out, max(conds)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    me.lib()


@pytest.mark.parametrize("extras", [(True, True), (False, False)], ids=["prior_roww", "plain"])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("m,n", SHAPES)
def test_lm_solve_vs_float64(m, n, B, extras):
    J, r, p, w, lam, mu = system(B, m, n, seed=1000 * m + n + B, prior=extras[0], row_w=extras[1])
    ref, cond = solve_np(J, r, p, w, lam, mu, np.float64)
    assert cond < 1e4, cond
    f32, _ = solve_np(J, r, p, w, lam, mu, np.float32)
    e32 = np.abs(f32.astype(np.float64) - ref).max()
    got = lm_solve(cu(J), cu(r), cu(lam), float(mu), cu(p), cu(w)).cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"(m,n)=({m},{n}) B={B} extras={extras}: cond={cond:.1f} |gpu-f64|={err:.3e} |np32-f64|={e32:.3e} "
          f"ratio={err / max(e32, 1e-30):.2f}")
    assert err <= 4 * e32 + 1e-6


def test_bits_do_not_depend_on_the_batch():
    J, r, p, w, lam, mu = system(65, 51, 66, seed=5)
    big = lm_solve(cu(J), cu(r), cu(lam), float(mu), cu(p), cu(w))
    for b in (0, 64):
        one = lm_solve(cu(J[b:b + 1]), cu(r[b:b + 1]), cu(lam[b:b + 1]), float(mu), cu(p[b:b + 1]), cu(w))
        assert torch.equal(one[0], big[b])
    assert torch.equal(lm_solve(cu(J), cu(r), cu(lam), float(mu), cu(p), cu(w)), big)


def test_a_matrix_that_is_not_positive_gives_nan_for_that_body_only():
    """J = 0, mu = 0, lambda = -1 for one body: an arithmetic outcome, the kernel returns normally."""
    J, r, p, w, lam, _ = system(5, 51, 66, seed=9, prior=False, row_w=False)
    ref = lm_solve(cu(J), cu(r), cu(lam), 0.0)
    J2, lam2 = J.copy(), lam.copy()
    J2[2] = 0.0
    lam2[2] = -1.0
    got = lm_solve(cu(J2), cu(r), cu(lam2), 0.0)
    torch.cuda.synchronize()
    assert torch.isnan(got[2]).all()
    keep = [0, 1, 3, 4]
    assert torch.equal(got[keep], ref[keep])
    # a pivot that fails late: rank-1 J, no damping left after lambda cancels mu
    J3 = np.zeros((1, 4, 3), np.float32)
    J3[0, 0] = (1, 1, 1)
    out = lm_solve(cu(J3), cu(np.ones((1, 4), np.float32)), cu(np.array([-0.5], np.float32)), 0.5)
    assert torch.isnan(out).all()


def test_rejected_arguments():
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    J, r, p, w, lam, mu = [cu(x) if isinstance(x, np.ndarray) else x for x in system(2, 5, 4, seed=1)]
    d = torch.empty((2, 4), device="cuda")

    def call(j=J.data_ptr(), rr=r.data_ptr(), l=lam.data_ptr(), o=d.data_ptr(), mu=0.1, B=2, m=5, n=4):
        return L.tik_lm_solve(j, rr, 0, 0, l, mu, B, m, n, o, 0)
    for kw in ({"j": 0}, {"rr": 0}, {"l": 0}, {"o": 0}, {"mu": -1.0}, {"mu": float("nan")}, {"B": 0}, {"m": 0}, {"m": 769},
               {"n": 0}, {"n": 166}):
        assert call(**kw) == _lib.TIK_E_INVALID, kw
    assert call() == _lib.TIK_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        lm_solve(J, r, lam, mu=-1.0)
    with pytest.raises(ValueError):
        lm_solve(J, r[:, :3].contiguous(), lam)
    with pytest.raises(ValueError):
        lm_solve(torch.zeros((1, 2, 166), device="cuda"), torch.zeros((1, 2), device="cuda"), torch.ones(1, device="cuda"))
