"""tik_lm_accumulate + tik_lm_solve_sum / smplx_fk.lm_accumulate + lm_solve_sum:
(sum_b J_b^T W J_b + (mu + lambda) I) delta = -(sum_b J_b^T W r_b + mu prior),
one system whose unknowns are shared by the whole batch.

Inputs are built like system() of tests/test_gpu_lm_solve.py; the float64
condition number of the summed, damped matrix is below 1e4 (asserted on the
CPU). The reference is numpy.linalg.solve in float64 on the same fp32 inputs.
The allowed error is that file's: 4 x the error of the same solve formed in
float32 numpy (each body's normal matrix and gradient in float32, added body by
body in float32) against the float64 solution, plus 1e-6. Each case prints
its ratio (kernel error / float32 numpy error). Measured on the MI355X: 0.88 ..
6.35 over the 14 cases, the largest (6.35) the (768,165,3) ones, whose entries
are one chain of 2304 FMAs where numpy sums in blocks; every error is below
1.7e-7, so those cases pass on the 1e-6 term; DESIGN.md "Shape Jacobian and
sequence solve".
"""
import numpy as np
import pytest
import torch

import fk_shape_ref as S   # noqa: F401  (the module fails to import where the feature is absent)
import memedge as me
from temporal_inverse_kinematics_amd.smplx_fk import LM_RUN, lm_accumulate, lm_solve_sum

pytestmark = pytest.mark.gpu
CASES = [(51, 10, 6), (51, 10, 65), (1, 1, 1), (7, 3, 31), (7, 3, 32), (7, 3, 33), (768, 165, 3)]   # (m, n, B)


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def width(n):
    return n * (n + 1) // 2 + n


def system(B, m, n, seed, prior=True, row_w=True):
    """Random fp32 inputs whose summed, damped normal matrix has a float64 condition number below 1e4."""
    rng = np.random.default_rng(seed)
    J = rng.normal(0, 1, (B, m, n)).astype(np.float32)
    r = rng.normal(0, 1, (B, m)).astype(np.float32)
    p = rng.normal(0, 1, n).astype(np.float32) if prior else None
    w = rng.uniform(0.2, 2.0, m).astype(np.float32) if row_w else None
    if row_w:
        w[m // 2] = 0.0   # a zero row weight
    mu = np.float32(0.25)
    W = np.ones(m) if w is None else w.astype(np.float64)
    J64 = J.astype(np.float64)
    top = np.linalg.eigvalsh(np.einsum("bmi,m,bmj->ij", J64, W, J64))[-1]
    lam = np.float32(top / 2e3 + rng.uniform(0.01, 0.1))
    return J, r, p, w, lam, mu


def solve_np(J, r, p, w, lam, mu, dt):
    B, m, n = J.shape
    W = np.ones(m, dt) if w is None else w.astype(dt)
    N, g = np.zeros((n, n), dt), np.zeros(n, dt)
    for b in range(B):
        Jb = J[b].astype(dt)
        N += (Jb.T * W) @ Jb
        g += (Jb.T * W) @ r[b].astype(dt)
    N = N + (dt(mu) + dt(lam)) * np.eye(n, dtype=dt)
    if p is not None:
        g = g + dt(mu) * p.astype(dt)
    return np.linalg.solve(N, -g), np.linalg.cond(N.astype(np.float64))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    me.lib()


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("extras", [(True, True), (False, False)], ids=["prior_roww", "plain"])
@pytest.mark.parametrize("m,n,B", CASES)
def test_solve_sum_vs_float64(m, n, B, extras):
    J, r, p, w, lam, mu = system(B, m, n, seed=1000 * m + n + B, prior=extras[0], row_w=extras[1])
    ref, cond = solve_np(J, r, p, w, lam, mu, np.float64)
    assert cond < 1e4, cond
    f32, _ = solve_np(J, r, p, w, lam, mu, np.float32)
    e32 = np.abs(f32.astype(np.float64) - ref).max()
    partial = lm_accumulate(cu(J), cu(r), row_weight=cu(w))
    assert partial.shape == ((B + LM_RUN - 1) // LM_RUN, width(n))
    got = lm_solve_sum(partial, mu=float(mu), lam=float(lam), prior=cu(p)).cpu().numpy()
    assert got.shape == (n,) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"(m,n,B)=({m},{n},{B}) extras={extras}: cond={cond:.1f} |gpu-f64|={err:.3e} |np32-f64|={e32:.3e} "
          f"ratio={err / max(e32, 1e-30):.2f}")
    assert err <= 4 * e32 + 1e-6


def test_partial_rows_hold_the_packed_triangle_and_the_gradient():
    """Row 0 of `partial` against float64, entry by entry: the packing is lm_solve's."""
    J, r, _, w, _, _ = system(5, 7, 4, seed=11)
    part = lm_accumulate(cu(J), cu(r), row_weight=cu(w)).cpu().numpy()
    J64, W = J.astype(np.float64), w.astype(np.float64)
    N = np.einsum("bmi,m,bmj->ij", J64, W, J64)
    g = np.einsum("bmi,m,bm->i", J64, W, r.astype(np.float64))
    tri = np.array([N[i, j] for i in range(4) for j in range(i + 1)])
    assert part.shape == (1, width(4))
    assert np.abs(part[0, :10] - tri).max() < 1e-4 and np.abs(part[0, 10:] - g).max() < 1e-4


# ---------------------------------------------------------------- 2. bits of the partial rows
def test_a_partial_row_depends_on_its_own_bodies_only():
    J, r, p, w, lam, mu = system(65, 51, 10, seed=5)
    big = lm_accumulate(cu(J), cu(r), row_weight=cu(w))
    assert big.shape == (3, width(10))
    for q in range(3):
        lo, hi = LM_RUN * q, min(65, LM_RUN * (q + 1))
        own = lm_accumulate(cu(J[lo:hi]), cu(r[lo:hi]), row_weight=cu(w))
        assert torch.equal(own[0], big[q]), q
    # two chunks into two slices of one buffer, the first a multiple of LM_RUN bodies: the rows of one call
    buf = torch.full((3, width(10)), float("nan"), device="cuda")
    lm_accumulate(cu(J[:64]), cu(r[:64]), row_weight=cu(w), out=buf[:2])
    lm_accumulate(cu(J[64:]), cu(r[64:]), row_weight=cu(w), out=buf[2:])
    assert torch.equal(buf, big)
    one = lm_solve_sum(big, mu=float(mu), lam=float(lam), prior=cu(p))
    two = lm_solve_sum(buf, mu=float(mu), lam=float(lam), prior=cu(p), n=10)
    assert torch.equal(one, two)
    assert torch.equal(lm_solve_sum(big, mu=float(mu), lam=float(lam), prior=cu(p)), one)


# ---------------------------------------------------------------- 3. a matrix that is not positive
def test_a_sum_that_is_not_positive_gives_nan_and_writes_nothing_else():
    """mu = lambda = 0 and n > B m: an arithmetic outcome, the kernel returns normally."""
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    n = 5
    J = np.zeros((1, 2, n), np.float32)
    J[0, :, :2] = [[1.0, 2.0], [3.0, 5.0]]          # columns 2.. are zero: the third pivot is exactly 0
    partial = lm_accumulate(cu(J), cu(np.ones((1, 2), np.float32)))
    before = partial.clone()
    out = torch.full((n + 1024,), 7.0, device="cuda")
    assert L.tik_lm_solve_sum(partial.data_ptr(), 1, 0, 0.0, 0.0, n, out.data_ptr(), 0) == _lib.TIK_OK
    torch.cuda.synchronize()
    assert torch.isnan(out[:n]).all()
    assert (out[n:] == 7.0).all() and torch.equal(partial, before)
    assert torch.isnan(lm_solve_sum(partial)).all()
    # the same sum with damping is solved
    assert torch.isfinite(lm_solve_sum(partial, lam=0.5)).all()
    # a pivot that fails late: rank-1 rows, no damping. Four bodies, so that every entry of the sum is 4 and
    # the factorisation is exact (sqrt 4 = 2, 4 / 2 = 2, 4 - 2 * 2 = 0): the second pivot is exactly 0
    J3 = np.zeros((4, 4, 3), np.float32)
    J3[:, 0] = (1, 1, 1)
    assert torch.isnan(lm_solve_sum(lm_accumulate(cu(J3), cu(np.ones((4, 4), np.float32))))).all()


# ---------------------------------------------------------------- 4. errors
def test_rejected_arguments():
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    J, r, p, w, lam, mu = [cu(x) if isinstance(x, np.ndarray) else x for x in system(2, 5, 4, seed=1)]
    part = torch.empty((1, width(4)), device="cuda")
    d = torch.empty((4,), device="cuda")

    def acc(j=J.data_ptr(), rr=r.data_ptr(), o=part.data_ptr(), B=2, m=5, n=4):
        return L.tik_lm_accumulate(j, rr, 0, B, m, n, o, 0)
    for kw in ({"j": 0}, {"rr": 0}, {"o": 0}, {"B": 0}, {"B": -3}, {"m": 0}, {"m": 769}, {"n": 0}, {"n": 166}):
        assert acc(**kw) == _lib.TIK_E_INVALID, kw
        assert "tik_lm_accumulate" in _lib.last_error()
    assert acc() == _lib.TIK_OK

    def solve(q=part.data_ptr(), o=d.data_ptr(), n_part=1, mu=0.1, lam=0.1, n=4):
        return L.tik_lm_solve_sum(q, n_part, 0, mu, lam, n, o, 0)
    for kw in ({"q": 0}, {"o": 0}, {"n_part": 0}, {"n": 0}, {"n": 166}, {"mu": -1.0}, {"mu": float("nan")}, {"lam": -1.0},
               {"lam": float("nan")}):
        assert solve(**kw) == _lib.TIK_E_INVALID, kw
        assert "tik_lm_solve_sum" in _lib.last_error()
    assert solve() == _lib.TIK_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        lm_accumulate(J, r[:, :3].contiguous())
    with pytest.raises(ValueError):
        lm_accumulate(J, r, row_weight=w[:4].contiguous())
    with pytest.raises(ValueError):
        lm_accumulate(J, r, out=torch.empty((2, width(4)), device="cuda"))
    with pytest.raises(ValueError):
        lm_accumulate(J.double(), r)
    with pytest.raises(ValueError):
        lm_solve_sum(part, mu=-1.0)
    with pytest.raises(ValueError):
        lm_solve_sum(part, lam=float("nan"))
    with pytest.raises(ValueError):
        lm_solve_sum(part, n=3)
    with pytest.raises(ValueError):
        lm_solve_sum(part[:, :13].contiguous())
    with pytest.raises(ValueError):
        lm_solve_sum(part, prior=torch.zeros(5, device="cuda"))
