"""refine._lm_loop, the Levenberg-Marquardt policy of refine_poses and
refine_smooth (accept where the cost fell, lambda / 3 on accept and * 3 on
reject, a NaN step rejected, one history row per iteration), on a toy problem
with CPU tensors: it is pure torch and calls no library. No GPU.

The toy: frames of 3 unknowns, cost 1/2 |A theta - b|^2 with A (5,3), in
float64. The step is the damped Gauss-Newton system
(A^T A + lambda I) delta = -A^T (A theta - b) solved exactly by
torch.linalg.solve: with lambda > 0 every step lowers the cost strictly and
stops short of the minimum, so a run of accepted steps stays one (the undamped
step reaches the minimum at once, and the next candidate's equal cost would be
a rejection). With lambda = 1e-6 the step is the undamped one to six digits:
three times it lands twice as far beyond the minimum as theta was before it,
at four times the excess cost.
"""
import pytest
import torch

from temporal_inverse_kinematics_amd.refine import _lm_loop

FRAMES = 3


class Toy:
    """frame_cost(th) (FRAMES,), exact(th, lam per frame) -> delta; step records the (th, lam) it was given."""

    def __init__(self, lam0, seg=None, spoil=None):
        g = torch.Generator().manual_seed(5)
        self.A = torch.randn((FRAMES, 5, 3), generator=g, dtype=torch.float64)
        self.b = torch.randn((FRAMES, 5), generator=g, dtype=torch.float64)
        self.th0 = torch.randn((FRAMES, 3), generator=g, dtype=torch.float64)
        self.seg = torch.arange(FRAMES) if seg is None else torch.tensor(seg)     # the unit of each frame
        self.units = int(self.seg.max()) + 1
        self.lam0 = torch.full((self.units,), float(lam0), dtype=torch.float64)
        self.spoil = spoil                                                        # delta -> delta, on iteration 0 only
        self.seen = []

    def residual(self, th):
        return torch.einsum("fmn,fn->fm", self.A, th) - self.b

    def frame_cost(self, th):
        return 0.5 * self.residual(th).square().sum(1)

    def cost_of(self, th):
        return torch.zeros(self.units, dtype=torch.float64).index_add(0, self.seg, self.frame_cost(th))

    def exact(self, th, lam):
        N = self.A.transpose(1, 2) @ self.A + lam[self.seg][:, None, None] * torch.eye(3, dtype=torch.float64)
        g = torch.einsum("fmn,fm->fn", self.A, self.residual(th))
        return torch.linalg.solve(N, -g)

    def step(self, th, lam):
        self.seen.append((th.clone(), lam.clone()))
        delta = self.exact(th, lam)
        return self.spoil(delta) if self.spoil is not None and len(self.seen) == 1 else delta

    def run(self, iters):
        return _lm_loop(self.th0, self.cost_of(self.th0), self.lam0, iters, self.step, self.cost_of, lambda ok: ok[self.seg])


def test_exact_steps_are_all_accepted():
    t, iters = Toy(1.0), 4
    th, hist = t.run(iters)
    assert hist.shape == (iters + 1, FRAMES) and th.shape == (FRAMES, 3)
    assert torch.equal(hist[0], t.cost_of(t.th0)) and torch.equal(hist[-1], t.cost_of(th))
    assert (hist[1:] < hist[:-1]).all(), hist
    lam = t.lam0
    for it in range(iters):
        assert torch.equal(t.seen[it][1], lam), it             # lam0, lam0 / 3, lam0 / 9, ...
        lam = lam / 3.0
    assert len(t.seen) == iters


def nan_for_frame_1(delta):
    delta = delta.clone()
    delta[1] = float("nan")
    return delta


def thrice_for_frame_1(delta):
    delta = delta.clone()
    delta[1] *= 3.0
    return delta


@pytest.mark.parametrize("lam0,spoil", [(1.0, nan_for_frame_1), (1e-6, thrice_for_frame_1)], ids=["nan", "overshoot"])
def test_a_step_that_does_not_lower_the_cost_is_rejected(lam0, spoil):
    clean, t = Toy(lam0), Toy(lam0, spoil=spoil)
    worse = t.cost_of(t.th0 + spoil(t.exact(t.th0, t.lam0)))[1]
    assert not worse < t.cost_of(t.th0)[1]                     # NaN, or a cost that rose: the premise
    (th_c, hist_c), (th, hist) = clean.run(2), t.run(2)
    assert torch.isfinite(th).all() and torch.isfinite(hist).all()
    # unit 1 after iteration 0: the poses it had, three times the lambda, the cost row repeated
    assert torch.equal(t.seen[1][0][1], t.th0[1])
    assert t.seen[1][1][1] == t.lam0[1] * 3.0
    assert hist[1, 1] == hist[0, 1] and hist[2, 1] < hist[1, 1]
    # the other units never see it
    for u in (0, 2):
        assert torch.equal(hist[:, u], hist_c[:, u]) and torch.equal(th[u], th_c[u])
        assert t.seen[1][1][u] == t.lam0[u] / 3.0
    assert hist_c[1, 1] < hist_c[0, 1]


def test_no_iterations_returns_the_inputs():
    t = Toy(1.0)
    th, hist = t.run(0)
    assert torch.equal(th, t.th0) and hist.shape == (1, FRAMES) and torch.equal(hist[0], t.cost_of(t.th0))
    assert t.seen == []


def test_a_sequence_moves_as_a_whole_or_not_at_all():
    seg = [0, 0, 1]                                            # sequences of 2 frames and of 1
    clean, t = Toy(1.0, seg), Toy(1.0, seg, spoil=nan_for_frame_1)
    (th_c, hist_c), (th, hist) = clean.run(1), t.run(1)
    assert hist.shape == (2, 2)
    assert (th_c != t.th0).any(1).all()                        # accepted: every frame of both sequences moved
    assert torch.equal(th[:2], t.th0[:2]) and hist[1, 0] == hist[0, 0]     # frame 1's NaN keeps frame 0 back too
    assert torch.equal(th[2], th_c[2]) and hist[1, 1] == hist_c[1, 1] < hist[0, 1]
