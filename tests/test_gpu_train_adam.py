"""Adam on the GPU (adam_kernel behind tik_trainer_step) from an arbitrary
optimizer state, every element against its exact expected value.

The free-running comparison of several steps with the CPU oracle cannot be
tight (test_gpu_train.py's docstring: a rounding-noise gradient moves its
parameter by +-lr with a sign set by summation order). Here Adam is checked on
the GPU's own gradient instead: exp_avg = m0 and exp_avg_sq = v0 are written
through tik_trainer_write and the step count through tik_trainer_set_steps,
one step runs, and g (the gradient that step computed), p1, m1, v1 are read
back. The reference is torch.optim.Adam, the library the reference trains
with, on float64 CPU copies: state = {step: steps0, exp_avg: m0, exp_avg_sq:
v0}, p.grad = the GPU's g, one opt.step(). Every element of every parameter
is checked, noise gradients included.

m0 and v0 (per tensor, seeded, scaled to S = max|g| of the tensor, taken from
a throw-away trainer's first step on the same batch: the gradient does not
depend on m or v): m0 = +-S * 10^U(-2,1) with a random sign, so both signs
relative to g; v0 = S^2 * 10^U(-4,4); and three runs of n/8 elements each at
the head of the tensor: v0 = 0 exactly (m0 as above), m0 = v0 = 0 (the eps
term dominates where g is noise), v0 = 1e-30; the last element has v0 = 1e4 S^2.

Bounds, u = 2^-24 (the fp32 unit roundoff), b1 = 0.9, b2 = 0.999:

  m1 = m0 + w1 * (g - m0), w1 = fl(1 - b1): the subtraction (u|g - m0|, times
  w1), w1's own rounding (u w1 |g - m0|), the product and the sum (one
  rounding if the compiler contracts them into an FMA, two if not: at most
  u w1 |g - m0| + u |m1|). With |g - m0|, |m1| <= |m0| + |g|:
  (0.1 + 0.1 + 0.1 + 1) u < 4u:          |m1 - m1_ref| <= 4u (|m0| + |g|).
  v1 = fl(v0 * fl(b2)) + fl(1 - b2) * g * g: b2's rounding (u b2 v0), the
  product (u v0), 1 - b2's rounding and the two products ((1 + 2) u * 1e-3 g^2,
  two of the three roundings if contracted), the sum (u v1 <= u (v0 + g^2)):
  under 3.1u v0 + 1.1u g^2:               |v1 - v1_ref| <= 4u (v0 + g^2).
  A contracted FMA only removes a rounding; neither bound is loosened for it.

  The update, resolved separately so that the rounding of m1 and v1 does not
  enter: D = p1 - p0 (both cast to float64: exact) against
  D64 = -(lr / bc1) * m1 / (sqrt(v1) / sqrt(bc2) + eps) in float64 from the
  GPU's own m1 and v1, bc = 1 - beta^(steps0 + 1):
                     |D - D64| <= 8u |D64| + 2^-23 max(|p0|, |p1|).
  8u: sqrtf, the division by fl(sqrt(bc2)) and that constant's rounding, the
  sum with fl(eps), m1 / denom, the product with step_size, step_size =
  fl(-fl(lr) / bc1) (lr arrives as a float: two roundings), 8 roundings of at
  most u each; the second term is the final rounding into p (u |p1|, doubled).
  An exponent off by one at steps0 = 999 changes D by 2.9e-4 relative.

  p1 against the torch step, the propagation written out: with dm, dv the
  two moment bounds, d = sqrt(v1) / sqrt(bc2) + eps of the GPU's v1 and d_ref
  of torch's, |sqrt(v1) - sqrt(v1_ref)| <= dv / (sqrt(v1) + sqrt(v1_ref)) =: ds,
  |m1 / d - m1_ref / d_ref| <= dm / d + |m1_ref| (ds / sqrt(bc2)) / (d d_ref):
  |p1 - p1_ref| <= 8u |D64| + 2^-23 max(|p0|, |p1|)
                   + (lr / bc1) (dm / d + |m1_ref| ds / (sqrt(bc2) d d_ref)).

Carried state: one trainer, six steps on six batches; one float64
torch.optim.Adam replays them on the GPU's g of each step. The error of a
moment after step k is at most the sum of k one-step errors (the recurrence
contracts: factors b1, b2 < 1), so it is within k x the one-step bound taken
at the largest |m| + |g| (v + g^2) the element has seen so far; p within k x
the largest one-step p bound so far, each evaluated with that step's
(accumulated) moment bounds.

What this caught when it was written: the bias corrections and the weights
1 - beta were computed from betas already rounded to fp32 (1 - 0.999f =
0.99998712e-3), which put sqrt(bc2), and so every update, 6e-6 = 108u off
torch's (the D check at every steps0). The betas are doubles on the host now."""
import zlib

import numpy as np
import pytest
import torch

import trainref as tref

pytestmark = pytest.mark.gpu

U = tref.U
B1, B2, EPS = 0.9, 0.999, 1e-8
N, T = 8, 9


@pytest.fixture(scope="module")
def lib():
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    return True


def _trainer(lr):
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    return GpuTrainer(tref.model(tref.weights(), T), lr=lr)


def _step(tr, b):
    x, tgt, mask = (torch.from_numpy(a).cuda() for a in b)
    return float(tr.step(x, tgt, mask))


def _set_steps(tr, steps):
    from temporal_inverse_kinematics_amd import _lib
    _lib.check(_lib.load().tik_trainer_set_steps(tr._h.h, steps), "tik_trainer_set_steps")


def _params(tr):
    return [n for n, _, kind in tr._names if kind == 0]


def _read(tr, what):
    return {k: tr.tensor(k, what).cpu().numpy() for k in _params(tr)}


@pytest.fixture(scope="module")
def scale(lib):
    """max|g| per tensor of the first step on the one-step batch (a throw-away trainer)."""
    tr = _trainer(1e-4)
    _step(tr, tref.batch(N, T, 51))
    return {k: float(np.abs(g).max()) for k, g in _read(tr, "grad").items()}


def _moments(name, shape, S):
    """(m0, v0) fp32 for one tensor: see the module docstring."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = int(np.prod(shape))
    S = S if S > 0 else 1e-8
    m0 = rng.choice([-1.0, 1.0], n) * S * 10.0 ** rng.uniform(-2, 1, n)
    v0 = S * S * 10.0 ** rng.uniform(-4, 4, n)
    r = max(n // 8, 1)
    v0[:r] = 0.0
    m0[r:2 * r] = 0.0
    v0[r:2 * r] = 0.0
    v0[2 * r:3 * r] = 1e-30
    v0[-1] = 1e4 * S * S
    return m0.astype(np.float32).reshape(shape), v0.astype(np.float32).reshape(shape)


def _torch_adam(p0, lr):
    ps = {k: torch.nn.Parameter(torch.from_numpy(np.asarray(v, np.float64)).clone()) for k, v in p0.items()}
    return ps, torch.optim.Adam(list(ps.values()), lr=lr, betas=(B1, B2), eps=EPS, foreach=False)


def _torch_step(ps, opt, g):
    for k, p in ps.items():
        p.grad = torch.from_numpy(np.asarray(g[k], np.float64)).clone()
    opt.step()
    return ({k: p.detach().numpy().copy() for k, p in ps.items()},
            {k: opt.state[p]["exp_avg"].numpy().copy() for k, p in ps.items()},
            {k: opt.state[p]["exp_avg_sq"].numpy().copy() for k, p in ps.items()})


def _delta64(m1, v1, lr, t):
    return -(lr / (1.0 - B1 ** t)) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - B2 ** t) + EPS)


def _p_bound(p0, p1, m1, v1, m1r, v1r, dm, dv, lr, t):
    """The bound of |p1 - p1_ref| (module docstring), per element."""
    sb2 = np.sqrt(1.0 - B2 ** t)
    d, dr = np.sqrt(v1) / sb2 + EPS, np.sqrt(v1r) / sb2 + EPS
    s = np.sqrt(v1) + np.sqrt(v1r)
    ds = np.where(s > 0, dv / np.where(s > 0, s, 1.0), 0.0)
    return (8 * U * np.abs(_delta64(m1, v1, lr, t)) + 2.0 ** -23 * np.maximum(np.abs(p0), np.abs(p1))
            + (lr / (1.0 - B1 ** t)) * (dm / d + np.abs(m1r) * ds / (sb2 * d * dr)))


def _worst(err, bound):
    """(index, error, bound) of the element furthest past its bound."""
    i = int(np.argmax(err - bound))
    return i, float(err.flat[i]), float(bound.flat[i])


def _f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


@pytest.mark.parametrize("lr", [1e-4, 1e-2])
@pytest.mark.parametrize("steps0,fresh", [(0, True), (0, False), (1, False), (9, False), (999, False)])
def test_adam_one_step_from_state(lib, scale, steps0, fresh, lr):
    """fresh: the untouched trainer (m0 = v0 = 0, steps 0) instead of a written state."""
    tr = _trainer(lr)
    names = _params(tr)
    p0 = _f64(_read(tr, "value"))
    if fresh:
        m0 = {k: np.zeros_like(p0[k]) for k in names}
        v0 = {k: np.zeros_like(p0[k]) for k in names}
    else:
        m0, v0 = {}, {}
        for k in names:
            a, b = _moments(k, p0[k].shape, scale[k])
            tr.write_tensor(k, torch.from_numpy(a).cuda(), "exp_avg")
            tr.write_tensor(k, torch.from_numpy(b).cuda(), "exp_avg_sq")
            m0[k], v0[k] = a.astype(np.float64), b.astype(np.float64)
        _set_steps(tr, steps0)
        assert tr.steps == steps0
    _step(tr, tref.batch(N, T, 51))
    assert tr.steps == steps0 + 1
    g, p1, m1, v1 = (_f64(_read(tr, w)) for w in ("grad", "value", "exp_avg", "exp_avg_sq"))
    ps, opt = _torch_adam(p0, lr)
    if not fresh:
        for k, p in ps.items():
            opt.state[p] = {"step": torch.tensor(float(steps0)), "exp_avg": torch.from_numpy(m0[k]).clone(),
                            "exp_avg_sq": torch.from_numpy(v0[k]).clone()}
    p1r, m1r, v1r = _torch_step(ps, opt, g)
    t = steps0 + 1
    seen = 0
    for k in names:
        assert np.isfinite(p1[k]).all() and np.isfinite(m1[k]).all() and np.isfinite(v1[k]).all(), k
        if not fresh and scale[k] > 0:
            gs, ms = np.sign(g[k]), np.sign(m0[k])
            assert (gs * ms > 0).any() and (gs * ms < 0).any(), k          # both signs of m0 relative to g
            assert (v0[k] == 0).any() and v0[k].max() >= 0.99e4 * scale[k] ** 2, k
        dm = 4 * U * (np.abs(m0[k]) + np.abs(g[k]))
        dv = 4 * U * (v0[k] + g[k] ** 2)
        em, ev = np.abs(m1[k] - m1r[k]), np.abs(v1[k] - v1r[k])
        assert (em <= dm).all(), ("exp_avg", k) + _worst(em, dm)
        assert (ev <= dv).all(), ("exp_avg_sq", k) + _worst(ev, dv)
        d64 = _delta64(m1[k], v1[k], lr, t)
        ed = np.abs((p1[k] - p0[k]) - d64)
        bd = 8 * U * np.abs(d64) + 2.0 ** -23 * np.maximum(np.abs(p0[k]), np.abs(p1[k]))
        assert (ed <= bd).all(), ("update", k) + _worst(ed, bd)
        ep = np.abs(p1[k] - p1r[k])
        bp = _p_bound(p0[k], p1[k], m1[k], v1[k], m1r[k], v1r[k], dm, dv, lr, t)
        assert (ep <= bp).all(), ("value", k) + _worst(ep, bp)
        seen += p1[k].size
    assert seen == sum(int(np.prod(s)) for _, s, kind in tr._names if kind == 0)


def test_adam_carried_state_six_steps(lib):
    """One trainer, six steps, against one float64 torch.optim.Adam fed the GPU's
    gradient of each step: the counter advances by one per step, the moments
    persist, and each tensor's slice of the flat parameter, gradient, exp_avg
    and exp_avg_sq buffers lines up."""
    lr = 1e-3
    tr = _trainer(lr)
    names = _params(tr)
    p_prev = _f64(_read(tr, "value"))
    ps, opt = _torch_adam(p_prev, lr)
    mr_prev = {k: np.zeros_like(v) for k, v in p_prev.items()}
    vr_prev = {k: np.zeros_like(v) for k, v in p_prev.items()}
    top_m = {k: np.zeros_like(v) for k, v in p_prev.items()}
    top_v = {k: np.zeros_like(v) for k, v in p_prev.items()}
    top_p = {k: np.zeros_like(v) for k, v in p_prev.items()}
    for step in range(1, 7):
        _step(tr, tref.batch(N, T, 60 + step))
        assert tr.steps == step
        g, p, m, v = (_f64(_read(tr, w)) for w in ("grad", "value", "exp_avg", "exp_avg_sq"))
        pr, mr, vr = _torch_step(ps, opt, g)
        for k in names:
            top_m[k] = np.maximum(top_m[k], 4 * U * (np.abs(mr_prev[k]) + np.abs(g[k])))
            top_v[k] = np.maximum(top_v[k], 4 * U * (vr_prev[k] + g[k] ** 2))
            dm, dv = step * top_m[k], step * top_v[k]
            em, ev = np.abs(m[k] - mr[k]), np.abs(v[k] - vr[k])
            assert (em <= dm).all(), (step, "exp_avg", k) + _worst(em, dm)
            assert (ev <= dv).all(), (step, "exp_avg_sq", k) + _worst(ev, dv)
            # this step's update from the GPU's own moments: the one-step bound, nothing accumulates
            d64 = _delta64(m[k], v[k], lr, step)
            ed = np.abs((p[k] - p_prev[k]) - d64)
            bd = 8 * U * np.abs(d64) + 2.0 ** -23 * np.maximum(np.abs(p_prev[k]), np.abs(p[k]))
            assert (ed <= bd).all(), (step, "update", k) + _worst(ed, bd)
            top_p[k] = np.maximum(top_p[k], _p_bound(p_prev[k], p[k], m[k], v[k], mr[k], vr[k], dm, dv, lr, step))
            ep = np.abs(p[k] - pr[k])
            assert (ep <= step * top_p[k]).all(), (step, "value", k) + _worst(ep, step * top_p[k])
        p_prev, mr_prev, vr_prev = p, mr, vr
