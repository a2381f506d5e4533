"""tik_lm_solve_chain / smplx_fk.lm_solve_chain: the block-tridiagonal system
    D_f delta_f - smooth delta_{f-1} - smooth delta_{f+1} = b_f      (include/tik.h)
of whole sequences, one workgroup per sequence.

The inputs follow tests/test_gpu_lm_solve.py::system: normal J, r, prior and
theta, mu = 0.25, lambda = top / 2e3 + 0.05 per sequence (top: the largest
eigenvalue of J^T W J over its frames), row weights per frame uniform in
(0.2, 2) with one zero column, and frame 1 of every sequence of 3 or more
frames with all weights zero (a frame that only its neighbours determine).

The reference is numpy.linalg.solve of the dense (L n)^2 system in float64 on
the same fp32 inputs; its condition number is asserted below 1e4. The allowed
error is measured, not fixed: 4 x the larger of two float32 numpy errors against
that float64 solution, plus 1e-6 - (a) the float32 dense solve, (b) a float32
block Thomas in this file (the kernel's recurrences with numpy's cholesky, inv
and M.T @ M). The factor 4 is test_gpu_lm_solve.py's and covers a different
summation order; the dense yardstick alone is not enough, an explicit inverse
per frame loses more than one dense LU does ((b) / (a) reached 4.2 on the CPU).
Each case prints its ratio (kernel error / the larger float32 numpy error).
Measured on the MI355X: 0.15 .. 3.11 over the 40 cases, the largest (2.63, 3.11)
at (3,96), smooth = 30, 2 and 3 frames (|gpu - f64| = 1.0e-4, 6.5e-5); (b) / (a)
is 0.41 .. 4.50 on the same cases; condition numbers 1 .. 694. DESIGN.md "LM
chain solve".
"""
import functools

import numpy as np
import pytest
import torch

import memedge as me
from temporal_inverse_kinematics_amd.smplx_fk import LM_CHAIN_MAX_N, lm_chain_workspace_floats, lm_solve, lm_solve_chain

pytestmark = pytest.mark.gpu
SHAPES = [(51, 66), (1, 1), (3, 96), (51, 7)]
LENGTHS = [(1,), (2,), (3,), (17,), (1, 2, 3, 17)]
MIXED = (1, 2, 3, 17)
MU = 0.25
MARGIN = 64


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()   # the shared inputs are read only


@functools.lru_cache(maxsize=None)
def chain_system(lengths, m, n, seed=0):
    """Random fp32 inputs (read only: shared by the tests) -> dict."""
    rng = np.random.default_rng(1000 * m + n + 7 * sum(lengths) + len(lengths) + seed)
    F = sum(lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    J = rng.normal(0, 1, (F, m, n)).astype(np.float32)
    r = rng.normal(0, 1, (F, m)).astype(np.float32)
    p = rng.normal(0, 1, (F, n)).astype(np.float32)
    th = rng.normal(0, 1, (F, n)).astype(np.float32)
    w = rng.uniform(0.2, 2.0, (F, m)).astype(np.float32)
    w[:, m // 2] = 0.0                      # a zero column
    for a, L in zip(starts[:-1], lengths):
        if L >= 3:
            w[a + 1] = 0.0                  # a frame nobody observed
    top = np.array([np.linalg.eigvalsh((J[f].astype(np.float64).T * w[f].astype(np.float64)) @ J[f].astype(np.float64))[-1]
                    for f in range(F)])
    lam = np.array([top[a:b].max() / 2e3 + 0.05 for a, b in zip(starts[:-1], starts[1:])], np.float32)
    out = dict(J=J, r=r, p=p, th=th, w=w, lam=lam, starts=starts, F=F, m=m, n=n)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def blocks(s, smooth, dt):
    """Per sequence the list of (D_f, b_f) in dtype dt."""
    out = []
    n, mu, sm = s["n"], dt(MU), dt(smooth)
    for q, (a, b) in enumerate(zip(s["starts"][:-1], s["starts"][1:])):
        seq = []
        for f in range(a, b):
            c = dt(int(f > a) + int(f + 1 < b))   # int: numpy bools add as "or"
            Jf, W, th = s["J"][f].astype(dt), s["w"][f].astype(dt), s["th"].astype(dt)
            D = (Jf.T * W) @ Jf + ((mu + dt(s["lam"][q])) + sm * c) * np.eye(n, dtype=dt)
            t = c * th[f] - (th[f - 1] if f > a else 0) - (th[f + 1] if f + 1 < b else 0)
            g = (Jf.T * W) @ s["r"][f].astype(dt) + mu * s["p"][f].astype(dt) + sm * t
            seq.append((D, -g))
        out.append(seq)
    return out


def dense_solve(s, smooth, dt):
    """-> (delta (F,n) in dt, the largest float64 condition number)."""
    n, out, conds = s["n"], [], []
    for seq in blocks(s, smooth, dt):
        L = len(seq)
        A, rhs = np.zeros((L * n, L * n), dt), np.zeros(L * n, dt)
        for k, (D, b) in enumerate(seq):
            A[k * n:(k + 1) * n, k * n:(k + 1) * n] = D
            rhs[k * n:(k + 1) * n] = b
            if k:
                A[k * n:(k + 1) * n, (k - 1) * n:k * n] = -dt(smooth) * np.eye(n, dtype=dt)
                A[(k - 1) * n:k * n, k * n:(k + 1) * n] = -dt(smooth) * np.eye(n, dtype=dt)
        out.append(np.linalg.solve(A, rhs).reshape(L, n))
        ev = np.linalg.eigvalsh(A.astype(np.float64))
        conds.append(ev[-1] / ev[0])
    return np.concatenate(out), max(conds)


def thomas32(s, smooth):
    """The kernel's recurrences in float32 numpy."""
    f32, out = np.float32, []
    sm = f32(smooth)
    for seq in blocks(s, smooth, f32):
        inv, xs, Sinv, x = [], [], None, None
        for k, (D, b) in enumerate(seq):
            Sf = D if k == 0 else D - sm * sm * Sinv
            y = b if k == 0 else b + sm * x
            M = np.linalg.inv(np.linalg.cholesky(Sf)).astype(f32)
            Sinv = (M.T @ M).astype(f32)
            x = (Sinv @ y).astype(f32)
            inv.append(Sinv)
            xs.append(x)
        d = [None] * len(seq)
        d[-1] = xs[-1]
        for k in range(len(seq) - 2, -1, -1):
            d[k] = (xs[k] + sm * (inv[k] @ d[k + 1])).astype(f32)
        out.append(np.stack(d))
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def reference(lengths, m, n, smooth):
    s = chain_system(lengths, m, n)
    ref, cond = dense_solve(s, smooth, np.float64)
    e_dense = np.abs(dense_solve(s, smooth, np.float32)[0].astype(np.float64) - ref).max()
    e_thomas = np.abs(thomas32(s, smooth).astype(np.float64) - ref).max()
    return ref, cond, e_dense, e_thomas


def gpu(s, smooth, mu=MU, lam=None, J=None, w="frame", starts=None, sl=slice(None), prior=True, workspace=None):
    """lm_solve_chain on the frames sl of s (w: "frame" = (F,m), "shared" = row 0 for all, None)."""
    wt = {"frame": s["w"][sl], "shared": s["w"][0], None: None}[w]
    J = s["J"] if J is None else J
    lam = s["lam"] if lam is None else lam
    return lm_solve_chain(cu(J[sl]), cu(s["r"][sl]), cu(lam), cu(s["th"][sl]), smooth, mu=mu,
                          prior=cu(s["p"][sl]) if prior else None, row_weight=cu(wt),
                          seq_starts=s["starts"] if starts is None else starts, workspace=workspace)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    me.lib()


@pytest.mark.parametrize("smooth", [0.3, 30.0])
@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda v: "L" + "_".join(map(str, v)))
@pytest.mark.parametrize("m,n", SHAPES)
def test_chain_vs_float64(m, n, lengths, smooth):
    s = chain_system(lengths, m, n)
    ref, cond, e_dense, e_thomas = reference(lengths, m, n, smooth)
    assert cond < 1e4, cond
    got = gpu(s, smooth).cpu().numpy()
    assert got.shape == (s["F"], n) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    e32 = max(e_dense, e_thomas)
    print(f"(m,n)=({m},{n}) lengths={lengths} smooth={smooth}: cond={cond:.1f} |gpu-f64|={err:.3e} "
          f"|dense32-f64|={e_dense:.3e} |thomas32-f64|={e_thomas:.3e} thomas/dense={e_thomas / max(e_dense, 1e-30):.2f} "
          f"ratio={err / max(e32, 1e-30):.2f}")
    assert err <= 4 * e32 + 1e-6


@pytest.mark.parametrize("m,n", [(51, 66), (3, 96)])
def test_inert_at_the_edges_bit_for_bit(m, n):
    """smooth = 0 at any length, and smooth = 30 with every sequence one frame long: lm_solve's bits."""
    s = chain_system(MIXED, m, n)
    seg = np.repeat(np.arange(len(MIXED)), MIXED)
    per_frame = lm_solve(cu(s["J"]), cu(s["r"]), cu(s["lam"][seg]), MU, cu(s["p"]), cu(s["w"][0]))
    assert torch.equal(gpu(s, 0.0, w="shared"), per_frame)
    plain = lm_solve(cu(s["J"]), cu(s["r"]), cu(s["lam"][seg]), MU, None, None)
    assert torch.equal(gpu(s, 0.0, w=None, prior=False), plain)
    no_theta = lm_solve_chain(cu(s["J"]), cu(s["r"]), cu(s["lam"]), None, 0.0, mu=MU, prior=cu(s["p"]),
                              row_weight=cu(s["w"][0]), seq_starts=s["starts"])
    assert torch.equal(no_theta, per_frame)
    singles = np.arange(s["F"] + 1, dtype=np.int32)
    assert torch.equal(gpu(s, 30.0, lam=s["lam"][seg], w="shared", starts=singles), per_frame)
    # per-frame weights, one frame per sequence: each frame against lm_solve with its own weight row
    each = gpu(s, 30.0, lam=s["lam"][seg], starts=singles)
    for f in (0, 2, s["F"] - 1):
        one = lm_solve(cu(s["J"][f:f + 1]), cu(s["r"][f:f + 1]), cu(s["lam"][seg][f:f + 1]), MU, cu(s["p"][f:f + 1]), cu(s["w"][f]))
        assert torch.equal(each[f], one[0])


@pytest.mark.parametrize("smooth", [0.3, 30.0])
def test_bits_do_not_depend_on_the_launch(smooth):
    s = chain_system(MIXED, 51, 66)
    big = gpu(s, smooth)
    for q, (a, b) in enumerate(zip(s["starts"][:-1], s["starts"][1:])):
        one = gpu(s, smooth, lam=s["lam"][q:q + 1], sl=slice(a, b), starts=np.array([0, b - a], np.int32))
        assert torch.equal(one, big[a:b]), q
    assert torch.equal(gpu(s, smooth), big)


@pytest.mark.parametrize("m,n,frame,lam_bad", [(51, 66, 5, -1.0), (51, 7, 16, -0.5), (51, 7, 0, -1.0)])
def test_a_matrix_that_is_not_positive_gives_nan_for_that_sequence_only(m, n, frame, lam_bad):
    """J = 0 at one frame of the 17-frame sequence, mu = 0, lambda = -1 for that sequence: D_f =
    (-1 + smooth c_f) I < 0 at smooth = 0.3. The second case fails at the end of the forward sweep
    only: at (51,7) J^T W J is positive definite by itself, with lambda = -0.5 the unobserved frame 1
    keeps (-0.5 + 0.6) I, and the last frame (one neighbour, J = 0) has D = -0.2 I. An arithmetic
    outcome: the call returns normally."""
    s = chain_system(MIXED, m, n)
    clean = gpu(s, 0.3, mu=0.0)
    assert torch.isfinite(clean[:6]).all()
    J2, lam2 = s["J"].copy(), s["lam"].copy()
    J2[6 + frame] = 0.0
    lam2[3] = lam_bad
    got = gpu(s, 0.3, mu=0.0, lam=lam2, J=J2)
    torch.cuda.synchronize()
    assert torch.isnan(got[6:]).all()
    assert torch.equal(got[:6], clean[:6])


def raw_call(L, t, smooth_, starts_d, dims, ws_t, delta_t, **kw):
    """tik_lm_solve_chain on the device tensors t; kw replaces single arguments (0: a null pointer)."""
    a = dict(jac=t["J"].data_ptr(), r=t["r"].data_ptr(), prior=t["p"].data_ptr(), theta=t["th"].data_ptr(),
             row_w=t["w"].data_ptr(), stride=dims[2], lam=t["lam"].data_ptr(), starts=starts_d.data_ptr(), mu=MU,
             smooth=smooth_, S=dims[0], F=dims[1], m=dims[2], n=dims[3], ws=ws_t.data_ptr(), delta=delta_t.data_ptr())
    a.update(kw)
    return L.tik_lm_solve_chain(a["jac"], a["r"], a["prior"], a["theta"], a["row_w"], a["stride"], a["lam"], a["starts"],
                                a["mu"], a["smooth"], a["F"], a["S"], a["m"], a["n"], a["ws"], a["delta"], 0)


def device_inputs(s):
    return {k: cu(s[k]) for k in ("J", "r", "p", "th", "w", "lam")}


def carve(count, fill):
    """A (count,) view with MARGIN sentinel floats on both sides -> (whole buffer, view)."""
    whole = torch.full((count + 2 * MARGIN,), 7.5, device="cuda")
    view = whole[MARGIN:MARGIN + count]
    view.fill_(fill)
    return whole, view


def margins_intact(whole):
    return bool((whole[:MARGIN] == 7.5).all()) and bool((whole[-MARGIN:] == 7.5).all())


def test_memory_margins_and_nothing_read_before_it_is_written():
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    m, n = 51, 66
    big, small = chain_system((20, 9), m, n), chain_system(MIXED, m, n)
    # buffers sized for the larger call, used by it first: the smaller one runs behind its rows
    cap_ws, cap_d = lm_chain_workspace_floats(big["F"], n), big["F"] * n
    results = []
    for fill in (float("nan"), 0.0):
        ws_whole, ws = carve(cap_ws, fill)
        d_whole, d = carve(cap_d, fill)
        out = {}
        for name, s in (("big", big), ("small", small)):
            t, S, F = device_inputs(s), len(s["starts"]) - 1, s["F"]
            ws.fill_(fill)
            d.fill_(fill)
            d_view = d[:F * n]
            assert raw_call(L, t, 0.3, cu(s["starts"]), (S, F, m, n), ws, d_view) == _lib.TIK_OK
            torch.cuda.synchronize()
            assert margins_intact(ws_whole) and margins_intact(d_whole), (name, fill)
            used = lm_chain_workspace_floats(F, n)
            rest_ws, rest_d = ws[used:], d[F * n:]
            same = torch.isnan if fill != fill else (lambda v: v == fill)
            assert bool(same(rest_ws).all()) and bool(same(rest_d).all()), (name, fill)   # nothing past the call's own rows
            out[name] = d_view.clone().reshape(F, n)
            assert torch.isfinite(out[name]).all(), (name, fill)
        results.append(out)
    for name in ("big", "small"):
        assert torch.equal(results[0][name], results[1][name]), name
    assert torch.equal(results[0]["small"], gpu(small, 0.3))


def test_rejected_arguments():
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    m, n = 5, 4
    s = chain_system((2, 3), m, n)
    F, S = s["F"], 2
    t = device_inputs(s)
    starts_d = cu(s["starts"])
    ws = torch.empty(lm_chain_workspace_floats(F, n), device="cuda")
    d = torch.empty((F, n), device="cuda")

    def call(**kw):
        return raw_call(L, t, 0.3, starts_d, (S, F, m, n), ws, d, **kw)
    nan = float("nan")
    for kw in ({"jac": 0}, {"r": 0}, {"lam": 0}, {"starts": 0}, {"ws": 0}, {"delta": 0}, {"theta": 0}, {"F": 0}, {"F": -1},
               {"S": 0}, {"S": F + 1}, {"n": 0}, {"n": 97}, {"m": 0}, {"m": 769}, {"mu": -1.0}, {"mu": nan},
               {"smooth": -0.5}, {"smooth": nan}, {"stride": 1}, {"stride": m + 1}, {"stride": -m}):
        assert call(**kw) == _lib.TIK_E_INVALID, kw
        assert "tik_lm_solve_chain" in _lib.last_error()
    assert call() == _lib.TIK_OK
    assert call(prior=0, row_w=0, stride=0) == _lib.TIK_OK          # the optional pointers
    assert call(theta=0, smooth=0.0) == _lib.TIK_OK                 # theta may be null with smooth == 0
    torch.cuda.synchronize()
    assert L.tik_lm_chain_workspace_floats(F, n) == F * (n * (n + 1) // 2 + n) == ws.numel()
    assert L.tik_lm_chain_workspace_floats(4096, 96) == 4096 * (96 * 97 // 2 + 96)
    assert LM_CHAIN_MAX_N == 96

    J, r, lam, th = t["J"], t["r"], t["lam"], t["th"]
    bad = [dict(smooth=-1.0), dict(smooth=nan), dict(mu=-1.0), dict(theta=None), dict(theta=th[:, :3].contiguous()),
           dict(r=r[:, :3].contiguous()), dict(lam=lam[:1]), dict(prior=th[:2]), dict(row_weight=t["w"][:2]),
           dict(row_weight=t["w"][0, :3]), dict(seq_starts=[0, 2]), dict(seq_starts=[1, 2, F]), dict(seq_starts=[0, 2, 2, F]),
           dict(seq_starts=[0, 3, 2, F]), dict(seq_starts=[]), dict(seq_starts=np.array([0.0, 2.0, F])),
           dict(workspace=ws[:-1]), dict(jac=J.double()), dict(jac=torch.zeros((F, m, 97), device="cuda")),
           dict(seq_starts=starts_d.long())]
    for kw in bad:
        a = dict(jac=J, r=r, lam=lam, theta=th, smooth=0.3, seq_starts=s["starts"])
        a.update(kw)
        with pytest.raises(ValueError):
            lm_solve_chain(**a)


@pytest.mark.parametrize("starts,S", [((0, 5 + 5), 1), ((3, 1), 1), ((0, 9, 2), 2), ((-4, 2, 5), 2)])
def test_sequence_bounds_outside_the_frames_do_no_work(starts, S):
    """Through the raw C call (the wrapper refuses these): delta and the margins stay as they were."""
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    m, n = 5, 4
    s = chain_system((2, 3), m, n)
    F = s["F"]
    assert F == 5
    t = device_inputs(s)
    ws_whole, ws = carve(lm_chain_workspace_floats(F, n), 0.0)
    d_whole, d = carve(F * n, -3.25)
    valid = [(a, b) for a, b in zip(starts[:-1], starts[1:]) if 0 <= a < b <= F]
    assert raw_call(L, t, 0.3, cu(np.array(starts, np.int32)), (S, F, m, n), ws, d) == _lib.TIK_OK
    torch.cuda.synchronize()
    assert margins_intact(ws_whole) and margins_intact(d_whole)
    touched = torch.zeros(F, dtype=torch.bool)
    for a, b in valid:
        touched[a:b] = True
    rows = d.reshape(F, n).cpu()
    assert bool((rows[~touched] == -3.25).all())
    assert len(valid) == 0 or bool((rows[touched] != -3.25).any())
