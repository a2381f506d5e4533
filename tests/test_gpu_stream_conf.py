"""Confidences per push in an online stream (tik_stream_push_conf, OnlineIK.push(frame, conf)) against the batch call of
the same kernel, bit for bit. The set-up is tests/test_gpu_stream_refine.py's: synthetic_model(win_size=9), the first 24
golden frames, 2 iterations, the 77-vertex body, both steps and both ways to run the step.

The pattern: keypoint 9 NaN with confidence 0 in frames 5..7, keypoint 11 with confidence 0 in frame 12 (a missing hip:
the whole frame weighs 0), frame 15 all NaN with every confidence 0, 0.5 on some finite keypoints elsewhere, one NaN
keypoint with positive confidence; frame 0 is complete. `filled` is lm_robust_ref.hold_last of it and `eff` its
effective_weights: the network must see `filled`, and every refined pose must be SMPLX.refine_frames of (the network's
pose, filled, joint_weight=eff) exactly.
"""
import numpy as np
import pytest
import torch

import lm_refine_ref as L
import lm_robust_ref as RR
import memedge as me

pytestmark = pytest.mark.gpu
CASES = [(True, "1"), (False, "1"), (True, "0")]   # (use_graph, TIK_ONLINE)
WIN, FRAMES, ITERS = 9, 24, 2
KW = dict(iters=ITERS, mu=1e-2, lam0=1e-2)


def cu(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


@pytest.fixture(scope="module")
def seq():
    return np.ascontiguousarray(me.golden("run_inference.npz")["seq"][:FRAMES], dtype=np.float32)


@pytest.fixture(scope="module")
def body():
    me.lib()
    return L.R.SMPLX(L.consts(), batch_size=9)


@pytest.fixture(scope="module")
def pattern(seq):
    """-> frames with the holes (24,17,3), conf (24,17), filled, the confidences after the fill."""
    frames, conf = seq.copy(), np.ones((FRAMES, 17), np.float32)
    frames[5:8, 9], conf[5:8, 9] = np.nan, 0
    conf[12, 11] = 0
    frames[15], conf[15] = np.nan, 0
    conf[3, [0, 5, 12]] = 0.5
    conf[18:21, 7] = 0.5
    conf[20, 11] = 0.25
    frames[22, 14, 1] = np.nan            # not finite with confidence one: counts as 0
    filled, cf = RR.hold_last(frames, conf)
    assert np.isfinite(filled).all() and not np.array_equal(filled, seq) and cf[22, 14] == 0 and (cf[15] == 0).all()
    return frames, conf, filled, cf


@pytest.mark.parametrize("graph,online", CASES)
def test_conf_stream_is_the_batch_kernel(seq, body, pattern, graph, online):
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    frames, conf, filled, cf = pattern
    eff = RR.effective_weights(cf)
    assert (eff[12] == 0).all() and (eff[15] == 0).all() and eff[6, 9] == 0 and eff[6, 8] == 1
    with me.env(TIK_ONLINE=online):
        m = synthetic_model(win_size=WIN, device="cuda")
        base = OnlineIK(m, use_graph=graph).run(filled)
        assert np.isfinite(base).all()
        # a stream without refinement: the fill only
        assert np.array_equal(OnlineIK(m, use_graph=graph).run(frames, conf), base)

        def stream(**kw):
            return OnlineIK(m, use_graph=graph, refine=ITERS, smplx_model=body, **kw)

        # raw and refined poses, push by push
        s = stream()
        s.reset()
        got, raw = [], []
        for i in list(range(FRAMES)) + [FRAMES - 1] * s.h:
            p = s.push(frames[i], conf[i])
            if p is not None:
                got.append(p)
                raw.append(s.raw)
        got, raw = np.stack(got), np.stack(raw)
        assert np.array_equal(raw, base)
        want, _ = body.refine_frames(cu(base), cu(filled), joint_weight=cu(eff), **KW)
        assert np.array_equal(got, want.cpu().numpy())
        assert np.array_equal(got[12], base[12]) and np.array_equal(got[15], base[15])   # all weights 0, no tie: the start
        assert np.array_equal(s.run(frames, conf), got)          # run and flush: the last frame with its confidences

        # joint weights times confidences, one fp32 multiply
        w = np.linspace(0.5, 1.5, 17).astype(np.float32)
        u = stream(joint_weight=w).run(frames, conf)
        want, _ = body.refine_frames(cu(base), cu(filled), joint_weight=cu(RR.effective_weights(cf, w)), **KW)
        assert np.array_equal(u, want.cpu().numpy())

        # the causal tie and the robust term: the sequential chain of batch calls
        for extra, ctor in ((dict(smooth=0.1), dict(smooth_weight=0.1)),
                            (dict(smooth=0.1, robust_sigma=RR.SIGMA), dict(smooth_weight=0.1, robust_sigma=RR.SIGMA)),
                            (dict(robust_sigma=RR.SIGMA), dict(robust_sigma=RR.SIGMA))):
            t = stream(**ctor).run(frames, conf)
            chain, prev = [], None
            for c in range(FRAMES):
                prev, _ = body.refine_frames(cu(base[c:c + 1]), cu(filled[c:c + 1]), prev=prev, joint_weight=cu(eff[c:c + 1]),
                                             **extra, **KW)
                chain.append(prev.cpu().numpy()[0])
            assert np.array_equal(t, np.stack(chain)), extra
            assert not np.array_equal(t, got)

        # a plain push on a stream that has a confidence ring: the bytes of a stream built before it existed
        plain_base = OnlineIK(m, use_graph=graph).run(seq)
        want, _ = body.refine_frames(cu(plain_base), cu(seq), **KW)
        assert np.array_equal(stream().run(seq), want.cpu().numpy())
        assert np.array_equal(stream().run(seq, np.ones((FRAMES, 17), np.float32)), want.cpu().numpy())
        # and mixed with confidence pushes on one stream: a plain push is a push with ones
        mixed = stream()
        mixed.reset()
        out = []
        for i in list(range(FRAMES)) + [FRAMES - 1] * mixed.h:
            p = mixed.push(frames[i]) if (conf[i] == 1).all() and np.isfinite(frames[i]).all() else mixed.push(frames[i], conf[i])
            if p is not None:
                out.append(p)
        assert np.array_equal(np.stack(out), got)


def test_refusals_leave_the_stream_untouched(seq, body, pattern):
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    frames, conf, _, _ = pattern
    me.lib()
    lib = _lib.load()
    m = synthetic_model(win_size=WIN, device="cuda")
    want = OnlineIK(m, refine=ITERS, smplx_model=body).run(frames, conf)
    s = OnlineIK(m, refine=ITERS, smplx_model=body)
    s.reset()
    hole, c0 = frames[0].copy(), np.ones(17, np.float32)
    hole[3] = np.nan
    c0[6] = 0
    for f, c in ((hole, np.ones(17, np.float32)), (frames[0], c0)):       # never seen: a NaN keypoint, a confidence 0
        with pytest.raises(ValueError, match="not been seen"):
            s.push(f, c)
    bad = np.ones(17, np.float32)
    bad[2] = -0.5
    pose = np.zeros(66, np.float32)
    out = []
    for i in list(range(FRAMES)) + [FRAMES - 1] * s.h:
        if i == 10:
            with pytest.raises(ValueError):
                s.push(frames[i], bad)                                    # refused in Python
            for v in (-0.5, float("nan")):                                # and by the library itself
                bad[2] = v
                rc = lib.tik_stream_push_conf(s._s, frames[i].ctypes.data_as(_lib._F), bad.ctypes.data_as(_lib._F),
                                              pose.ctypes.data_as(_lib._F))
                assert rc == _lib.TIK_E_INVALID and "confidence 2" in _lib.last_error()
            with pytest.raises(ValueError):
                s.push(np.full((17, 3), np.nan, np.float32))              # a plain push refuses a NaN as ever
        p = s.push(frames[i], conf[i])
        if p is not None:
            out.append(p)
    assert np.array_equal(np.stack(out), want)
    s.reset()                                                             # reset clears what was seen
    with pytest.raises(ValueError, match="not been seen"):
        s.push(hole, np.ones(17, np.float32))
    for bad_sigma in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            OnlineIK(m, refine=ITERS, smplx_model=body, robust_sigma=bad_sigma)
        assert lib.tik_stream_set_robust(s._s, bad_sigma) == _lib.TIK_E_INVALID
    with pytest.raises(ValueError):
        OnlineIK(m, robust_sigma=0.1)                                     # no refinement to make robust
    assert np.array_equal(s.run(frames, conf), want)                      # the refused settings changed nothing


def test_conf_ring_across_the_count_wrap(body, pattern):
    """The confidence ring uses the keypoint ring's index rule, the 2^30 wrap of stream_next_count included: a stream
    moved to just below the wrap gives the bytes of one that never wrapped."""
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    frames, conf = (np.concatenate([x, x]) for x in pattern[:2])          # the pattern twice: 48 frames
    me.lib()
    m = synthetic_model(win_size=WIN, device="cuda")
    a, b = (OnlineIK(m, refine=ITERS, smplx_model=body, smooth_weight=0.1) for _ in range(2))
    a.reset()
    b.reset()
    # past the left-edge clamp (more than 2 h frames) before the count moves; 2^30 = 10 modulo 2 W = 18, so from 25
    # pushes the count can go to 2^30 - 3
    n0 = 25
    for i in range(n0):
        pa, pb = a.push(frames[i], conf[i]), b.push(frames[i], conf[i])
        assert (pa is None and pb is None) or np.array_equal(pa, pb)
    W = 2 * b.h + 1
    start = n0 + 2 * W * (((1 << 30) - 1 - n0) // (2 * W))
    assert W == 9 and start == (1 << 30) - 3
    _lib.check(_lib.load().tik_debug_stream_set_count(b._s, start))
    # the third push from here wraps: confidences with holes (frames 22, 29..31, 36, 39) are stored and read below the
    # wrap, across it and after it
    for i in list(range(n0, 2 * FRAMES)) + [2 * FRAMES - 1] * b.h:
        pa, pb = a.push(frames[i], conf[i]), b.push(frames[i], conf[i])
        assert np.array_equal(pa, pb), i
