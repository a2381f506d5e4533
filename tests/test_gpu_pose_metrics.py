"""tik_fk_pose_metrics / SMPLX.pose_metrics / inference.evaluate_poses (csrc/fk_metrics.hip: MPJPE, Procrustes-aligned
MPJPE, mean per-joint angle error and the weight sum of a frame in one launch) against the float64 reference of
tests/pose_metrics_ref.py, and bit for bit against itself.

The body is fk_jacobian_ref.small_consts(1, 1) (77 vertices); poses U(-0.3, 0.3), keypoints those of other random
poses, target poses the poses plus N(0, 0.1) and four constructed angles. The bounds on the positions are no new
constants: the project's per-entry FK tolerance R.TOL = 1e-4 on x gives sqrt(3) TOL on mpjpe (exact) and on the
reference's pa_mpjpe (tests/test_pose_metrics_host.py measures 0.94 of it on these frames), doubled for pa_mpjpe because
the kernel's rotation is itself rounded. mpjae has no project constant: MPJAE_BOUND is eight times the worst
|mpjae - ref| measured on the MI355X over the 65 frames (the constructed angles 0, 1e-3, pi/2, pi - 1e-3 included), 2.832e-8
rad (2.3e-8 at pi - 1e-3), and may never exceed 1e-4 rad. Each case prints its worst ratio to the bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import memedge as me
import pose_metrics_ref as P

pytestmark = pytest.mark.gpu
K, R = P.K, P.R
MPJAE_MEASURED = 2.832e-8
MPJAE_BOUND = 8 * MPJAE_MEASURED
assert MPJAE_BOUND <= 1e-4
COLS = ("mpjpe", "pa_mpjpe", "mpjae", "weight")


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def new_model(skin):
    me.lib()
    with me.env(TIK_FK_SKIN=skin):
        return R.SMPLX(K.consts(), batch_size=9)


@pytest.fixture(scope="module")
def models():
    """One handle per skinning table form for the whole module."""
    return {skin: new_model(skin) for skin in ("sparse", "dense")}


@pytest.fixture(scope="module")
def model(models):
    return models["sparse"]


@pytest.fixture(scope="module")
def dev65():
    th, betas, kps = K.inputs65()
    return cu(th), cu(betas), cu(kps), cu(P.targets65())


def wide(t, ld, fill=7.0):
    """t (B,66) as a view of a (B, ld) tensor whose padding columns hold `fill`."""
    w = torch.full((t.shape[0], ld), fill, device="cuda")
    w[:, :66] = t
    return w[:, :66]


def table(m):
    """The four columns as one (B,4) tensor (the views' common base)."""
    return torch.stack([m[c] for c in COLS], 1)


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("skin", ["sparse", "dense"])
@pytest.mark.parametrize("ld", [66, 68])
@pytest.mark.parametrize("weighted", [None, "shared", "frame"])
@pytest.mark.parametrize("shaped", [None, "shared", "frame"], ids=["mean_shape", "betas_shared", "betas_frame"])
def test_against_float64(models, dev65, shaped, weighted, ld, skin):
    t, b, k, tg = dev65
    w, ref = P.case65(shaped, weighted)
    m = models[skin]
    T = R.TOL
    bound = {"mpjpe": P.SQ3 * T, "pa_mpjpe": 2 * P.SQ3 * T, "mpjae": MPJAE_BOUND}
    worst = dict.fromkeys(("mpjpe", "pa_mpjpe", "mpjae", "joints"), 0.0)
    for B in (1, 3, 65):
        wB = None if w is None else (w if w.ndim == 1 else w[:B])
        bB = None if shaped is None else (b[0] if shaped == "shared" else b[:B])
        oj = torch.full((B, 17, 3), -3.0, device="cuda")
        got = m.pose_metrics(wide(t[:B], ld, float("nan")), k[:B], betas=bB, joint_weight=cu(wB),
                             target_poses=wide(tg[:B], ld, float("nan")), out_joints=oj)
        assert set(got) == set(COLS) | {"joints"} and got["joints"].data_ptr() == oj.data_ptr()
        base = got["mpjpe"]._base
        assert base.shape == (B, 4) and all(got[c].shape == (B,) and got[c]._base is base for c in COLS)
        for c in ("mpjpe", "pa_mpjpe", "mpjae"):
            g, r = got[c].cpu().numpy().astype(np.float64), ref[c][:B]
            assert np.array_equal(np.isnan(g), np.isnan(r)), (c, B, g, r)       # NaN exactly where the reference has it
            ok = ~np.isnan(r)
            if ok.any():
                e = np.abs(g[ok] - r[ok]).max()
                worst[c] = max(worst[c], float(e / bound[c]))
                assert e <= bound[c], (c, B, e, bound[c])
        wsum = np.ones((B, 17), np.float32) if wB is None else np.broadcast_to(wB, (B, 17))
        assert torch.equal(got["weight"].cpu(), butterfly_sum(wsum))            # exact: the kernel's own order of the sum
        # and against float64: 16 additions, each rounding a partial sum of at most 17 * 2 by at most 2^-24 of it
        assert np.abs(got["weight"].cpu().numpy() - ref["weight"][:B]).max() <= 16 * 34 * 2.0 ** -24
        ej = np.abs(oj.cpu().numpy() - ref["x"][:B]).max()
        worst["joints"] = max(worst["joints"], float(ej / T))
        assert ej <= T
    print(f"skin={skin} ld={ld} weights={weighted} betas={shaped}: worst error / bound: "
          + ", ".join(f"{c} {v:.2e}" for c, v in worst.items()))


def butterfly_sum(w):
    """(B,17) float32 -> (B,) the sum in wave_sum's order: 64 lanes (zeros past 17), lane l adds lane l ^ off, off = 32 .. 1."""
    v = np.zeros((w.shape[0], 64), np.float32)
    v[:, :17] = w
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ off]
    return torch.from_numpy(v[:, 0].copy())


def test_mpjae_measured(model, dev65):
    """The measurement MPJAE_BOUND comes from, printed: the worst |mpjae - ref| over the 65 frames, and the constructed
    angles on their own."""
    t, b, k, tg = dev65
    got = model.pose_metrics(t, k, target_poses=tg)["mpjae"].cpu().numpy().astype(np.float64)
    ref = P.mpjae(K.inputs65()[0], P.targets65())
    e = np.abs(got - ref)
    print(f"worst |mpjae - ref| = {e.max():.3e} rad over 65 frames; constructed angles {P.CONSTRUCTED}: {e[:4]}")
    assert got[0] == 0.0                                                        # a pose against itself: exactly zero
    assert e.max() <= MPJAE_BOUND


# ---------------------------------------------------------------- 2. bits
def full65(model, dev65, **kw):
    t, b, k, tg = dev65
    w = cu(P.weights65("frame"))
    oj = torch.empty(65, 17, 3, device="cuda")
    m = model.pose_metrics(t, k, betas=b, joint_weight=w, target_poses=tg, out_joints=oj, **kw)
    return table(m), oj, w


def same(a, b):
    """Bit for bit, NaN included."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_frame_bits_do_not_depend_on_the_batch(model, dev65):
    t, b, k, tg = dev65
    out, oj, w = full65(model, dev65)
    out2, oj2, _ = full65(model, dev65)
    assert same(out, out2) and same(oj, oj2)                                    # two identical calls
    for i in (0, 1, 63, 64):
        o1 = torch.empty(1, 17, 3, device="cuda")
        m1 = model.pose_metrics(t[i:i + 1], k[i:i + 1], betas=b[i:i + 1], joint_weight=w[i:i + 1], target_poses=tg[i:i + 1],
                                out_joints=o1)
        assert same(table(m1)[0], out[i]) and same(o1[0], oj[i]), i
    idx = torch.tensor([64, 5, 1], device="cuda")
    o3 = torch.empty(3, 17, 3, device="cuda")
    m3 = model.pose_metrics(t[idx], k[idx], betas=b[idx], joint_weight=w[idx], target_poses=tg[idx], out_joints=o3)
    assert same(table(m3), out[idx]) and same(o3, oj[idx])


def test_rows(model, dev65):
    t, b, k, tg = dev65
    out, oj, w = full65(model, dev65)
    sub = np.random.default_rng(2).permutation(65)[:23].astype(np.int32)
    rows = torch.from_numpy(sub).cuda()
    o, j = torch.full((65, 4), -3.0, device="cuda"), torch.full((65, 17, 3), -3.0, device="cuda")
    m = model.pose_metrics(t, k, betas=b, joint_weight=w, target_poses=tg, rows=rows, out=o, out_joints=j)
    assert m["mpjpe"]._base is o
    rest = torch.from_numpy(np.setdiff1d(np.arange(65), sub)).cuda()
    assert same(o[rows.long()], out[rows.long()]) and same(j[rows.long()], oj[rows.long()])
    assert (o[rest] == -3.0).all() and (j[rest] == -3.0).all()
    fresh = model.pose_metrics(t, k, betas=b, joint_weight=w, target_poses=tg, rows=rows)   # rows not listed: NaN
    assert same(table(fresh)[rows.long()], out[rows.long()]) and torch.isnan(table(fresh)[rest]).all()


def test_padding_columns_are_not_read(model, dev65):
    t, b, k, tg = dev65
    out, oj, w = full65(model, dev65)
    j = torch.empty(65, 17, 3, device="cuda")
    m = model.pose_metrics(wide(t, 68, float("nan")), k, betas=b, joint_weight=w, target_poses=wide(tg, 70, float("nan")),
                           out_joints=j)
    assert same(table(m), out) and same(j, oj)


def test_nan_pose(model, dev65):
    t, b, k, tg = dev65
    out, oj, w = full65(model, dev65)
    for col in (40, 0, 32):                                                     # a shoulder chain, the root, a foot
        tt = t.clone()
        tt[7, col] = float("nan")
        m = model.pose_metrics(tt, k, betas=b, joint_weight=w, target_poses=tg)
        got = table(m)
        assert torch.isnan(got[7]).all(), (col, got[7])
        keep = [i for i in range(65) if i != 7]
        assert same(got[keep], out[keep])
    tt = t.clone()
    tt[7, 40] = float("inf")
    assert torch.isnan(table(model.pose_metrics(tt, k, betas=b, joint_weight=w, target_poses=tg))[7]).all()
    m = model.pose_metrics(tt, k, betas=b, joint_weight=w)                      # without a target too
    assert torch.isnan(table(m)[7]).all()
    tn = tg.clone()
    tn[9, 3] = float("nan")                                                     # a NaN target: its mpjae alone
    got = table(model.pose_metrics(t, k, betas=b, joint_weight=w, target_poses=tn))
    assert torch.isnan(got[9, 2]) and same(got[9, [0, 1, 3]], out[9, [0, 1, 3]])
    keep = [i for i in range(65) if i != 9]
    assert same(got[keep], out[keep])


def test_skip_nonfinite(model, dev65):
    t, b, k, tg = dev65
    w = cu(P.weights65("frame"))
    kk, kz, wz = k.clone(), k.clone(), w.clone()
    kk[2, 7, 1] = float("nan")
    kk[3, 9] = float("inf")
    kz[2, 7] = 0.0
    kz[3, 9] = 0.0
    wz[2, 7] = 0.0
    wz[3, 9] = 0.0
    oa, ob = torch.empty(65, 17, 3, device="cuda"), torch.empty(65, 17, 3, device="cuda")
    a = model.pose_metrics(t, kk, betas=b, joint_weight=w, target_poses=tg, skip_nonfinite=True, out_joints=oa)
    z = model.pose_metrics(t, kz, betas=b, joint_weight=wz, target_poses=tg, out_joints=ob)
    assert same(table(a), table(z)) and same(oa, ob)
    assert torch.isfinite(table(a)[2:4]).all()
    # the flag off: a NaN component gives NaN in columns 0 and 1 (an Inf one Inf or NaN), the other two stay finite
    off = table(model.pose_metrics(t, kk, betas=b, joint_weight=w, target_poses=tg))
    assert torch.isnan(off[2, :2]).all() and not torch.isfinite(off[3, :2]).any() and torch.isfinite(off[2:4, 2:]).all()
    kh = k.clone()
    kh[5, 12, 0] = float("nan")                                                 # a NaN hip: the frame has no weight
    h = table(model.pose_metrics(t, kh, betas=b, joint_weight=w, target_poses=tg, skip_nonfinite=True))
    assert h[5, 3].item() == 0.0 and torch.isnan(h[5, :2]).all() and torch.isfinite(h[5, 2])
    keep = [i for i in range(65) if i != 5]
    assert same(h[keep], table(model.pose_metrics(t, k, betas=b, joint_weight=w, target_poses=tg))[keep])


def test_without_target(model, dev65):
    t, b, k, tg = dev65
    out, _, w = full65(model, dev65)
    got = table(model.pose_metrics(t, k, betas=b, joint_weight=w))
    assert torch.isnan(got[:, 2]).all() and same(got[:, [0, 1, 3]], out[:, [0, 1, 3]])


def test_mirrored_body(model, dev65):
    """The kernel's rotation is proper: against the mirror image of its own FK keypoints pa_mpjpe is the reference's
    best proper rotation's value, far from the reflection's zero."""
    t, b, k, tg = dev65
    x = P.xy_of(K.inputs65()[0], K.inputs65()[2])[0]
    km = P.mirrored(x).astype(np.float32)
    ref = P.point_metrics(x, P.mirrored(x))
    got = model.pose_metrics(t, cu(km))
    e = np.abs(got["pa_mpjpe"].cpu().numpy() - ref["pa_mpjpe"])
    assert (ref["pa_mpjpe"] > 1e-2).all() and e.max() <= 2 * P.SQ3 * R.TOL, e.max()


# ---------------------------------------------------------------- 3. across paths
def test_evaluate_poses_against_fk_check(model):
    from temporal_inverse_kinematics_amd.inference import evaluate_poses, fk_check
    th, betas, kps = K.inputs65()
    ev = evaluate_poses(th, kps, model, betas=betas[0], target_poses=P.targets65())
    fc = fk_check(th, kps, model, betas=betas[0])
    assert abs(ev["mpjpe_mean"] - fc["mean"]) <= P.SQ3 * R.TOL
    assert np.abs(ev["mpjpe"] - fc["mpjpe"]).max() <= P.SQ3 * R.TOL
    assert ev["weight"].tolist() == [17.0] * 65 and np.isfinite(ev["mpjae_mean"]) and np.isfinite(ev["pa_mpjpe_mean"])
    ref = P.reference(th, kps, betas[0], None, P.targets65())
    assert abs(ev["pa_mpjpe_mean"] - ref["pa_mpjpe"].mean()) <= 2 * P.SQ3 * R.TOL
    assert abs(ev["mpjae_mean"] - ref["mpjae"].mean()) <= MPJAE_BOUND


def test_evaluate_poses_accel_and_chunks(model, monkeypatch):
    from temporal_inverse_kinematics_amd import inference
    th, betas, kps = K.inputs65()
    th, kps = th[:12], kps[:12].copy()
    starts = np.array([0, 7, 12], np.int32)
    x, y = P.xy_of(th, kps)
    want = P.accel(x, y, starts)
    ev = inference.evaluate_poses(th, kps, model, seq_starts=starts)
    assert np.array_equal(np.isnan(ev["accel"]), np.isnan(want))
    ok = ~np.isnan(want)
    # four entries of x per term, each within TOL: 4 sqrt(3) TOL on every keypoint's norm and on their mean
    assert np.abs(ev["accel"][ok] - want[ok]).max() <= 4 * P.SQ3 * R.TOL
    assert abs(ev["accel_mean"] - want[ok].mean()) <= 4 * P.SQ3 * R.TOL
    monkeypatch.setattr(inference, "MAX_WINDOWS_PER_CALL", 5)                   # three launches: the same bytes
    ev5 = inference.evaluate_poses(th, kps, model, seq_starts=starts)
    for c in ("mpjpe", "pa_mpjpe", "weight", "accel"):
        assert np.array_equal(ev5[c], ev[c], equal_nan=True), c
    kps[4, 3] = np.nan                                                          # a missing keypoint: no NaN in the metrics
    kps[9, 11] = np.nan                                                         # a missing hip: the frame has no value
    evm = inference.evaluate_poses(th, kps, model, seq_starts=starts)
    assert evm["weight"][4] == 16.0 and np.isfinite(evm["mpjpe"][4]) and evm["weight"][9] == 0.0 and np.isnan(evm["mpjpe"][9])
    assert np.isfinite(evm["mpjpe_mean"]) and np.isfinite(evm["pa_mpjpe_mean"])


# ---------------------------------------------------------------- 4. refusals
def test_refusals(model, dev65):
    from temporal_inverse_kinematics_amd import _lib
    t, b, k, tg = dev65
    t, b, k, tg = t[:3], b[:3], k[:3], tg[:3]
    for kw in (dict(betas=torch.zeros(3, 9, device="cuda")), dict(joint_weight=torch.ones(3, 16, device="cuda")),
               dict(target_poses=torch.zeros(3, 65, device="cuda")), dict(out=torch.zeros(3, 3, device="cuda")),
               dict(out_joints=torch.zeros(3, 51, device="cuda")),
               dict(rows=torch.tensor([0, 0], dtype=torch.int32, device="cuda")),
               dict(rows=torch.tensor([0, 3], dtype=torch.int32, device="cuda")),
               dict(rows=torch.tensor([0, 1], device="cuda"))):
        with pytest.raises(ValueError):
            model.pose_metrics(t, k, **kw)
    with pytest.raises(TypeError):
        model.pose_metrics(t, k, betas=np.zeros(10, np.float32))
    lib = _lib.load()
    o, oj = torch.empty(3, 4, device="cuda"), torch.empty(3, 17, 3, device="cuda")
    ints = lambda v: (ctypes.c_int * len(v))(*v)

    def call(h=model._h, p=t.data_ptr(), pld=66, kp=k.data_ptr(), betas=None, bld=0, jw=None, jld=0, tp=tg.data_ptr(), tld=66,
             sel=None, B=3, flags=0, out=o.data_ptr(), joints=oj.data_ptr()):
        return lib.tik_fk_pose_metrics(h, p, pld, kp, betas, bld, jw, jld, tp, tld, sel, None, B, flags, out, joints, None)
    assert call(sel=ints(R.COCO[:16] + [55 + 21])) == _lib.TIK_E_INVALID and "three vertices" in _lib.last_error()
    for kw in (dict(h=None), dict(p=None), dict(kp=None), dict(out=None), dict(B=0), dict(B=-2), dict(pld=65), dict(tld=65),
               dict(betas=t.data_ptr(), bld=3), dict(jw=t.data_ptr(), jld=16), dict(flags=2), dict(flags=-1)):
        assert call(**kw) == _lib.TIK_E_INVALID, kw
    assert "flags" in _lib.last_error()
    assert call(tp=None, tld=0) == _lib.TIK_OK                 # target_ld is only checked with target_poses
    assert call(joints=None, flags=1) == _lib.TIK_OK and call(sel=ints(R.COCO)) == _lib.TIK_OK
    torch.cuda.synchronize()
