"""tik_fk_keypoint_loss / SMPLX.keypoint_loss (csrc/fk_kploss.hip: the keypoint loss of a pose and its pose gradient
in one launch) against the float64 reference of tests/kp_loss_ref.py, and bit for bit against itself.

The body is fk_jacobian_ref.small_consts(1, 1) (77 vertices); poses U(-0.3, 0.3), keypoints those of other random
poses. The bounds are no new constants: they follow from the project's per-entry FK tolerance R.TOL = 1e-4 on r and
on J (kp_loss_ref.bounds). Each case prints its worst ratio to the bound.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import kp_loss_ref as K
import memedge as me

pytestmark = pytest.mark.gpu
R = K.R


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def new_model(skin):
    me.lib()
    with me.env(TIK_FK_SKIN=skin):
        return R.SMPLX(K.consts(), batch_size=9)


@pytest.fixture(scope="module")
def model():
    return new_model("sparse")


@pytest.fixture(scope="module")
def dev65():
    th, betas, kps = K.inputs65()
    return cu(th), cu(betas), cu(kps)


def wide(t, ld):
    """t (B,66) as a view of a (B, ld) tensor filled with a sentinel."""
    w = torch.full((t.shape[0], ld), 7.0, device="cuda")
    w[:, :66] = t
    return w[:, :66]


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("skin", ["sparse", "dense"])
@pytest.mark.parametrize("ld", [66, 68])
@pytest.mark.parametrize("weighted", [None, "shared", "frame"])
@pytest.mark.parametrize("shaped", [True, False], ids=["betas", "mean_shape"])
def test_against_float64(dev65, shaped, weighted, ld, skin):
    t, b, k = dev65
    w, ref = K.case65(shaped, weighted)
    lb, gb = K.bounds(ref)
    m = new_model(skin)
    worst = [0.0, 0.0]
    for B in (1, 3, 65):
        wB = None if w is None else (w if w.ndim == 1 else w[:B])
        og = wide(torch.zeros(B, 66, device="cuda"), ld)
        loss, grad = m.keypoint_loss(wide(t[:B], ld), k[:B], betas=b[:B] if shaped else None, joint_weight=cu(wB), out_grad=og)
        assert grad.data_ptr() == og.data_ptr() and loss.shape == (B,) and grad.shape == (B, 66)
        el = np.abs(loss.cpu().numpy() - ref["loss"][:B])
        eg = np.abs(grad.cpu().numpy() - ref["g"][:B])
        pos = lb[:B] > 0                                       # a frame with no weight has a zero bound: exact
        if pos.any():
            worst[0] = max(worst[0], float((el[pos] / lb[:B][pos]).max()))
            worst[1] = max(worst[1], float((eg[pos] / gb[:B][pos]).max()))
        assert (el <= lb[:B]).all(), (B, el, lb[:B])
        assert (eg <= gb[:B]).all(), (B, eg.max())
        if ld > 66:
            assert (og._base[:, 66:] == 7.0).all()             # the padding columns are not written
    if weighted == "frame":                                     # a frame with no weight: exactly zero
        assert loss[0].item() == 0.0 and (grad[0] == 0).all()
    print(f"skin={skin} ld={ld} weights={weighted} shaped={shaped}: worst |loss - loss64| / bound = {worst[0]:.2e}, "
          f"worst |g - g64| / bound = {worst[1]:.2e}")


def test_one_betas_row_for_all_frames(model, dev65):
    """betas_ld = 0 against the same row repeated (betas_ld = nb): the same bits, and the float64 bound."""
    t, b, k = dev65
    shared = model.keypoint_loss(t[:3], k[:3], betas=b[0])
    rows = model.keypoint_loss(t[:3], k[:3], betas=b[0:1].expand(3, -1).contiguous())
    assert torch.equal(shared[0], rows[0]) and torch.equal(shared[1], rows[1])
    th, betas, kps = K.inputs65()
    ref = K.reference(th[:3], kps[:3], betas[0])
    lb, gb = K.bounds(ref)
    assert (np.abs(shared[0].cpu().numpy() - ref["loss"]) <= lb).all()
    assert (np.abs(shared[1].cpu().numpy() - ref["g"]) <= gb).all()


# ---------------------------------------------------------------- 2. rows and bits
def test_rows_and_bits(model, dev65):
    t, b, k = dev65
    w = cu(K.weights65("frame"))
    loss, grad = model.keypoint_loss(t, k, betas=b, joint_weight=w)
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all()
    # a frame's bits at B = 1 and 3, at any place in the batch
    for i in (0, 1, 63, 64):
        l1, g1 = model.keypoint_loss(t[i:i + 1], k[i:i + 1], betas=b[i:i + 1], joint_weight=w[i:i + 1])
        assert torch.equal(l1[0], loss[i]) and torch.equal(g1[0], grad[i]), i
    idx = torch.tensor([64, 5, 1], device="cuda")
    l3, g3 = model.keypoint_loss(t[idx], k[idx], betas=b[idx], joint_weight=w[idx])
    assert torch.equal(l3, loss[idx]) and torch.equal(g3, grad[idx])
    # a permuted strict subset: the listed frames get the full call's bits, the others keep a sentinel
    sub = np.random.default_rng(2).permutation(65)[:23].astype(np.int32)
    rows = torch.from_numpy(sub).cuda()
    ol, og = torch.full((65,), -3.0, device="cuda"), torch.full((65, 66), -3.0, device="cuda")
    model.keypoint_loss(t, k, betas=b, joint_weight=w, rows=rows, out_loss=ol, out_grad=og)
    rest = np.setdiff1d(np.arange(65), sub)
    assert torch.equal(ol[rows.long()], loss[rows.long()]) and torch.equal(og[rows.long()], grad[rows.long()])
    assert (ol[rest] == -3.0).all() and (og[rest] == -3.0).all()
    # loss only and gradient only (the C entry point: the Python method always asks for both)
    from temporal_inverse_kinematics_amd import _lib
    lib = _lib.load()
    lo, go = torch.full((65,), -3.0, device="cuda"), torch.full((65, 66), -3.0, device="cuda")
    args = (model._h, t.data_ptr(), 66, k.data_ptr(), b.data_ptr(), 10, w.data_ptr(), 17, None, None, 65)
    assert lib.tik_fk_keypoint_loss(*args, lo.data_ptr(), None, 0, 1.0, 0, None) == 0
    assert lib.tik_fk_keypoint_loss(*args, None, go.data_ptr(), 66, 1.0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(lo, loss) and torch.equal(go, grad)


def test_accumulate_and_scale(model, dev65):
    t, b, k = dev65
    _, g = model.keypoint_loss(t, k, betas=b)
    prev = torch.from_numpy(np.random.default_rng(4).normal(0, 1, (65, 66)).astype(np.float32)).cuda()
    s = 0.37
    acc = prev.clone()
    model.keypoint_loss(t, k, betas=b, out_grad=acc, grad_scale=s, accumulate=True)
    # fmaf(s, g, prev) rounds the exact value once: in exact rational arithmetic, no float32 neighbour of the result is closer
    got, gh, ph = acc.cpu().numpy(), g.cpu().numpy(), prev.cpu().numpy()
    sf = Fraction(float(np.float32(s)))
    for x, gv, pv in zip(got.ravel(), gh.ravel(), ph.ravel()):
        e = sf * Fraction(float(gv)) + Fraction(float(pv))
        d = abs(Fraction(float(x)) - e)
        for nb in (np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))):
            assert d <= abs(Fraction(float(nb)) - e), (x, gv, pv)
    _, scaled = model.keypoint_loss(t, k, betas=b, grad_scale=s)
    assert torch.equal(scaled, g * np.float32(s))
    keep = prev.clone()
    model.keypoint_loss(t, k, betas=b, out_grad=keep, grad_scale=0.0, accumulate=True)
    assert torch.equal(keep, prev)


def test_nan_frame(model, dev65):
    t, b, k = dev65
    clean = model.keypoint_loss(t[:3], k[:3], betas=b[:3])
    for what in ("keypoint", "pose"):
        tt, kk = t[:3].clone(), k[:3].clone()
        if what == "keypoint":
            kk[1, 7, 1] = float("nan")
        else:
            tt[1, 40] = float("nan")
        loss, grad = model.keypoint_loss(tt, kk, betas=b[:3])
        torch.cuda.synchronize()
        assert torch.isnan(loss[1]) and torch.isnan(grad[1]).all(), what
        for i in (0, 2):
            assert torch.equal(loss[i], clean[0][i]) and torch.equal(grad[i], clean[1][i]), (what, i)


def test_autograd(model, dev65):
    t, b, k = dev65
    loss, grad = model.keypoint_loss(t[:3], k[:3], betas=b[:3])
    p = t[:3].clone().requires_grad_(True)
    fn = model.keypoint_loss_fn(k[:3], betas=b[:3])
    out = fn(p)
    assert torch.equal(out, loss)
    out.sum().backward()
    assert torch.equal(p.grad, grad)
    p.grad = None
    fn(p).mean().backward()
    assert torch.allclose(p.grad, grad / 3, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- 3. refusals
def test_refusals(model, dev65):
    from temporal_inverse_kinematics_amd import _lib
    t, b, k = dev65
    t, b, k = t[:3], b[:3], k[:3]
    for kw in (dict(betas=torch.zeros(3, 9, device="cuda")), dict(joint_weight=torch.ones(3, 16, device="cuda")),
               dict(sel17=R.COCO[:16] + [55 + 21]), dict(sel17=R.COCO[:16]), dict(grad_scale=float("nan")),
               dict(out_grad=torch.zeros(3, 65, device="cuda")), dict(out_loss=torch.zeros(2, device="cuda")),
               dict(rows=torch.tensor([0, 0], dtype=torch.int32, device="cuda")),
               dict(rows=torch.tensor([0, 3], dtype=torch.int32, device="cuda")),
               dict(rows=torch.tensor([0, 1], device="cuda"))):
        with pytest.raises(ValueError):
            model.keypoint_loss(t, k, **kw)
    with pytest.raises(ValueError):
        model.keypoint_loss(t, k.reshape(3, 51))
    with pytest.raises(ValueError):
        model.keypoint_loss(cu(np.zeros((66, 3))).t(), k)
    # the C entry point itself
    lib = _lib.load()
    lo, go = torch.empty(3, device="cuda"), torch.empty(3, 66, device="cuda")
    ints = lambda v: (ctypes.c_int * len(v))(*v)

    def call(h=model._h, p=t.data_ptr(), pld=66, kp=k.data_ptr(), betas=None, bld=0, jw=None, jld=0, sel=None, B=3,
             loss=lo.data_ptr(), grad=go.data_ptr(), gld=66, scale=1.0):
        return lib.tik_fk_keypoint_loss(h, p, pld, kp, betas, bld, jw, jld, sel, None, B, loss, grad, gld, scale, 0, None)
    assert call(sel=ints(R.COCO[:16] + [55 + 21])) == _lib.TIK_E_INVALID and "three vertices" in _lib.last_error()
    assert call(sel=ints(R.COCO[:16] + [500])) == _lib.TIK_E_INVALID
    for kw in (dict(h=None), dict(p=None), dict(kp=None), dict(loss=None, grad=None), dict(B=0), dict(B=-2), dict(pld=65),
               dict(gld=65), dict(scale=float("nan")), dict(scale=float("inf")), dict(betas=t.data_ptr(), bld=3),
               dict(jw=t.data_ptr(), jld=16)):
        assert call(**kw) == _lib.TIK_E_INVALID, kw
    assert call(gld=0, grad=None) == _lib.TIK_OK               # grad_ld is only checked with grad
    assert call(sel=ints(R.COCO)) == _lib.TIK_OK and call() == _lib.TIK_OK
    torch.cuda.synchronize()
