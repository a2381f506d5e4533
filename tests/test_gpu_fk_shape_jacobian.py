"""tik_fk_joints_shape_jacobian / SMPLX.joints_shape_jacobian against the float64
oracle (tests/fk_shape_ref.py: joints(e_i) - joints(0), exact because the
joints are affine in the betas) at the FK tolerance of tests/test_gpu_fk.py
(1e-4 absolute; entries are metres per unit beta and reach 0.036), and bit
for bit against itself across batch sizes, positions, selections and the
shape / expression / translation inputs, which must not enter.

Every batch is cut from fk_inputs(65); the oracle rows are taken once per
checked body and shared. The kernel works one lane per body in tiles of 64
with no exchange between lanes, so the bodies checked against the oracle are
0, 1, 31, 62, 63, 64 (those below B); test_bits_are_stable ties every other
position to these.

Measured on the MI355X: max |jac - oracle| = 8.2e-9 over all cases of
test_shape_jacobian_vs_oracle and the dense-rows case (7.3e-9 at B = 1);
DESIGN.md "Shape Jacobian and sequence solve". Each case prints its own figure.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fk_jacobian_ref as R
import fk_shape_ref as S
import memedge as me

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LMK = 55 + 21 + 7                              # a static landmark
SEL = R.COCO + [LMK, R.COCO[3]]                # COCO-17, a landmark, a duplicated index (column 3)
CHECKED = (0, 1, 31, 62, 63, 64)
NB = 10
_REF = {}


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_rows(b):
    """The oracle shape Jacobian of body b of fk_inputs(65) for SEL, computed once."""
    if b not in _REF:
        j = S.oracle_shape_jacobian(R.small_consts(), R.inputs65()[0], SEL, bodies=[b])[0]
        j.setflags(write=False)
        _REF[b] = j
    return _REF[b]


def args65(bare, B, lo=0):
    pose, betas, expr, transl = R.inputs65()
    a = [pose] if bare else [pose, betas, expr, transl]
    return [cu(x[lo:lo + B]) for x in a]


@pytest.fixture(scope="module")
def model():
    me.lib()
    return S.SMPLX(R.small_consts(), batch_size=9)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("bare", [False, True], ids=["shape_expr_transl", "pose_only"])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_shape_jacobian_vs_oracle(model, B, bare):
    assert model.num_joints == R.NUM_STATIC and model.num_betas == NB
    jac, joints = model.joints_shape_jacobian(*args65(bare, B), select=SEL)
    assert jac.shape == (B, 3 * len(SEL), NB) and joints.shape == (B, len(SEL), 3)
    assert torch.isfinite(jac).all()
    bodies = [b for b in CHECKED if b < B]
    ref = np.stack([ref_rows(b) for b in bodies])
    err = np.abs(jac[bodies].cpu().numpy() - ref).max()
    print(f"B={B} bare={bare}: max |jac - oracle| = {err:.3e} (largest entry {np.abs(ref).max():.3e})")
    assert err < S.TOL


def test_the_oracle_is_affine_in_the_betas():
    """On the CPU: the oracle's difference does not depend on where it is taken (what makes it exact)."""
    c = R.small_consts()
    pose, betas, expr, transl = R.inputs65()
    at = S.oracle_shape_jacobian(c, pose, SEL, bodies=[1], betas=betas, expr=expr, transl=transl)[0]
    assert np.abs(at - ref_rows(1)).max() < 1e-13


def test_dense_weight_rows_vs_oracle():
    """TIK_FK_SKIN=dense: all 55 weights of a vertex from the dense rows (the kernel's other branch)."""
    me.lib()
    with me.env(TIK_FK_SKIN="dense"):
        m = S.SMPLX(R.small_consts(), batch_size=9)
    jac, _ = m.joints_shape_jacobian(*args65(False, 65), select=SEL)
    bodies = list(CHECKED)
    err = np.abs(jac[bodies].cpu().numpy() - np.stack([ref_rows(b) for b in bodies])).max()
    print(f"dense rows: max |jac - oracle| = {err:.3e}")
    assert err < S.TOL


@pytest.mark.parametrize("nzmax", [4, 12, 20])
def test_weight_layouts(nzmax):
    """The weights of tests/test_gpu_fk_joints.py::test_weight_layouts on the small constants: 4 and 16 pairs per
    vertex and more than 16 live joints (no pairs: the dense WT rows). One full tile plus one body, 19 columns (a
    partial last workgroup of the 4-wave kernel); bodies 0, 63, 64 against the oracle on the same weights."""
    import fkref
    me.lib()
    c = dict(R.small_consts())
    c["lbs_weights"] = fkref._nz_weights(c["v_template"].shape[0], nzmax)
    lo, hi = {4: (1, 4), 12: (9, 16), 20: (17, 55)}[nzmax]   # live joints of the fullest vertex: 4 pairs, 16 pairs, none
    assert lo <= int(fkref.live_counts(c).max()) <= hi
    with me.env(TIK_FK_SKIN="sparse"):
        m = S.SMPLX(c, batch_size=9)
    jac, _ = m.joints_shape_jacobian(*args65(False, 65), select=SEL)
    assert torch.isfinite(jac).all()
    bodies = [0, 63, 64]
    ref = S.oracle_shape_jacobian(c, R.inputs65()[0], SEL, bodies=bodies)
    err = np.abs(jac[bodies].cpu().numpy() - ref).max()
    print(f"nzmax={nzmax}: max |jac - oracle| = {err:.3e}")
    assert err < S.TOL


# ---------------------------------------------------------------- 2. each term is visible
def test_each_term_is_visible(model):
    c = R.small_consts()
    pose = R.inputs65()[0][:3]
    vrows = [3 * s + k for s, j in enumerate(SEL) if j >= 55 for k in range(3)]
    crows = [3 * s + k for s, j in enumerate(SEL) if j < 55 for k in range(3)]
    full = np.stack([ref_rows(b) for b in range(3)])
    # on the CPU, from the oracle alone, before the GPU call: the term-by-term formula is the oracle, and
    # each term moves it by more than 10 x the bound
    assert np.abs(S.formula_shape_jacobian(c, pose, SEL) - full).max() < 1e-13
    for drop, rows in (("sd", vrows), ("rjd", vrows), ("dp", vrows), ("one_w", vrows), ("jd_chain", crows)):
        d = np.abs(S.formula_shape_jacobian(c, pose, SEL, drop=drop)[:, rows] - full[:, rows]).max()
        print(f"reference moves by {d:.3e} with drop={drop}")
        assert d > 10 * S.TOL, drop
    jac, _ = model.joints_shape_jacobian(*args65(False, 3), select=SEL)
    assert np.abs(jac.cpu().numpy() - full).max() < S.TOL


# ---------------------------------------------------------------- 3. stability of bits
def test_bits_are_stable(model):
    big, _ = model.joints_shape_jacobian(*args65(False, 65), select=SEL)
    one, _ = model.joints_shape_jacobian(*args65(False, 1), select=SEL)
    assert torch.equal(one[0], big[0])
    last, _ = model.joints_shape_jacobian(*args65(False, 1, lo=64), select=SEL)
    assert torch.equal(last[0], big[64])
    a = args65(False, 65)
    swapped = [torch.cat([x[64:65], x[1:64], x[0:1]]).contiguous() for x in a]
    sw, _ = model.joints_shape_jacobian(*swapped, select=SEL)
    assert torch.equal(sw[64], big[0]) and torch.equal(sw[0], big[64]) and torch.equal(sw[1:64], big[1:64])
    longer = [3, 60] + SEL + [100, 0, 126]
    lg, _ = model.joints_shape_jacobian(*a, select=longer)
    assert torch.equal(lg[:, 6:6 + 3 * len(SEL)], big)
    # betas, expression and translation do not enter
    bare, _ = model.joints_shape_jacobian(*args65(True, 65), select=SEL)
    assert torch.equal(bare, big)
    dup = len(SEL) - 1
    assert torch.equal(big[:, 3 * dup:3 * dup + 3], big[:, 9:12])


# ---------------------------------------------------------------- 4. returned joints
@pytest.mark.parametrize("sel", ["coco", [0, 12, 7], SEL])
def test_returned_joints_are_joints(model, sel):
    a = args65(False, 65)
    jac, j = model.joints_shape_jacobian(*a, select=sel)
    assert torch.equal(j, model.joints(*a, select=sel))
    again, none = model.joints_shape_jacobian(*a, select=sel, return_joints=False)
    assert none is None
    assert torch.equal(again, jac)


# ---------------------------------------------------------------- 5. bookkeeping
def test_workspace_is_the_documented_budget():
    me.lib()
    m = S.SMPLX(R.small_consts(), batch_size=9)
    assert m.workspace_bytes == 0
    B = 65
    per_body = S.WS_FLOATS_FIXED + S.WS_FLOATS_PER_BETA * NB
    m.joints_shape_jacobian(*args65(False, B), select="coco")
    torch.cuda.synchronize()
    assert m.workspace_bytes == 4 * per_body * B
    m.joints_shape_jacobian(*args65(False, 3), select=SEL)
    assert m.workspace_bytes == 4 * per_body * B


def test_profile_labels():
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    m = S.SMPLX(R.small_consts(), batch_size=9)
    _lib.check(L.tik_fk_profile(m._h, 8))
    m.joints_shape_jacobian(*args65(False, 3), select="coco", return_joints=False)
    m.joints_shape_jacobian(*args65(False, 3), select="coco")
    torch.cuda.synchronize()
    labels = []
    for i in range(_lib.check(L.tik_fk_profile_count(m._h))):
        buf = _lib.ctypes.create_string_buffer(64)
        _lib.check(L.tik_fk_profile_read(m._h, i, buf, 64, None, None, None))
        labels.append(buf.value.decode())
    assert labels == ["fk_chain", "fk_shape_jacobian", "fk_chain", "fk_joints", "fk_shape_jacobian"]


def test_rejected_arguments(model):
    from temporal_inverse_kinematics_amd import _lib
    pose = args65(True, 3)[0]
    full = S.SMPLX(me.fk_consts(), batch_size=9)          # with face contours: joints 127..143
    with pytest.raises(ValueError, match="contour"):
        full.joints_shape_jacobian(pose, select=[0, 127])
    for kw in ({"select": None}, {"select": [200]}, {"select": []}, {"select": [0] * 257}, {"select": "body25"}):
        with pytest.raises(ValueError):
            model.joints_shape_jacobian(pose, **kw)
    L = _lib.load()
    ints = lambda v: None if v is None else (_lib.ctypes.c_int * len(v))(*v)
    jac = torch.empty((3, 3 * 257, NB), device="cuda")

    def call(h=full._h, sel=(0,), n=None, B=3, p=pose.data_ptr(), o=jac.data_ptr()):
        ns = (len(sel) if sel else 0) if n is None else n
        return L.tik_fk_joints_shape_jacobian(h, p, 0, 0, 0, B, ints(sel), ns, o, 0, 0)
    assert call(sel=[0, 127]) == _lib.TIK_E_INVALID and "contour" in _lib.last_error()
    assert call(sel=None) == _lib.TIK_E_INVALID
    assert call(sel=[144]) == _lib.TIK_E_INVALID
    assert call(sel=[-1]) == _lib.TIK_E_INVALID
    assert call(sel=[0] * 257) == _lib.TIK_E_INVALID
    assert call(sel=[0], n=0) == _lib.TIK_E_INVALID
    assert call(B=0) == _lib.TIK_E_INVALID
    assert call(p=0) == _lib.TIK_E_INVALID
    assert call(o=0) == _lib.TIK_E_INVALID
    assert call(h=None) == _lib.TIK_E_INVALID
    assert call(sel=[126, 0]) == _lib.TIK_OK               # the last static landmark
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. guards and poison
def test_no_guard_zone_written_and_no_poison_read():
    import fk_shape_guard_child as child
    me.lib()
    env = dict(os.environ)
    env.update(TIK_GUARD="1", TIK_POISON="ff")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fk_shape_guard_child.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = {d["family"]: d for d in (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))}
    assert p.returncode == 0, (p.returncode, lines, p.stderr[-3000:])
    assert sorted(lines) == sorted(child.FAMILY_NAMES)
    for name, r in lines.items():
        assert r["checks"] > 0 and r["bad"] == 0 and r["nan"] == 0, (name, r)
