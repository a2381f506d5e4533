"""tik_fk_joints_jacobian / SMPLX.joints_jacobian against float64 central
differences of the numpy SMPL-X oracle (tests/fk_jacobian_ref.py) at the FK
tolerance of tests/test_gpu_fk.py (1e-4 absolute; entries are metres per
radian, bounded by the body's extent like the joints themselves), and bit for
bit against itself across batch sizes, positions and selections.

Every batch is cut from fk_inputs(65); the oracle Jacobian (all 55 dofs) is
taken once per checked body and shared. The kernel works one lane per body in
tiles of 64 with no exchange between lanes, so the bodies checked against the
oracle are the first two, one in the middle and the last three of the tile
edge (0, 1, 31, 62, 63, 64, those below B); test_bits_are_stable ties every
other position to these.

Measured on the MI355X: max |jac - oracle| = 2.9e-7 over all cases of
test_jacobian_vs_oracle and the dense-rows case (1.0e-7 .. 2.9e-7 per case),
2.1e-7 in test_small_angles (8.0e-8 for the body whose rotation vectors are
exactly zero); DESIGN.md "FK Jacobian". Each case prints its own figure.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fk_jacobian_ref as R
import memedge as me

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LMK = 55 + 21 + 7                              # a static landmark
SEL = R.COCO + [LMK, R.COCO[3]]                # COCO-17, a landmark, a duplicated index (column 3)
CHECKED = (0, 1, 31, 62, 63, 64)
DOFS = {
    "default": None,
    "root": [0],
    "all55": list(range(55)),
    "shuffled": [17, 3, 54, 0, 12, 21, 40, 9, 22, 15, 6],
}
_REF = {}


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_rows(bare, b):
    """The oracle Jacobian of body b of fk_inputs(65) for SEL and all 55 dofs, computed once."""
    if (bare, b) not in _REF:
        pose, betas, expr, transl = R.inputs65()
        extra = (None, None, None) if bare else (betas, expr, transl)
        j = R.oracle_jacobian(R.small_consts(), pose, *extra, sel=SEL, dof=range(55), bodies=[b])[0]
        j.setflags(write=False)
        _REF[(bare, b)] = j
    return _REF[(bare, b)]


def ref_for(bare, bodies, dof):
    cols = [3 * j + a for j in (range(22) if dof is None else dof) for a in range(3)]
    return np.stack([ref_rows(bare, b)[:, cols] for b in bodies])


def args65(bare, B, lo=0):
    pose, betas, expr, transl = R.inputs65()
    a = [pose] if bare else [pose, betas, expr, transl]
    return [cu(x[lo:lo + B]) for x in a]


@pytest.fixture(scope="module")
def model():
    me.lib()
    return R.SMPLX(R.small_consts(), batch_size=9)


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("bare", [False, True], ids=["shape_expr_transl", "pose_only"])
@pytest.mark.parametrize("dof", list(DOFS))
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_jacobian_vs_oracle(model, B, dof, bare):
    assert model.num_joints == R.NUM_STATIC
    jac, joints = model.joints_jacobian(*args65(bare, B), select=SEL, dof=DOFS[dof])
    nd = 22 if DOFS[dof] is None else len(DOFS[dof])
    assert jac.shape == (B, 3 * len(SEL), 3 * nd) and joints.shape == (B, len(SEL), 3)
    assert torch.isfinite(jac).all()
    bodies = [b for b in CHECKED if b < B]
    err = np.abs(jac[bodies].cpu().numpy() - ref_for(bare, bodies, DOFS[dof])).max()
    print(f"B={B} dof={dof} bare={bare}: max |jac - oracle| = {err:.3e}")
    assert err < R.TOL


def test_dense_weight_rows_vs_oracle():
    """TIK_FK_SKIN=dense: all 55 weights of a vertex from the dense rows (the kernel's other instantiation)."""
    me.lib()
    with me.env(TIK_FK_SKIN="dense"):
        m = R.SMPLX(R.small_consts(), batch_size=9)
    jac, _ = m.joints_jacobian(*args65(False, 65), select=SEL, dof=range(55))
    bodies = list(CHECKED)
    err = np.abs(jac[bodies].cpu().numpy() - ref_for(False, bodies, range(55))).max()
    print(f"dense rows: max |jac - oracle| = {err:.3e}")
    assert err < R.TOL


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
        m = R.SMPLX(c, batch_size=9)
    jac, _ = m.joints_jacobian(*args65(False, 65), select=SEL, dof=range(55))
    assert torch.isfinite(jac).all()
    bodies = [0, 63, 64]
    ref = R.oracle_jacobian(c, *R.inputs65(), sel=SEL, dof=range(55), bodies=bodies)
    err = np.abs(jac[bodies].cpu().numpy() - ref).max()
    print(f"nzmax={nzmax}: max |jac - oracle| = {err:.3e}")
    assert err < R.TOL


# ---------------------------------------------------------------- 2. structure
def test_structure(model):
    par = R.small_consts()["parents"]
    anc = {k: set() for k in range(55)}
    for k in range(55):
        p = int(par[k])
        while p >= 0:
            anc[k].add(p)
            p = int(par[p])
    jac, _ = model.joints_jacobian(*args65(False, 65), select=SEL, dof=range(55))
    J = jac.cpu().numpy().reshape(65, len(SEL), 3, 55, 3)
    seen = 0
    for s, k in enumerate(SEL):
        if k >= 55:
            continue
        for j in range(55):
            if j not in anc[k]:
                assert (J[:, s, :, j, :] == 0.0).all(), (k, j)
                seen += 1
            else:
                assert (J[:, s, :, j, :] != 0.0).any(), (k, j)
    assert seen > 0
    dup = len(SEL) - 1
    assert torch.equal(jac[:, 3 * dup:3 * dup + 3], jac[:, 9:12])


# ---------------------------------------------------------------- 3. small angles
def _small_angle_poses():
    pose = R.inputs65()[0][:4].copy()
    pose[0, :22] = 0.0
    pose[1, :22] = 1e-4
    pose[2, :22] = 1e-3
    d = np.array([1.0, 2.0, 2.0], np.float32) / 3.0
    pose[3, 3] = d * np.float32(np.pi - 1e-3)
    return pose


def test_small_angles(model):
    pose = _small_angle_poses()
    c = R.small_consts()
    # the hands of body 0 exactly -pose_mean: every one of its 55 rotations is of the exact zero vector
    pose[0] = -c["pose_mean"]
    _, betas, expr, transl = R.inputs65()
    ref = R.oracle_jacobian(c, pose, betas[:4], expr[:4], transl[:4], sel=SEL, dof=range(55))
    assert np.isfinite(ref).all()
    jac, _ = model.joints_jacobian(cu(pose), cu(betas[:4]), cu(expr[:4]), cu(transl[:4]), select=SEL, dof=range(55))
    assert torch.isfinite(jac).all()
    err = np.abs(jac.cpu().numpy() - ref).max(axis=(1, 2))
    print(f"small angles: max |jac - oracle| per body (0, 1e-4, 1e-3, pi - 1e-3) = {err}")
    assert err.max() < R.TOL


# ---------------------------------------------------------------- 4. each term is visible
def test_each_term_is_visible(model):
    c = R.small_consts()
    pose, betas, expr, transl = [x[:1] for x in R.inputs65()]
    face = [SEL.index(j) for j in R.FACE]
    rows = [3 * s + k for s in face for k in range(3)]
    full = ref_for(False, [0], None)[0][rows]
    # on the CPU, from the oracle alone: each term moves the reference by more than 10 x the bound
    z = dict(c)
    z["posedirs"] = np.zeros_like(c["posedirs"])
    no_pd = R.oracle_jacobian(z, pose, betas, expr, transl, sel=R.FACE)[0]
    w = c["lbs_weights"]
    w1 = np.zeros_like(w)
    w1[np.arange(len(w)), w.argmax(1)] = 1.0
    z = dict(c)
    z["lbs_weights"] = w1
    one_w = R.oracle_jacobian(z, pose, betas, expr, transl, sel=R.FACE)[0]
    d_pd, d_w = np.abs(no_pd - full).max(), np.abs(one_w - full).max()
    print(f"reference moves by {d_pd:.3e} without posedirs, {d_w:.3e} with one skinning weight per vertex")
    assert d_pd > 10 * R.TOL and d_w > 10 * R.TOL
    jac, _ = model.joints_jacobian(*args65(False, 1), select=SEL)
    assert np.abs(jac[0].cpu().numpy()[rows] - full).max() < R.TOL


# ---------------------------------------------------------------- 5. stability of bits
def test_bits_are_stable(model):
    big, _ = model.joints_jacobian(*args65(False, 65), select=SEL)
    one, _ = model.joints_jacobian(*args65(False, 1), select=SEL)
    assert torch.equal(one[0], big[0])
    last, _ = model.joints_jacobian(*args65(False, 1, lo=64), select=SEL)
    assert torch.equal(last[0], big[64])
    a = args65(False, 65)
    swapped = [torch.cat([x[64:65], x[1:64], x[0:1]]).contiguous() for x in a]
    sw, _ = model.joints_jacobian(*swapped, select=SEL)
    assert torch.equal(sw[64], big[0]) and torch.equal(sw[0], big[64]) and torch.equal(sw[1:64], big[1:64])
    longer = [3, 60] + SEL + [100, 0, 126]
    lg, _ = model.joints_jacobian(*a, select=longer)
    assert torch.equal(lg[:, 6:6 + 3 * len(SEL)], big)


# ---------------------------------------------------------------- 6. returned joints
@pytest.mark.parametrize("sel", ["coco", [0, 12, 7], SEL])
def test_returned_joints_are_joints(model, sel):
    a = args65(False, 65)
    _, j = model.joints_jacobian(*a, select=sel, dof=[0, 5])
    assert torch.equal(j, model.joints(*a, select=sel))
    jac, none = model.joints_jacobian(*a, select=sel, dof=[0, 5], return_joints=False)
    assert none is None
    assert torch.equal(jac, model.joints_jacobian(*a, select=sel, dof=[0, 5])[0])


# ---------------------------------------------------------------- 7. workspace
def test_workspace_is_the_documented_budget():
    me.lib()
    m = R.SMPLX(R.small_consts(), batch_size=9)
    assert m.workspace_bytes == 0
    B = 65
    m.joints_jacobian(*args65(False, B), select="coco")
    torch.cuda.synchronize()
    assert m.workspace_bytes == 4 * R.WS_FLOATS * B
    m.joints_jacobian(*args65(False, 3), select=SEL, dof=range(55))
    assert m.workspace_bytes == 4 * R.WS_FLOATS * B


def test_profile_labels():
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    m = R.SMPLX(R.small_consts(), batch_size=9)
    _lib.check(L.tik_fk_profile(m._h, 8))
    m.joints_jacobian(*args65(False, 3), select="coco", return_joints=False)
    m.joints_jacobian(*args65(False, 3), select="coco")
    torch.cuda.synchronize()
    labels = []
    for i in range(_lib.check(L.tik_fk_profile_count(m._h))):
        buf = _lib.ctypes.create_string_buffer(64)
        _lib.check(L.tik_fk_profile_read(m._h, i, buf, 64, None, None, None))
        labels.append(buf.value.decode())
    assert labels == ["fk_chain", "fk_jacobian", "fk_chain", "fk_joints", "fk_jacobian"]


# ---------------------------------------------------------------- errors
def test_rejected_arguments(model):
    from temporal_inverse_kinematics_amd import _lib
    pose = args65(True, 3)[0]
    full = R.SMPLX(me.fk_consts(), batch_size=9)          # with face contours: joints 127..143
    with pytest.raises(ValueError, match="contour"):
        full.joints_jacobian(pose, select=[0, 127])
    for kw in ({"select": None}, {"select": [200]}, {"dof": [0, 0]}, {"dof": [55]}, {"dof": []}, {"dof": list(range(56))}):
        with pytest.raises(ValueError):
            model.joints_jacobian(pose, **kw)
    L = _lib.load()
    ints = lambda v: None if v is None else (_lib.ctypes.c_int * len(v))(*v)
    jac = torch.empty((3, 3 * 257, 3 * 55), device="cuda")

    def call(h=full._h, sel=(0,), n=None, dof=None, nd=0, B=3, p=pose.data_ptr(), o=jac.data_ptr()):
        ns = (len(sel) if sel else 0) if n is None else n
        return L.tik_fk_joints_jacobian(h, p, 0, 0, 0, B, ints(sel), ns, ints(dof), nd, o, 0, 0)
    assert call(sel=[0, 127]) == _lib.TIK_E_INVALID and "contour" in _lib.last_error()
    assert call(sel=None) == _lib.TIK_E_INVALID
    assert call(sel=[144]) == _lib.TIK_E_INVALID
    assert call(sel=[0] * 257) == _lib.TIK_E_INVALID
    assert call(sel=[0], n=0) == _lib.TIK_E_INVALID
    assert call(B=0) == _lib.TIK_E_INVALID
    assert call(p=0) == _lib.TIK_E_INVALID
    assert call(o=0) == _lib.TIK_E_INVALID
    assert call(h=None) == _lib.TIK_E_INVALID
    assert call(dof=[0, 0], nd=2) == _lib.TIK_E_INVALID
    assert call(dof=[55], nd=1) == _lib.TIK_E_INVALID
    assert call(dof=[0], nd=0) == _lib.TIK_E_INVALID
    assert call(dof=[0] * 56, nd=56) == _lib.TIK_E_INVALID
    assert call(sel=[126, 0]) == _lib.TIK_OK               # the last static landmark
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 8. guards and poison
def test_no_guard_zone_written_and_no_poison_read():
    import fk_jacobian_guard_child as child
    me.lib()
    env = dict(os.environ)
    env.update(TIK_GUARD="1", TIK_POISON="ff")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fk_jacobian_guard_child.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = {d["family"]: d for d in (json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{"))}
    assert p.returncode == 0, (p.returncode, lines, p.stderr[-3000:])
    assert sorted(lines) == sorted(child.FAMILY_NAMES)
    for name, r in lines.items():
        assert r["checks"] > 0 and r["bad"] == 0 and r["nan"] == 0, (name, r)
