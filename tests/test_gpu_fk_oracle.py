"""tik_fk_forward and tik_fk_joints against the float64 SMPL-X oracle at the float32
oracle's own noise (tests/fkref.py): per output group (vertices, chain joints 0..54,
joints 55..143), max|got - f64| <= MARGIN * max(max|f32 - f64|, 2^-23 max|f64|) on
the case itself, MARGIN = 4. The bar comes from the reference alone; what it passes
and what it fails is shown on the host in tests/test_fk_oracle_host.py (a P matrix at
two bf16 planes or one dropped bf16x3 product of the blend measures 11 to 20 units and
passed the fixed 1e-4 of tests/test_gpu_fk.py by a factor of 18).

Handles: sparse (bf16x3, the sparse skinning kernels), dense (bf16x3, TIK_FK_SKIN=dense:
the skinning GEMM), fp32 (both GEMMs exact fp32 MFMA), chunk4 (TIK_FK_CHUNK=4: the
two-stream chunk pipeline at test sizes; B = 9 is three chunks, the third on the first
v_posed buffer). Constants and inputs: fkref.consts / fkref.inputs. V = 777 is three
256-vertex tiles, the last ragged, and 3V = 2331 is no multiple of the 128-column GEMM
tile; the full V = 10475 runs where it is listed only (the float64 oracle costs seconds
there).

Worst ratio per path and group, measured on the MI355X (every case prints its own):

    path, V                          vertices  joints 0..54  joints 55..143
    tik_fk_forward sparse, 777         1.76        1.78          1.68
    tik_fk_forward dense, 777          1.76        1.78          1.68
    tik_fk_forward chunk4, 777         1.76        1.78          1.68
    tik_fk_forward fp32, 777           1.76        1.78          1.76
    tik_fk_forward sparse, 10475       1.24        0.98          0.91
    tik_fk_forward fp32, 10475         1.24        0.98          1.06
    tik_fk_joints bf16x3 handle, 777     -         1.16          1.36
    tik_fk_joints fp32 handle, 777       -         1.16          1.36

The worst vertices and chain joints are std, random, B = 9 on every handle (the chain kernel
is shared); the worst joints 55..143 blend_heavy, random, B = 129 (fp32: std, B = 5); the
joints path's blend_heavy at B = 193 and 65. Nothing comes near MARGIN: the second float32 evaluation of the host test
measures up to 1.82 on the same cases.
"""
import numpy as np
import pytest
import torch

import fkref as fr
import memedge as me

pytestmark = pytest.mark.gpu

# name -> (precision, TIK_FK_SKIN, TIK_FK_CHUNK), read at handle creation
CONFIGS = {
    "sparse": ("bf16x3", "sparse", None),
    "dense": ("bf16x3", "dense", None),
    "fp32": ("fp32", "sparse", None),
    "chunk4": ("bf16x3", "sparse", "4"),
}
BATCHES = (1, 3, 4, 5, 9, 127, 128, 129)     # the 4-body skinning tile and its run split; the 128-row blend tile
JOINT_BATCHES = (1, 63, 64, 65, 193)         # the 64-body tile of fk_joints.hip; 193: the lane-per-body mapping
_MODELS = {}


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()   # the cached inputs are read-only


def model(config, cname, V=fr.V_SMALL):
    """One handle per (config, constants, V) for the module."""
    key = (config, cname, V)
    if key not in _MODELS:
        from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
        prec, skin, chunk = CONFIGS[config]
        me.lib()
        with me.env(TIK_FK_SKIN=skin, TIK_FK_CHUNK=chunk):
            _MODELS[key] = SMPLX(dict(fr.consts(cname, V)), batch_size=9, precision=prec)
    return _MODELS[key]


def check_forward(config, cname, kind, B=None, V=fr.V_SMALL):
    ref = fr.reference(cname, V, kind, B)
    m = model(config, cname, V)
    j, v = m.full_forward(*[cu(a) for a in ref["inputs"]])
    n = ref["v64"].shape[0]
    assert j.shape == (n, 144, 3) and v.shape == (n, V, 3)
    ok, r = fr.compare(j.cpu().numpy(), v.cpu().numpy(), ref)
    print(f"FK-ORACLE forward {config} {cname} {kind} B={n} V={V}: {fr.fmt(r)}")
    assert ok, (config, cname, kind, n, V, r)
    return j, v


def check_joints(config, cname, kind, B=None):
    ref = fr.reference(cname, fr.V_SMALL, kind, B)
    j = model(config, cname).joints(*[cu(a) for a in ref["inputs"]])
    assert j.shape == ref["j64"].shape
    ok, r = fr.compare(j.cpu().numpy(), None, ref)
    print(f"FK-ORACLE joints {config} {cname} {kind} B={j.shape[0]}: {fr.fmt(r)}")
    assert ok, (config, cname, kind, j.shape[0], r)


# ---------------------------------------------------------------- tik_fk_forward, V = 777
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("cname", ["std", "blend_heavy"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_forward_random(config, cname, B):
    check_forward(config, cname, "random", B)


@pytest.mark.parametrize("kind", ["yaw_sweep", "angles", "far", "bare"])
@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_forward_edges(config, kind):
    """Every contour bin and both clamps; the Rodrigues edges on the mesh path (exact zero, 1e-8,
    1e-4, near pi and 2 pi); metres of translation; pose only, the vertices returned."""
    check_forward(config, "std", kind)


@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_forward_open_barycentrics_far(config):
    """Barycentric triples that sum to 0.7 .. 1.3 under a translation of hundreds of metres:
    the landmark kernel's t (1 - sb) term is tens of metres here and dead code elsewhere."""
    check_forward(config, "bary_open", "far")


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("cname", ["nz8", "nz16", "nz17"])
def test_forward_weight_classes(cname, B):
    """Up to 7, 12 and 17 live joints per vertex: the 8- and 16-entry sparse kernels and, past
    16, the fallback of a default handle to the skinning GEMM, which is then the
    TIK_FK_SKIN=dense handle's path bit for bit."""
    j, v = check_forward("sparse", cname, "random", B)
    if cname == "nz17":
        ref = fr.reference(cname, fr.V_SMALL, "random", B)
        jd, vd = model("dense", cname).full_forward(*[cu(a) for a in ref["inputs"]])
        assert torch.equal(v, vd) and torch.equal(j, jd)


# ---------------------------------------------------------------- tik_fk_forward, V = 10475
@pytest.mark.parametrize("kind,B", [("random", 5), ("yaw_sweep", None)])
@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_forward_full_size(config, kind, B):
    check_forward(config, "std", kind, B, V=fr.V_FULL)


# ---------------------------------------------------------------- chunking
@pytest.mark.parametrize("B", [8, 9])
def test_chunk4_is_the_unchunked_handle_bitwise(B):
    """Two full chunks, and three with a ragged last one on the first chunk's v_posed buffer."""
    args = [cu(a) for a in fr.inputs("random", B)]
    j, v = model("sparse", "std").full_forward(*args)
    jc, vc = model("chunk4", "std").full_forward(*args)
    torch.cuda.synchronize()
    assert torch.isfinite(vc).all()
    assert torch.equal(vc, v) and torch.equal(jc, j)


# ---------------------------------------------------------------- tik_fk_joints
@pytest.mark.parametrize("B", JOINT_BATCHES)
@pytest.mark.parametrize("cname", ["std", "blend_heavy"])
@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_joints_random(config, cname, B):
    check_joints(config, cname, "random", B)


@pytest.mark.parametrize("kind", ["yaw_sweep", "angles"])
@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_joints_edges(config, kind):
    check_joints(config, "std", kind)


@pytest.mark.parametrize("config", ["sparse", "fp32"])
def test_joints_open_barycentrics_far(config):
    check_joints(config, "bary_open", "far")
