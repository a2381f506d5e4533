"""Every block of the inference forward against the float64 oracle, and the
dense graph mix.

A backbone over the first k layers of the IK config, with the full model's
weights, returns block k-1's output in full (tik_backbone_forward), so every
block of the network is compared element by element with the oracle's output
of the same block (oracle/stgcn.py, taps=), k = 1..8; k = 8 is the full model's
own handle. The head (pose_regressor) is checked on its own: the GPU poses
against the oracle's head applied in float64 to the GPU's own features.

Bar (tests/fwdblocks.py): max|gpu - f64| <= MARGIN * max(rel32_k, 2^-23) *
max|f64| per block, rel32_k the float32 oracle's own relative error at that
block on a fixed 8x32 calibration batch with the same weights. MARGIN = 4, the
ratio test_gpu_precision.py grants bf16x3 over fp32; a last input frame read
from two bf16 planes instead of three shows at 5x to 25x on blocks 1-4
(tests/test_forward_blocks_host.py proves the bar can fail).

Shapes, adjacencies, weights and inputs: tests/fwdblocks.py. Adjacencies: the
standard hop-2 graph and a hop-2 graph with zero and negative edge importance
(sparse mix); graph_A('coco','uniform',3,1) and a random full 17x17 matrix
(dense mix: the branch of xblock, xgraph, xtws' fused gcn and cgemm that no
other forward test runs). For the dense kinds the layered launches run too
(TIK_XBLK=0 TIK_XGW=0: layer0.hip and xgemm's graph epilogue). Hostile
weights: every BatchNorm with gamma sign-flipped on half the channels and 0 on
one, running_var log-uniform over [1e-6, 1e2], running_mean within +-2.

Every case asserts the launch labels of its forward (tik_model_profile), so a
fall-back to another kernel cannot pass; whether a mix is sparse or dense is
not in the labels and is asserted on the host from orc.hop_distance.

Measured on an MI355X: max|gpu - f64| over the float32 oracle's noise
(max(rel32_k, 2^-23) * max|f64|), the worst over every shape and input of the
weight set, in the unit of MARGIN. Every block of every case passed at 4 and
every launch list matched; the layered 8-layer forward of the dense kinds gave
block 7's figure exactly. The largest is 2.93: no rounding source needed more
than the starting margin, and nothing was widened.

    weights        precision   b0   b1   b2   b3   b4   b5   b6   b7  head | MARGIN
    hop2/std       bf16x3     1.62 1.77 2.43 1.92 1.76 1.74 1.19 2.45 1.80 | 4
    hop2/std       fp32       1.24 1.35 2.10 1.91 1.62 1.51 1.00 1.18 1.27 | 4
    hop3/std       bf16x3     1.42 1.73 1.18 1.21 1.65 2.05 1.17 2.83 1.75 | 4
    hop3/std       fp32       1.02 1.44 1.04 1.14 1.32 1.55 0.98 0.89 0.88 | 4
    dense/std      bf16x3     1.43 1.50 1.03 1.05 1.11 1.62 1.39 2.04 2.18 | 4
    dense/std      fp32       1.00 1.08 1.12 1.10 1.12 1.56 1.21 1.74 1.17 | 4
    hop2_signed    bf16x3     1.41 1.88 0.83 0.81 0.88 1.03 1.07 1.37 2.44 | 4
    hop2_signed    fp32       0.96 1.07 1.14 1.08 1.21 1.21 1.01 0.91 1.28 | 4
    hop2/hostile   bf16x3     1.43 1.56 1.43 1.42 2.10 2.93 2.02 2.78 1.92 | 4
    hop2/hostile   fp32       1.31 0.89 0.78 0.89 1.02 1.17 1.02 2.21 1.18 | 4
    dense/hostile  bf16x3     2.14 1.07 1.74 1.27 1.31 1.32 2.23 2.25 2.19 | 4
    dense/hostile  fp32       0.82 0.85 1.18 0.89 0.98 0.97 1.02 0.77 1.08 | 4

(The float32 oracle itself, same unit: up to 1.9 on a block and 3.3 on the head.)
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import fwdblocks as fb
from oracle import stgcn as orc

pytestmark = pytest.mark.gpu

PRECS = ("bf16x3", "fp32")


# ------------------------------------------------------------------ models
def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _prefix_backbone(sd, k, env=None):
    """StgGcn18 over the first k IK layers with the full state dict's weights."""
    from temporal_inverse_kinematics_amd.models import StgConfig, StgGcn18, StgLayerConfig
    cfg = StgConfig([StgLayerConfig(a, b, s, True) for a, b, s in fb.LAYERS[:k]], 3)
    m = StgGcn18(cfg, {"layout": "coco", "strategy": "uniform", "max_hop": 2, "dilation": 1})
    pre = "backbone."
    keep = {}
    for key, v in sd.items():
        if not key.startswith(pre):
            continue
        parts = key[len(pre):].split(".")
        if parts[0] in ("st_gcn_networks", "edge_importance") and int(parts[1]) >= k:
            continue
        keep[key[len(pre):]] = torch.from_numpy(np.array(v))
    r = m.load_state_dict(keep, strict=False)
    assert not [x for x in r.missing_keys if "num_batches_tracked" not in x] and not r.unexpected_keys, r
    m = m.cuda().eval()
    _with_env(env or {}, m.tik_handle)   # the path is fixed when the handle is created
    return m


def _full_model(sd):
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams
    m = IKPoseTrainer(default_hparams(64))
    m.regressor.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
    m = m.cuda().eval()
    m.regressor.tik_handle()
    return m.regressor


ALT_ENV = {"TIK_XBLK": "0", "TIK_XGW": "0"}
_models = {}


def models(graph, kind):
    """The handles of one weight set: prefixes 1..7, the full model, and for a
    dense adjacency the 8-layer backbone on the layered launches. One set alive at a time."""
    if (graph, kind) not in _models:
        _models.clear()
        sd = fb.weights(graph, kind)
        ms = {k: _prefix_backbone(sd, k) for k in range(1, fb.NL)}
        ms[fb.NL] = _full_model(sd)
        if not fb.SPARSE[graph]:
            ms["alt"] = _prefix_backbone(sd, fb.NL, ALT_ENV)
        _models[(graph, kind)] = ms
    return _models[(graph, kind)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    yield
    _models.clear()


# ------------------------------------------------------------------ launches
def profiled(mod, fn):
    """fn() with the handle's launch profiler on -> (result, launch labels in order)."""
    from temporal_inverse_kinematics_amd import _lib
    lib, h = _lib.load(), mod.tik_handle()
    _lib.check(lib.tik_model_profile(h, 64))
    try:
        out = fn()
        torch.cuda.synchronize()
        n = _lib.check(lib.tik_model_profile_count(h))
        lab = ctypes.create_string_buffer(64)
        labels = []
        for i in range(n):
            _lib.check(lib.tik_model_profile_read(h, i, lab, 64, None, None, None))
            labels.append(lab.value.decode())
    finally:
        lib.tik_model_profile(h, 0)
    return out, labels


def expected_labels(k, T, prec, alt=False):
    """The launches of a k-layer backbone forward at window length T (csrc/forward.cpp:
    backbone / backbone_x, with the predicates of Layer in csrc/model.h)."""
    if prec == "fp32":   # cgemm.hip: graph tile + temporal conv per layer
        labs = ["data_bn"]
        for l in range(k):
            labs += [f"G272x64.L{l}", ("T128x128.L" if fb.LAYERS[l][1] >= 128 else "T256x64.L") + str(l)]
        return labs
    xblk = k >= 2 and not alt
    labs = ["XB0.L0", "XB1.L1"] if xblk else ["G0f_raw.L0", "XP64.L0"]
    t, zin = T, False
    for l in range(2 if xblk else 1, k):
        cin, cout, s = fb.LAYERS[l]
        xtws = cin == cout == 128 and s == 1 and t % 8 == 0
        fuse = xtws and not alt and l + 1 < k and fb.LAYERS[l + 1][:2] == (128, 128)
        if not zin:   # else the previous block's fused launch made this block's z
            labs.append((f"XG{min(cout, 128)}.L" if alt else "XGW.L") + str(l))
        if xtws:
            labs.append(("XTWG.L" if fuse else "XTW.L") + str(l))
        else:
            labs.append(("XP64.L" if cout == 64 else "XT128.L") + str(l))
        zin = fuse
        t = (t - 1) // s + 1
    return labs


HEAD_LABELS = {"bf16x3": ["XH128.head0", "XR.head0", "H64x64.head3"], "fp32": ["H64x64.head0", "H64x64.head3"]}


def test_expected_labels_cover_the_kernels():
    """The label model itself: where blocks 3 and 4 see a multiple of 8 frames
    (T = 16, and T = 31 as well: 16 frames after the stride-2 block) the full
    bf16x3 forward is the two whole blocks, xgraph on the 128- and 256-channel
    blocks and the fused xtws launches on blocks 3 and 4; any other T takes the
    tiled temporal convs."""
    assert expected_labels(8, 16, "bf16x3") == ["XB0.L0", "XB1.L1", "XGW.L2", "XT128.L2", "XGW.L3", "XTWG.L3", "XTWG.L4",
                                                 "XT128.L5", "XGW.L6", "XT128.L6", "XGW.L7", "XT128.L7"]
    assert expected_labels(8, 29, "bf16x3") == ["XB0.L0", "XB1.L1", "XGW.L2", "XT128.L2", "XGW.L3", "XT128.L3", "XGW.L4",
                                                 "XT128.L4", "XGW.L5", "XT128.L5", "XGW.L6", "XT128.L6", "XGW.L7", "XT128.L7"]
    assert expected_labels(8, 31, "bf16x3") == expected_labels(8, 16, "bf16x3")
    assert expected_labels(4, 16, "bf16x3")[-2:] == ["XGW.L3", "XTW.L3"]
    assert expected_labels(5, 16, "bf16x3")[-2:] == ["XTWG.L3", "XTW.L4"]
    assert expected_labels(1, 16, "bf16x3") == ["G0f_raw.L0", "XP64.L0"]


# ------------------------------------------------------------------ the cases
def _run_case(graph, kind, N, T, prec, report):
    """Every block, the layered variant (dense kinds) and the head of one case.
    -> list of failures; report(tag, block, err / noise) receives every ratio."""
    rel = fb.rel32(graph, kind)
    ms = models(graph, kind)
    fails = []
    for inp in fb.input_kinds(N):
        ref = fb.reference(graph, kind, inp, N, T)
        xd = torch.from_numpy(np.array(fb.inputs(inp, N, T))).cuda()
        tag = f"{graph}/{kind} ({N},{T}) {inp} {prec}"

        def check(what, k, got, want, r, labels, expect):
            ok, err, b, idx = fb.compare(got, want, r)
            report(what, err / (b / fb.MARGIN))
            if labels != expect:
                fails.append(f"{tag} {what}: launches {labels}, expected {expect}")
            if not ok:
                fails.append(f"{tag} {what}: max|gpu - f64| = {err:.3e} > bar {b:.3e} ({err / (b / fb.MARGIN):.1f}x the "
                             f"float32 oracle's noise) at {fb.describe(want, idx, k)}")

        keys = list(range(1, fb.NL + 1)) + (["alt"] if "alt" in ms and prec == "bf16x3" else [])
        feat = None
        for key in keys:
            m = ms[key]
            k = fb.NL if key == "alt" else key
            m.tik_precision = prec
            fwd = m.backbone_features if key == fb.NL else m
            with torch.no_grad():
                out, labels = profiled(m, lambda: fwd(xd))
            out = out.cpu().numpy()
            assert out.shape == ref[k - 1].shape, (tag, key, out.shape)
            if key == fb.NL:
                feat = out
            check(f"block{k - 1}" + ("-layered" if key == "alt" else ""), k - 1, out, ref[k - 1], rel[k - 1], labels,
                  expected_labels(k, T, prec, alt=key == "alt"))
        # the head on the GPU's own features
        m = ms[fb.NL]
        with torch.no_grad():
            out, labels = profiled(m, lambda: m(xd)["poses"])
        poses = out.cpu().numpy()
        sd = fb.weights(graph, kind)
        want = orc.head(feat.reshape(-1, feat.shape[-1]), sd, np.float64).reshape(poses.shape)
        check("head", fb.NL, poses, want, rel[fb.NL], labels, expected_labels(fb.NL, T, prec) + HEAD_LABELS[prec])
    return fails


RATIOS = {}   # (graph, kind, prec, what) -> worst err / float32-oracle noise over the cases run


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("graph,kind,N,T", fb.cases(), ids=lambda v: str(v))
def test_blocks_vs_oracle(graph, kind, N, T, prec):
    def report(what, ratio):
        key = (graph, kind, prec, what)
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    fails = _run_case(graph, kind, N, T, prec, report)
    print(f"FWDBLOCKS {graph}/{kind} ({N},{T}) {prec}: " +
          " ".join(f"{w}={RATIOS[(graph, kind, prec, w)]:.2f}" for (g, kd, p, w) in RATIOS if (g, kd, p) == (graph, kind, prec)))
    assert not fails, "\n".join(fails)
