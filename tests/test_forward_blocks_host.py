"""Host test of the per-block comparator (tests/fwdblocks.py), on the oracle's
own arrays: the bar of tests/test_gpu_forward_blocks.py passes what is right and
fails what is subtly wrong, so it cannot drift into one that nothing can fail.

1. The float32 oracle passes every block and the head at MARGIN on every shape,
   input and weight set of the GPU test (the two largest shapes on their first
   8 windows: windows are independent in eval mode, and the float64 oracle
   costs seconds on the whole of them).
2. The float64 output of a block whose last input frame was rounded to two
   bf16 planes fails at blocks 1-4 (standard weights, every adjacency, (5, 31)).
3. Rounded to one plane it fails at every block, on every weight set. With a
   3-tap temporal conv and padding 1 the last input frame is sampled at every
   stride, so "every block whose last input frame is sampled" is all eight.

Measured (err / float32-oracle noise; the bar is MARGIN = 4): 1. at most 1.6
on a block and 2.0 on the head (1.9 and 3.3 on the whole of the largest
shapes); 2. 5.3 to 25.8 on blocks 1-4, (5, 31); 3. at
least 350. With the hostile BatchNorms a two-plane rounding stays below the
bar (0.7 to 6.9): a few channels with 1/sqrt(var + eps) near 300 set max|f64|,
and the bar is relative to it. That set is there for the BatchNorm fold.
"""
import numpy as np
import pytest

import fwdblocks as fb
from oracle import stgcn as orc

HOST_WINDOWS = 8


def _host_inputs(inp, N, T):
    return fb.inputs(inp, N, T)[:HOST_WINDOWS]


@pytest.mark.parametrize("graph,kind", fb.WEIGHT_SETS)
def test_float32_oracle_passes(graph, kind):
    sd, rel = fb.weights(graph, kind), fb.rel32(graph, kind)
    worst = np.zeros(fb.NL + 1)
    for g, kd, N, T in fb.cases():
        if (g, kd) != (graph, kind):
            continue
        for inp in fb.input_kinds(N):
            x = _host_inputs(inp, N, T)
            t64, t32 = fb._taps(x, sd, np.float64), fb._taps(x, sd, np.float32)
            f = t64[-1].reshape(-1, t64[-1].shape[-1]).astype(np.float32)
            t64.append(orc.head(f, sd, np.float64))
            t32.append(orc.head(f, sd, np.float32))
            for k in range(fb.NL + 1):
                ok, err, b, idx = fb.compare(t32[k], t64[k], rel[k])
                worst[k] = max(worst[k], err / (b / fb.MARGIN))
                assert ok, (graph, kind, N, T, inp, k, err, b)
    print(f"FWDBLOCKS-HOST f32 oracle {graph}/{kind}: " + " ".join(f"{v:.2f}" for v in worst))


def _injected_ratios(graph, kind, N, T, planes):
    sd, rel = fb.weights(graph, kind), fb.rel32(graph, kind)
    inp = fb.input_kinds(N)[0]
    x = fb.inputs(inp, N, T)
    ref = fb.reference(graph, kind, inp, N, T)
    out = []
    for k in range(fb.NL):
        y = fb.last_frame_rounded(sd, k, x if k == 0 else ref[k - 1], planes)
        ok, err, b, idx = fb.compare(y, ref[k], rel[k])
        assert idx[1] >= ref[k].shape[1] - 2       # the damage is at the window's end
        out.append((ok, err / (b / fb.MARGIN)))
    return out


@pytest.mark.parametrize("graph", fb.GRAPHS)
def test_two_plane_last_frame_fails_blocks_1_to_4(graph):
    r = _injected_ratios(graph, "std", 5, 31, 2)
    print(f"FWDBLOCKS-HOST two planes {graph}: " + " ".join(f"{v:.1f}" for _, v in r))
    for k in (1, 2, 3, 4):
        assert not r[k][0], (graph, k, r[k])


@pytest.mark.parametrize("graph,kind", fb.WEIGHT_SETS)
def test_one_plane_last_frame_fails_every_block(graph, kind):
    N, T = (5, 31) if kind == "std" else (2, 29)
    r = _injected_ratios(graph, kind, N, T, 1)
    print(f"FWDBLOCKS-HOST one plane {graph}/{kind}: " + " ".join(f"{v:.0f}" for _, v in r))
    for k in range(fb.NL):
        assert not r[k][0] and r[k][1] > 10 * fb.MARGIN, (graph, kind, k, r[k])


def test_three_planes_are_exact_and_round_planes_is_bf16():
    """The injection tool itself: three planes reproduce a float32 exactly, one
    plane is round-to-nearest-even bfloat16."""
    import torch
    a = np.random.default_rng(5).normal(0, 3, 4096).astype(np.float32)
    assert np.array_equal(fb.round_planes(a, 3), a)
    assert np.array_equal(fb.round_planes(a, 1), torch.from_numpy(a).bfloat16().float().numpy())
    e2 = np.abs(fb.round_planes(a, 2).astype(np.float64) - a).max() / np.abs(a).max()
    assert 2.0 ** -19 < e2 < 2.0 ** -16


def test_taps_are_the_prefix_backbones():
    """taps[k-1] is what a backbone over the first k layers returns (the GPU test
    compares a k-layer handle with it), and the last tap is the backbone's output."""
    sd, x = fb.weights("hop2"), fb.inputs("white", 2, 9)
    t = []
    out = orc.backbone(x, sd, taps=t)
    assert len(t) == fb.NL and np.array_equal(t[-1], out)
    for k in (1, 3, 6):
        assert np.array_equal(orc.backbone(x, sd, layers=fb.LAYERS[:k]), t[k - 1])


def test_dense_and_sparse_adjacencies_are_what_they_claim():
    """mix_sparse is not in the launch labels: the dense matrices fall outside the
    hop <= 2 pattern in every layer and the sparse ones inside (the pattern
    recomputed from orc.hop_distance), zeros and negative entries included."""
    pat = fb.hop2_pattern()
    assert int(pat.sum()) == 107
    for g, kind in fb.WEIGHT_SETS:
        sd = fb.weights(g, kind)
        for l in range(fb.NL):
            assert fb.is_sparse(sd, l) == fb.SPARSE[g], (g, kind, l)
    imp = fb.weights("hop2_signed")["backbone.edge_importance.3"][0]
    assert (imp[pat] == 0).any() and (imp[pat] < 0).any()
    assert (fb.a_eff(fb.weights("dense"), 0) != 0).all()
    hostile = fb.weights("hop2", "hostile")
    for k in [k for k in hostile if k.endswith(".running_var")]:
        g = hostile[k[:-len("running_var")] + "weight"]
        assert (g == 0).sum() == 1 and (g < 0).any() and (g > 0).any()
        assert hostile[k].min() >= fb.HOSTILE_VAR[0] * 0.999 and hostile[k].max() <= fb.HOSTILE_VAR[1] * 1.001
    assert min(hostile[k].min() for k in hostile if k.endswith(".running_var")) < orc.BN_EPS
