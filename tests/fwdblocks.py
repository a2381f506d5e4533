"""Weights, inputs, references and the comparator of the per-block forward tests
(tests/test_gpu_forward_blocks.py on the GPU, tests/test_forward_blocks_host.py
on the host). Not a test module.

Everything here is numpy on the float64 oracle (oracle/stgcn.py); nothing
imports the HIP library, so the host test of the comparator runs anywhere.

The bar of block k: with rel32_k = max|oracle_f32 - oracle_f64| / max|oracle_f64|
at block k's output on a fixed calibration batch (the same weights),

    max|got - oracle_f64|  <=  MARGIN * max(rel32_k, 2^-23) * max|oracle_f64|

on the case's own block output. The bar is a property of the reference alone.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from oracle import stgcn as orc
from temporal_inverse_kinematics_amd import synthetic as syn

LAYERS = list(orc.IK_LAYERS)
NL = len(LAYERS)
V = 17

# how many times the float32 oracle's own rounding noise a kernel may be off
# (the ratio test_gpu_precision.py grants bf16x3 over the fp32 path). Below the
# 7.6x at which one frame read from two bf16 planes instead of three shows.
MARGIN = 4.0
EPS32 = 2.0 ** -23

# (N, T): each chosen for a tile edge
SHAPES = [
    (1, 1), (1, 2),        # a single frame / both halo frames zero
    (2, 9), (3, 17),       # shorter than, and one past, a 16-frame xgraph group; odd through four stride-2 layers
    (2, 29),               # two 14-frame xblock tiles + a 1-frame tail
    (1, 16),               # the smallest window that reaches xtws (L3/L4 have 8 frames: one tile, one workgroup)
    (2, 48),               # three xtws tiles per window: fused gcn with interior halos
    (3, 65),               # T = 65 (win_size 64): 33-frame stride chain
    (5, 31),               # ragged in every kernel
    (37, 64),              # N*T*17 is no multiple of the 128-row xgemm tile
    (257, 16),             # more tiles than workgroups in the persistent kernels (256 CUs)
]
HOSTILE_SHAPES = [(2, 29), (1, 16), (3, 65)]
CALIB = (8, 32)

GRAPHS = ("hop2", "hop3", "dense", "hop2_signed")     # x "std" weights
SPARSE = {"hop2": True, "hop3": False, "dense": False, "hop2_signed": True}
HOSTILE_GRAPHS = ("hop2", "dense")                     # x "hostile" weights
WEIGHT_SETS = [(g, "std") for g in GRAPHS] + [(g, "hostile") for g in HOSTILE_GRAPHS]
# The float64 oracle costs seconds on the two largest shapes, so (257, 16), which
# is about tile scheduling and not the mix, runs on one sparse and one dense graph.
BIG = (257, 16)
BIG_GRAPHS = ("hop2", "dense")


def cases():
    """(graph, kind, N, T), grouped by weight set."""
    out = []
    for g, kind in WEIGHT_SETS:
        for N, T in (SHAPES if kind == "std" else HOSTILE_SHAPES):
            if (N, T) != BIG or g in BIG_GRAPHS:
                out.append((g, kind, N, T))
    return out


def input_kinds(N):
    """One window: both inputs in turn. More: one batch that alternates them."""
    return ("windows", "white") if N == 1 else ("mixed",)


# running_var of the hostile BatchNorms: log-uniform over this range (eps = 1e-5
# dominates the channels below it). The issue's full range; the float32 oracle
# passes the comparator on it, so it was not narrowed.
HOSTILE_VAR = (1e-6, 1e2)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def hop2_pattern():
    """(17,17) bool: the COCO hop <= 2 pattern the sparse graph mix unrolls,
    recomputed from the oracle's hop distances."""
    n, edges, _ = orc._edges("coco")
    return orc.hop_distance(n, edges, 2) <= 2


def a_eff(sd, l):
    return sd["backbone.A"][0].astype(np.float64) * sd[f"backbone.edge_importance.{l}"][0].astype(np.float64)


def is_sparse(sd, l):
    """What fold_block (csrc/fold.h) decides: every nonzero of A_eff inside the hop <= 2 pattern."""
    return not np.any((a_eff(sd, l) != 0) & ~hop2_pattern())


@functools.lru_cache(maxsize=None)
def weights(graph, kind="std"):
    """Seed-0 state dict (float32 arrays) for one adjacency kind, optionally with hostile BatchNorms."""
    if graph in ("hop2", "hop2_signed"):
        A = orc.graph_A("coco", "uniform", 2, 1)
    elif graph == "hop3":
        A = orc.graph_A("coco", "uniform", 3, 1)
    elif graph == "dense":
        # every entry nonzero, mixed signs, columns of L1 norm 1.5
        r = _rng("dense-A")
        A = r.uniform(0.2, 1.0, (1, V, V)) * r.choice([-1.0, 1.0], (1, V, V))
        A = 1.5 * A / np.abs(A).sum(1, keepdims=True)
    else:
        raise ValueError(graph)
    sd = dict(syn.ik_state_dict(A, seed=0))
    if graph == "hop2_signed":
        # edge importance with negative entries and exact zeros (still inside the pattern)
        for l in range(NL):
            r = _rng("imp", l)
            imp = r.uniform(-1.5, 1.5, (1, V, V))
            imp[r.uniform(size=imp.shape) < 0.15] = 0.0
            sd[f"backbone.edge_importance.{l}"] = imp.astype(np.float32)
    if kind == "hostile":
        for k in [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]:
            r = _rng("hostile", k)
            c = sd[k + ".weight"].shape[0]
            g = sd[k + ".weight"].astype(np.float64) * r.choice([-1.0, 1.0], c)   # sign-flipped on about half
            g[int(r.integers(c))] = 0.0                                            # one channel exactly 0
            sd[k + ".weight"] = g.astype(np.float32)
            lo, hi = np.log10(HOSTILE_VAR[0]), np.log10(HOSTILE_VAR[1])
            sd[k + ".running_var"] = (10.0 ** r.uniform(lo, hi, c)).astype(np.float32)
            sd[k + ".running_mean"] = r.uniform(-2.0, 2.0, c).astype(np.float32)
    elif kind != "std":
        raise ValueError(kind)
    for l in range(NL):
        assert is_sparse(sd, l) == SPARSE[graph], (graph, l)
    for v in sd.values():
        v.setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def inputs(kind, N, T):
    """(N,T,17,3) float32. 'windows': crops of the sample sequence; 'white': N(0, 0.3)
    iid per frame, joint and coordinate, so a frame-indexing error is not softened
    by the sequence's smoothness; 'mixed': the two in alternating windows."""
    if kind == "windows":
        x = syn.synthetic_windows(N, T, seed=1000 + 7 * N + T)
    elif kind == "white":
        x = _rng("white", N, T).normal(0.0, 0.3, (N, T, V, 3)).astype(np.float32)
    elif kind == "mixed":   # even windows from the sample sequence, odd ones white
        x = np.array(inputs("windows", N, T), copy=True)
        x[1::2] = inputs("white", N, T)[1::2]
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    return x


def _taps(x, sd, dtype):
    t = []
    orc.backbone(x, sd, dtype=dtype, taps=t)
    return t


@functools.lru_cache(maxsize=2)
def reference(graph, kind, inp, N, T):
    """The float64 oracle's eight block outputs, (N,T_k,17*C_k) each. Computed once, read-only."""
    t = _taps(inputs(inp, N, T), weights(graph, kind), np.float64)
    for a in t:
        a.setflags(write=False)
    return t


def calib_inputs():
    n, T = CALIB
    return np.concatenate([inputs("windows", n // 2, T), inputs("white", n - n // 2, T)])


@functools.lru_cache(maxsize=None)
def rel32(graph, kind):
    """rel32_k for k = 0..7, and the head's (index 8, on the float64 features
    rounded to float32: what the head kernels are given), on the calibration batch."""
    sd, x = weights(graph, kind), calib_inputs()
    t64, t32 = _taps(x, sd, np.float64), _taps(x, sd, np.float32)
    out = [float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()) for a, b in zip(t32, t64)]
    f = t64[-1].reshape(-1, t64[-1].shape[-1]).astype(np.float32)
    h64 = orc.head(f, sd, np.float64)
    out.append(float(np.abs(orc.head(f, sd, np.float32).astype(np.float64) - h64).max() / np.abs(h64).max()))
    return tuple(out)


def bar(rel, ref, margin=MARGIN):
    return margin * max(rel, EPS32) * float(np.abs(ref).max())


def compare(got, ref, rel, margin=MARGIN):
    """-> (ok, err, bar, index of the worst element in ref's shape)."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    d = np.abs(got - ref)
    i = np.unravel_index(int(np.argmax(d)), d.shape)
    err, b = float(d[i]), bar(rel, ref, margin)
    return bool(np.isfinite(got).all() and err <= b), err, b, i


def describe(ref, idx, k):
    """Where the worst element sits: window, frame (of how many), joint, channel."""
    c = LAYERS[k][1] if k < NL else ref.shape[-1]
    n, t, vc = idx if len(idx) == 3 else (idx[0], 0, idx[-1])
    return f"window {n}, frame {t} of {ref.shape[1] if ref.ndim == 3 else 1}, joint {vc // c}, channel {vc % c}"


# ------------------------------------------------------------ error injections
def round_planes(a, planes):
    """a rounded to the sum of its first `planes` bf16 planes (round to nearest
    even on the exact float32 residuals, as the kernels split their operands)."""
    a = np.asarray(a, dtype=np.float32)
    acc = np.zeros_like(a)
    for _ in range(planes):
        r = (a - acc).astype(np.float32)
        u = r.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        acc = acc + u.astype(np.uint32).view(np.float32)
    return acc


def block_from_input(sd, k, xin):
    """Block k in float64 from its input in the taps' layout (N,T,17*C) (k = 0: the raw keypoints (N,T,17,3))."""
    if k == 0:
        t = []
        orc.backbone(xin, sd, dtype=np.float64, layers=LAYERS[:1], taps=t)
        return t[0]
    ci, co, s = LAYERS[k]
    n, T, _ = xin.shape
    h = np.asarray(xin, dtype=np.float64).reshape(n, T, V, ci).transpose(0, 3, 1, 2)
    y = orc.stgcn_block(h, a_eff(sd, k)[None], sd, f"backbone.st_gcn_networks.{k}.", ci, co, s)
    return y.transpose(0, 2, 3, 1).reshape(n, y.shape[2], -1)


def last_frame_rounded(sd, k, xin, planes):
    """Block k's float64 output when the last frame of its input is read from
    `planes` bf16 planes instead of in full: what a halo or partial-tile path
    that drops planes would produce."""
    x = np.array(xin, dtype=np.float64, copy=True)
    x[:, -1] = round_planes(x[:, -1].astype(np.float32), planes).astype(np.float64)
    return block_from_input(sd, k, x)
