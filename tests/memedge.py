"""Workloads shared by tests/test_gpu_memory_edges.py (in the pytest process,
under TIK_POISON) and tests/guard_child.py (in a child process, under
TIK_GUARD=1): every handle type of libtik.so at the shapes where a tile, a
temporal tap or a padded row ends. Not a test module (pytest does not
collect it); each family returns {key: tensor or ndarray} so that two runs
can be compared bit for bit.
"""
import contextlib
import functools
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

# (windows, frames): the tile edges the kernels' own tests name. 1 frame; 9
# (L3 has 5 frames: no xtws); 13 / 14 / 15 around block 0's 14-frame tile;
# 16 (one 8-frame xtws tile at L3); 29 and 31 (partial last tiles, odd
# halves at every stride-2 layer); 65 (one frame past the bench window).
SHAPES = [(1, 1), (2, 9), (1, 13), (1, 14), (1, 15), (3, 16), (2, 29), (5, 31), (3, 65)]
RESERVE = (8, 65)          # larger than any shape above in every buffer
SPLIT_SHAPE = (513, 64)    # the two-stream split starts at 32768 frames

# name -> (precision, switches read at handle creation)
IK_CONFIGS = {
    "default": ("bf16x3", {"TIK_SPLIT": "0"}),
    "xblk0": ("bf16x3", {"TIK_SPLIT": "0", "TIK_XBLK": "0"}),
    "xgw0": ("bf16x3", {"TIK_SPLIT": "0", "TIK_XGW": "0"}),
    "xtws0": ("bf16x3", {"TIK_SPLIT": "0", "TIK_XTWS": "0"}),
    "xtws255": ("bf16x3", {"TIK_SPLIT": "0", "TIK_XTWS": "255"}),
    "xfg0": ("bf16x3", {"TIK_SPLIT": "0", "TIK_XFG": "0"}),
    "xchunk3": ("bf16x3", {"TIK_SPLIT": "0", "TIK_X_CHUNK": "3"}),
    "fp32": ("fp32", {"TIK_SPLIT": "0"}),
    "split": ("bf16x3", {"TIK_SPLIT": "1"}),
}
_IK_SWITCHES = ("TIK_SPLIT", "TIK_XBLK", "TIK_XGW", "TIK_XTWS", "TIK_XFG", "TIK_X_CHUNK", "TIK_PRECISION")

BLOCK_TAGS = ["conv_l0", "iden_l1", "conv_s2_l2", "zero"]
GCONV_TAGS = ["k5_t1", "k5_t3", "k5_t3d2"]

# name -> (precision, TIK_FK_SKIN, TIK_FK_CHUNK)
FK_CONFIGS = {
    "sparse": ("bf16x3", "sparse", None),
    "dense": ("bf16x3", "dense", None),
    "chunk2": ("bf16x3", "sparse", "2"),    # the two-stream chunk pipeline at test sizes
    "fp32": ("fp32", "sparse", None),
}
FK_BATCHES = (1, 3, 37)
FK_RESERVE = 64

STREAM_CASES = [(9, "1"), (64, "1"), (9, "0"), (64, "0")]   # (win_size, TIK_ONLINE)


@contextlib.contextmanager
def env(**kv):
    """Set (value) or unset (None) environment variables for the block."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# Called (when set) while a family's handle is still alive and its work is done:
# tests/guard_child.py checks the guard zones there, before the buffers are freed.
ON_RELEASE = None


def release(*handles):
    if ON_RELEASE is not None:
        torch.cuda.synchronize()
        ON_RELEASE()


def poison(fill):
    """TIK_POISON=fill for the block (None: unset, the reference runs)."""
    return env(TIK_POISON=fill)


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def lib():
    from temporal_inverse_kinematics_amd import _build, _lib
    _build.build()
    return _lib.load()


def nan_like(shape):
    return torch.full(tuple(shape), float("nan"), device="cuda", dtype=torch.float32)


# ---------------------------------------------------------------- IK model
@functools.lru_cache(maxsize=None)
def ik_named():
    """The seeded PoseRegressor state dict as tik_model_create takes it."""
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.models import _state_numpy
    reg = synthetic_model(win_size=64, device="cpu").regressor
    named = _state_numpy(reg)
    named.append(("tik.strides", np.array(reg.backbone.strides, dtype=np.float32)))
    return named


@functools.lru_cache(maxsize=None)
def ik_input(N, T):
    from temporal_inverse_kinematics_amd import synthetic as syn
    return torch.from_numpy(syn.synthetic_windows(N, T, seed=1000 * N + T)).cuda()


def ik_handle(config):
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.models import _create_model_handle
    prec, switches = IK_CONFIGS[config]
    lib()
    with env(**{**{k: None for k in _IK_SWITCHES}, **switches}):
        h = _create_model_handle(ik_named())
    _lib.check(_lib.load().tik_model_set_precision(h.h, _lib.precision_code(prec)))
    return h


def ik_forward(h, x, feat=None, poses=None):
    """tik_backbone_forward and tik_ik_forward on x -> (features, poses)."""
    from temporal_inverse_kinematics_amd import _lib
    L = _lib.load()
    N, T = x.shape[:2]
    To = _lib.check(L.tik_model_out_frames(h.h, T))
    feat = nan_like((N, To, 17 * 256)) if feat is None else feat
    poses = nan_like((N, To, 66)) if poses is None else poses
    st = _lib.stream_of(x)
    _lib.check(L.tik_backbone_forward(h.h, x.data_ptr(), N, T, feat.data_ptr(), st), "tik_backbone_forward")
    _lib.check(L.tik_ik_forward(h.h, x.data_ptr(), N, T, poses.data_ptr(), st), "tik_ik_forward")
    torch.cuda.synchronize()
    return feat, poses


def ik_shapes(config):
    return [SPLIT_SHAPE] if config == "split" else list(SHAPES)


def ik_reference(config, shapes=None):
    """Every shape on a handle of its own: each buffer exactly as large as the call needs."""
    out = {}
    for s in shapes or ik_shapes(config):
        h = ik_handle(config)
        out[s] = ik_forward(h, ik_input(*s))
        release(h)
        del h
    return out


def ik_family(config, shapes=None, reserve=RESERVE):
    """One handle, its workspace reserved larger than any call uses, the
    shapes ascending and then descending (stale rows of the larger calls
    behind the smaller ones) -> {(pass, shape): (features, poses)}."""
    from temporal_inverse_kinematics_amd import _lib
    shapes = shapes or ik_shapes(config)
    h = ik_handle(config)
    if reserve:
        _lib.check(_lib.load().tik_model_reserve(h.h, *reserve), "tik_model_reserve")
    out = {}
    for tag, order in (("up", shapes), ("down", shapes[::-1])):
        for s in order:
            out[(tag, s)] = ik_forward(h, ik_input(*s))
    release(h)
    return out


# ---------------------------------------------------------------- block API, gconv
def _block(tag, prec):
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.models import StGcnBlock
    b = golden("blocks.npz")
    cin, cout, s, residual = [int(v) for v in b[f"{tag}|cfg"]]
    blk = StGcnBlock(cin, cout, (3, 1), stride=s, residual=bool(residual))
    sdb = syn.block_state_dict("", cin, cout, s, residual=bool(residual), seed=5)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in sdb.items()}, strict=False)
    blk = blk.cuda().eval()
    blk.tik_precision = prec
    return blk, torch.from_numpy(b["A"] * b[f"{tag}|imp"]).cuda()


def block_family(fresh=False):
    """tik_stgcn_block_fwd on the four golden blocks: T = 9, 16, then 9 again
    behind the larger call's rows (fresh: a handle per call, exactly sized)."""
    lib()
    b = golden("blocks.npz")
    out = {}
    for prec in ("bf16x3", "fp32"):
        for tag in BLOCK_TAGS:
            blk, A = _block(tag, prec)
            for i, T in enumerate((9, 16, 9)):
                if fresh and i:
                    release(blk)
                    blk, A = _block(tag, prec)
                with torch.no_grad():
                    y, _ = blk(torch.from_numpy(b[f"{tag}|T{T}|x"]).cuda(), A)
                torch.cuda.synchronize()
                out[(prec, tag, i, T)] = y
            release(blk)
    return out


def gconv_family():
    from temporal_inverse_kinematics_amd.st_gcn import ConvTemporalGraphical
    lib()
    g = golden("gconv.npz")
    A = torch.from_numpy(g["A"]).cuda()
    out = {}
    for tag in GCONV_TAGS:
        cin, cout, tk, ts, tp, td, bias = [int(v) for v in g[f"{tag}|cfg"]]
        op = ConvTemporalGraphical(cin, cout, A.shape[0], tk, ts, tp, td, bool(bias))
        st = {"conv.weight": torch.from_numpy(g[f"{tag}|conv.weight"])}
        if bias:
            st["conv.bias"] = torch.from_numpy(g[f"{tag}|conv.bias"])
        op.load_state_dict(st)
        op = op.cuda()
        with torch.no_grad():
            y, _ = op(torch.from_numpy(g[f"{tag}|x"]).cuda(), A)
        torch.cuda.synchronize()
        out[tag] = y
    release()   # no handle and no library buffer: the kernel works on the caller's tensors only
    return out


# ---------------------------------------------------------------- FK
@functools.lru_cache(maxsize=None)
def fk_consts():
    from temporal_inverse_kinematics_amd import synthetic as syn
    return syn.synthetic_smplx_constants(seed=1)


def fk_inputs(B, seed=None):
    """test_gpu_fk.py's inputs: pose, betas, expression, translation (numpy)."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    seed = 10 + B if seed is None else seed
    pose, betas = syn.synthetic_fk_inputs(B, seed=seed)
    rng = np.random.default_rng(seed)
    expr = rng.normal(0, 0.5, (B, 10)).astype(np.float32)
    transl = rng.normal(0, 0.5, (B, 3)).astype(np.float32)
    return pose, betas, expr, transl


def fk_model(config):
    from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
    prec, skin, chunk = FK_CONFIGS[config]
    lib()
    with env(TIK_FK_SKIN=skin, TIK_FK_CHUNK=chunk):
        return SMPLX(fk_consts(), batch_size=9, precision=prec)


def fk_family(config, reserve=FK_RESERVE):
    """tik_fk_forward at B = 1, 3, 37 on a handle reserved for 64 bodies
    (reserve=None: the buffers grow to each batch exactly), with vertices and,
    at B = 3, joints only (the handle's own vertex workspace)."""
    from temporal_inverse_kinematics_amd import _lib
    m = fk_model(config)
    if reserve:
        _lib.check(_lib.load().tik_fk_reserve(m._h, reserve), "tik_fk_reserve")
    out = {}
    for B in FK_BATCHES:
        args = [torch.from_numpy(a).cuda() for a in fk_inputs(B)]
        bufs = (nan_like((B, m.num_joints, 3)), nan_like((B, m.num_verts, 3)))
        j, v = m.full_forward(*args, out=bufs)
        torch.cuda.synchronize()
        out[(B, "joints")], out[(B, "verts")] = j, v
        if B == 3:
            j2, _ = m.full_forward(*args, return_verts=False, out=(nan_like((B, m.num_joints, 3)), None))
            torch.cuda.synchronize()
            out[(B, "joints_only")] = j2
    release(m)
    return out


# ---------------------------------------------------------------- trainer
TRAIN_STEPS = [(64, 9), (64, 9), (3, 9), (6, 17), (2, 1), (1, 2), (5, 4)]
TRAIN_EVALS = [(1, 1), (5, 17)]


def train_batch(N, T, seed):
    from temporal_inverse_kinematics_amd import synthetic as syn
    x = torch.from_numpy(syn.synthetic_windows(N, T, seed=seed)).cuda()
    To = T
    for s in (1, 1, 2, 1, 1, 2, 2, 2):
        To = (To - 1) // s + 1
    y = torch.from_numpy(np.random.default_rng(seed).normal(0, 0.5, (N, To, 66)).astype(np.float32)).cuda()
    return x, y


def new_trainer():
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    lib()
    return GpuTrainer(synthetic_model(win_size=9, device="cpu"), lr=1e-4)


def trainer_state(tr, tag, out):
    """Every gradient, parameter, Adam moment and buffer of the trainer."""
    for name, _, kind in tr._names:
        out[(tag, name, "value")] = tr.tensor(name)
        if kind == 0:
            for what in ("grad", "exp_avg", "exp_avg_sq"):
                out[(tag, name, what)] = tr.tensor(name, what)


def trainer_family():
    """Two steps at (64,9), then a smaller batch and another window length
    (the workspaces keep the larger calls' rows), then windows below 9 frames
    ((2,1): every temporal tap in the padding; (1,2), (5,4): the stride-2
    layers collapse to one frame), the whole state after each; then evals at one frame and at (5,17)."""
    tr = new_trainer()
    out = {}
    for i, (N, T) in enumerate(TRAIN_STEPS):
        x, y = train_batch(N, T, 40 + i)
        out[("loss", i)] = tr.step(x, y, seed=7 + i)
        trainer_state(tr, f"step{i}", out)
    for N, T in TRAIN_EVALS:
        x, y = train_batch(N, T, 50 + T)
        out[("eval_poses", N, T)], out[("eval_loss", N, T)] = tr.evaluate(x, y)
    trainer_state(tr, "after_eval", out)
    torch.cuda.synchronize()
    release(tr)
    return out


# ---------------------------------------------------------------- online stream
def stream_family(win, online):
    """h + 6 pushes (the first 6 poses) of the online stream against the same
    frames of run_inference."""
    from temporal_inverse_kinematics_amd.inference import run_inference, synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    lib()
    seq = golden("run_inference.npz")["seq"][:100]
    h = win // 2
    with env(TIK_ONLINE=online):
        m = synthetic_model(win_size=win, device="cuda")
        ref = run_inference(m, seq)[:6]
        s = OnlineIK(m, use_graph=True)   # no reset: the first launch runs on what tik_stream_create set up
        got = [s.push(fr) for fr in seq[:h + 6]]
        release(s, m)
    assert all(p is None for p in got[:h]) and all(p is not None for p in got[h:])
    return {"got": np.stack(got[h:]), "ref": ref, "path": s.path}


# ---------------------------------------------------------------- comparison
def as_list(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def assert_same(got, ref, what):
    """got and ref ({key: tensor | ndarray | tuple of them}) are finite and bit-identical."""
    assert set(got) == set(ref), (what, sorted(map(str, set(got) ^ set(ref))))
    for k in ref:
        for i, (a, b) in enumerate(zip(as_list(got[k]), as_list(ref[k]))):
            if a is None and b is None:
                continue
            if isinstance(a, str) or isinstance(b, str):
                assert a == b, (what, k, a, b)
                continue
            a, b = torch.as_tensor(a), torch.as_tensor(b)
            assert a.shape == b.shape, (what, k, i, a.shape, b.shape)
            if a.is_floating_point():
                assert bool(torch.isfinite(a).all()), (what, k, i, "non-finite values",
                                                       int((~torch.isfinite(a)).sum()))
            assert torch.equal(a, b), (what, k, i, "max |diff|",
                                       float((a.double() - b.double()).abs().max()))
