"""What the kernels do to memory outside their logical tensors.

The arithmetic tests run on workspaces that are zero (fresh pages) or hold
small finite stale activations, and on caller tensors with nothing of
interest around them. A kernel that reads a never-written row, joint lane or
padded channel and multiplies it by a zero weight, or whose range check is a
row too wide, is bit-correct there. Here:

  * poisoned workspaces (TIK_POISON=ff: NaN; 7f: 3.39e38, finite, so it
    survives a ReLU that flushes NaN): every handle is created and run with
    every new library buffer filled with the poison byte, its workspace
    reserved larger than any call uses (a poison tail), the tile-edge shapes
    ascending and then descending (stale rows of larger calls). The outputs
    must be finite and bit-identical (torch.equal) to an unpoisoned handle
    sized exactly for the call;
  * a positive control: the fill is really applied (tik_debug_alloc_fill) and
    malformed values are refused;
  * sentinel slabs: each input and output of each C-ABI entry point sits
    inside a buffer with 64 Ki floats of NaN (inputs also 0x7f7f7f7f; the
    outputs' NaN carries a payload of its own) on both sides. After the call every pad still holds its fill bit for bit (no
    out-of-bounds store) and the outputs equal the plain call's bit for bit
    (no over-read contributed).

No tolerance is involved except the one oracle comparison per configuration
(1e-4, as in test_gpu_ik.py).
"""
import ctypes

import numpy as np
import pytest
import torch

import memedge as me
from oracle import stgcn as orc

pytestmark = pytest.mark.gpu

FILLS = ["ff", "7f"]
TOL = 1e-4


@pytest.fixture(autouse=True)
def _no_poison_left(monkeypatch):
    monkeypatch.delenv("TIK_POISON", raising=False)
    yield


# ---------------------------------------------------------------- a. poisoned workspaces, IK model
_ik_ref_cache = {}


def _ik_ref(config):
    if config not in _ik_ref_cache:
        with me.poison(None):
            _ik_ref_cache[config] = me.ik_reference(config)
    return _ik_ref_cache[config]


@pytest.mark.parametrize("config", list(me.IK_CONFIGS))
def test_ik_reference_vs_oracle(config):
    """The reference of the poison tests is itself right: one shape per configuration against the float64 oracle."""
    ref = _ik_ref(config)
    s = me.SPLIT_SHAPE if config == "split" else (5, 31)
    pick = [0, s[0] - 1]
    x = me.ik_input(*s)[pick].cpu().numpy()
    sd = {k: v for k, v in me.ik_named() if not k.startswith("tik.")}
    want = orc.pose_regressor(x, sd)["poses"]
    got = ref[s][1][pick].cpu().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() < TOL


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("config", list(me.IK_CONFIGS))
def test_ik_poisoned_workspace(config, fill):
    ref = _ik_ref(config)
    with me.poison(fill):
        got = me.ik_family(config)
    assert me.lib().tik_debug_alloc_fill() == int(fill, 16)
    want = {(tag, s): ref[s] for tag in ("up", "down") for s in me.ik_shapes(config)}
    me.assert_same(got, want, (config, fill))


# ---------------------------------------------------------------- b. the other handles
_ref_cache = {}


def _ref(key, fn):
    if key not in _ref_cache:
        with me.poison(None):
            _ref_cache[key] = fn()
    return _ref_cache[key]


@pytest.mark.parametrize("fill", FILLS)
def test_block_poisoned_workspace(fill):
    ref = _ref("block", lambda: me.block_family(fresh=True))
    with me.poison(fill):
        got = me.block_family()
    me.assert_same(got, ref, ("block", fill))


@pytest.mark.parametrize("fill", FILLS)
def test_gconv_under_poison(fill):
    ref = _ref("gconv", me.gconv_family)
    with me.poison(fill):
        got = me.gconv_family()
    me.assert_same(got, ref, ("gconv", fill))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("config", list(me.FK_CONFIGS))
def test_fk_poisoned_workspace(config, fill):
    ref = _ref(("fk", config), lambda: me.fk_family(config, reserve=None))
    with me.poison(fill):
        got = me.fk_family(config)
    me.assert_same(got, ref, ("fk", config, fill))


@pytest.mark.parametrize("fill", FILLS)
def test_trainer_poisoned_workspace(fill):
    """Losses, every gradient, parameter, Adam moment and running statistic
    after each step, and the evals, against an unpoisoned trainer (two
    trainers agree bitwise: test_train_step_bitwise_reproducible)."""
    ref = _ref("trainer", me.trainer_family)
    with me.poison(fill):
        got = me.trainer_family()
    me.assert_same(got, ref, ("trainer", fill))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("win,online", me.STREAM_CASES)
def test_stream_poisoned_workspace(win, online, fill):
    """stream.cpp (alloc_common, alloc_dataflow) sets onl_act (tags), onl_cnt,
    count and ring before the first launch; the layered step (stream_step.cpp)
    writes window, frame_in and poses before it reads them."""
    ref = _ref(("stream", win, online), lambda: me.stream_family(win, online))
    with me.poison(fill):
        got = me.stream_family(win, online)
    assert got["path"] == ("dataflow" if online == "1" else "layered")
    assert got["got"].shape == got["ref"].shape == (6, 66)
    assert np.abs(got["got"] - got["ref"]).max() < 1e-5      # as test_stream_matches_run_inference
    me.assert_same(got, ref, ("stream", win, online, fill))


# ---------------------------------------------------------------- c. positive control
def test_poison_fill_is_applied_and_parsed():
    """Allocations report the fill they got; unset means none; anything but
    two hex digits fails the allocation (TIK_E_INVALID -> ValueError)."""
    L = me.lib()
    from temporal_inverse_kinematics_amd import _lib
    for fill, want in (("ff", 0xFF), ("7f", 0x7F), ("A5", 0xA5), ("00", 0), (None, -1)):
        with me.poison(fill):
            h = me.ik_handle("default")
            assert L.tik_debug_alloc_fill() == want, fill
            _lib.check(L.tik_model_reserve(h.h, 1, 9))     # read per call: the lazily reserved workspace too
            assert L.tik_debug_alloc_fill() == want, fill
    h = me.ik_handle("default")
    for bad in ("", "f", "fff", "zz", "0x", " ff", "1"):
        with me.poison(bad):
            with pytest.raises(ValueError, match="TIK_POISON"):
                _lib.check(L.tik_model_reserve(h.h, 2, 9))
            with pytest.raises(ValueError, match="TIK_POISON"):
                me.ik_handle("default")
    # switched on in a process that has long loaded the library, and off again
    with me.poison("7f"):
        _lib.check(L.tik_model_reserve(h.h, 2, 9))
        assert L.tik_debug_alloc_fill() == 0x7F
    _lib.check(L.tik_model_reserve(h.h, 3, 9))
    assert L.tik_debug_alloc_fill() == -1
    f, p = me.ik_forward(h, me.ik_input(2, 9))
    me.assert_same({"x": (f, p)}, {"x": _ik_ref("default")[(2, 9)]}, "after poison")


# ---------------------------------------------------------------- d. sentinel slabs
PAD = 1 << 16                      # 64 Ki elements of fill on each side
NAN_BITS = 0x7FC00000              # torch's float('nan'): around the inputs
BIG_BITS = 0x7F7F7F7F              # 3.39e38: around the inputs, second pass
OUT_BITS = 0x7FD5A5A5              # a quiet NaN with a payload no arithmetic produces: around (and in) the outputs,
#                                    so a stray store of a NaN, which carries 0x7FC00000 or an input's payload, shows
IN_FILLS = [NAN_BITS, BIG_BITS]
FILL_IDS = ["nan", "7f7f7f7f"]


class Slabs:
    """Places tensors inside 1-D buffers with PAD elements of fill on each side."""

    def __init__(self, in_bits, out_bits=OUT_BITS):
        self.in_bits, self.out_bits, self.items = in_bits, out_bits, []

    def _place(self, shape, dtype, bits, what):
        n = int(np.prod(shape))
        assert torch.empty((), dtype=dtype).element_size() == 4
        buf = torch.full((n + 2 * PAD,), bits, device="cuda", dtype=torch.int32)
        view = buf[PAD:PAD + n].view(dtype).view(*shape)
        assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * PAD
        self.items.append((what, buf, n, bits))
        return view

    def inp(self, t, what="in"):
        v = self._place(t.shape, t.dtype, self.in_bits, what)
        v.copy_(t)
        return v

    def out(self, shape, what="out", dtype=torch.float32):
        return self._place(shape, dtype, self.out_bits, what)   # the payload starts as the fill too

    def check(self, ctx):
        torch.cuda.synchronize()
        for what, buf, n, bits in self.items:
            for side, pad in (("front", buf[:PAD]), ("back", buf[PAD + n:])):
                changed = int((pad != bits).sum())
                assert changed == 0, (ctx, what, side, f"{changed} pad words changed")


class Plain:
    """The same interface on ordinary tensors (the reference call)."""

    def inp(self, t, what="in"):
        return t.clone()

    def out(self, shape, what="out", dtype=torch.float32):
        return torch.full(tuple(shape), float("nan"), device="cuda", dtype=dtype)

    def check(self, ctx):
        torch.cuda.synchronize()


def _sentinel(call, ctx, fills=IN_FILLS):
    """call(placer) -> {name: output}; once plain, then in slabs with each input fill."""
    want = call(Plain())
    torch.cuda.synchronize()
    for bits in fills:
        sl = Slabs(bits)
        got = call(sl)
        sl.check((ctx, hex(bits)))
        me.assert_same(got, want, (ctx, hex(bits)))


@pytest.mark.parametrize("config", ["default", "xblk0", "fp32"])
def test_sentinel_model_entry_points(config):
    """tik_ik_forward and tik_backbone_forward: x, poses and features in slabs, over the shape list."""
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    h = me.ik_handle(config)
    for s in me.SHAPES:
        x = me.ik_input(*s)
        To = _lib.check(L.tik_model_out_frames(h.h, s[1]))

        def call(p):
            f, y = me.ik_forward(h, p.inp(x, "x"), p.out((s[0], To, 17 * 256), "feat"), p.out((s[0], To, 66), "poses"))
            return {"feat": f, "poses": y}
        _sentinel(call, (config, s))


@pytest.mark.parametrize("tag", me.BLOCK_TAGS)
def test_sentinel_block_fwd(tag):
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    b = me.golden("blocks.npz")
    blk, A = me._block(tag, "bf16x3")
    h = blk._handle(A)
    x = torch.from_numpy(b[f"{tag}|T9|x"]).cuda().permute(0, 2, 3, 1).contiguous()   # channels-last
    N, T, V, _ = x.shape
    To = (T - 1) // blk.stride + 1

    def call(p):
        xi, o = p.inp(x, "x"), p.out((N, To, V, blk.out_channels))
        _lib.check(L.tik_stgcn_block_fwd(h, xi.data_ptr(), N, T, o.data_ptr(), _lib.stream_of(x)))
        return {"out": o}
    _sentinel(call, tag)


@pytest.mark.parametrize("tag", me.GCONV_TAGS)
def test_sentinel_gconv(tag):
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    g = me.golden("gconv.npz")
    cin, cout, tk, ts, tp, td, bias = [int(v) for v in g[f"{tag}|cfg"]]
    x = torch.from_numpy(g[f"{tag}|x"]).cuda()
    A = torch.from_numpy(g["A"]).cuda()
    W = torch.from_numpy(g[f"{tag}|conv.weight"]).cuda()
    bv = torch.from_numpy(g[f"{tag}|conv.bias"]).cuda() if bias else None
    N, _, T, V = x.shape
    K = A.shape[0]
    To = (T + 2 * tp - td * (tk - 1) - 1) // ts + 1

    def call(p):
        xi, Ai, Wi = p.inp(x, "x"), p.inp(A, "A"), p.inp(W, "W")
        bi = p.inp(bv, "b") if bv is not None else None
        o = p.out((N, cout, To, V))
        _lib.check(L.tik_gconv_fwd(xi.data_ptr(), N, cin, T, V, Ai.data_ptr(), K, Wi.data_ptr(), _lib.ptr(bi), cout,
                                   tk, ts, tp, td, o.data_ptr(), _lib.stream_of(x)))
        return {"out": o}
    _sentinel(call, tag)


def test_sentinel_window_gather():
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    seq = torch.from_numpy(me.golden("windowing.npz")["ids_in"]).cuda()
    F, V, _ = seq.shape
    h = 4

    def call(p):
        s, o = p.inp(seq, "seq"), p.out((F, 2 * h + 1, V, 3))
        _lib.check(L.tik_window_gather(s.data_ptr(), F, V, 0, F, h, 11, 12, 1, o.data_ptr(), _lib.stream_of(seq)))
        return {"windows": o}
    _sentinel(call, "window_gather")


def test_sentinel_aa_to_rotmat():
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    aa = torch.from_numpy(me.golden("kornia.npz")["aa"].astype(np.float32)).cuda()
    n = aa.shape[0]

    def call(p):
        a, o = p.inp(aa, "aa"), p.out((n, 3, 3))
        _lib.check(L.tik_aa_to_rotmat(a.data_ptr(), n, o.data_ptr(), _lib.stream_of(aa)))
        return {"R": o}
    _sentinel(call, "aa_to_rotmat")


def test_sentinel_moveai_to_coco():
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.keypoints import generate_moveai3d_to_coco_mappings
    L = me.lib()
    k = me.golden("keypoints.npz")
    j = torch.from_numpy(k["moveai_joints"].astype(np.float32)).cuda()
    F, J, _ = j.shape
    m = (ctypes.c_int * 17)(*generate_moveai3d_to_coco_mappings(k["moveai_names"].tolist()))

    def call(p):
        ji, o = p.inp(j, "joints"), p.out((F, 17, 3))
        _lib.check(L.tik_moveai_to_coco(ji.data_ptr(), F, J, m, o.data_ptr(), _lib.stream_of(j)))
        return {"coco": o}
    _sentinel(call, "moveai_to_coco")


def test_sentinel_train_windows():
    """One 20-frame sequence of 60 joints, windows of 9 frames at the left edge, inside and at the right edge, with noise."""
    from temporal_inverse_kinematics_amd import _lib
    from temporal_inverse_kinematics_amd.training_data import SMPLX_TO_COCO, coco_kps_sigma
    L = me.lib()
    rng = np.random.default_rng(3)
    F, J, ld, h = 20, 60, 70, 4
    joints = torch.from_numpy(rng.normal(0, 1, (F, J, 3)).astype(np.float32)).cuda()
    poses = torch.from_numpy(rng.normal(0, 1, (F, ld)).astype(np.float32)).cuda()
    local = [0, 3, 10, 16, 19]
    B = len(local)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    start, length, idx, uid = i32([0] * B), i32([F] * B), i32(local), i32(local)
    cmap = (ctypes.c_int * 17)(*SMPLX_TO_COCO)
    sig = (ctypes.c_float * 17)(*[float(s) for s in coco_kps_sigma()])

    def call(p):
        args = [p.inp(t, n) for t, n in ((joints, "joints"), (poses, "poses"), (start, "start"), (length, "len"),
                                         (idx, "idx"), (uid, "uid"))]
        win, tgt = p.out((B, 2 * h + 1, 17, 3), "windows"), p.out((B, 66), "target")
        _lib.check(L.tik_train_windows(args[0].data_ptr(), J, args[1].data_ptr(), ld, args[2].data_ptr(),
                                       args[3].data_ptr(), args[4].data_ptr(), args[5].data_ptr(), B, h,
                                       ctypes.addressof(cmap), ctypes.addressof(sig), 1, 1, 12345, win.data_ptr(),
                                       tgt.data_ptr(), _lib.stream_of(joints)))
        return {"windows": win, "target": tgt}
    _sentinel(call, "train_windows")


@pytest.mark.parametrize("config", ["sparse", "dense"])
def test_sentinel_fk_forward(config):
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    m = me.fk_model(config)
    B = 3
    args = [torch.from_numpy(a).cuda() for a in me.fk_inputs(B)]

    def call(p):
        a = [p.inp(t, n) for t, n in zip(args, ("pose", "betas", "expr", "transl"))]
        j, v = p.out((B, m.num_joints, 3), "joints"), p.out((B, m.num_verts, 3), "verts")
        _lib.check(L.tik_fk_forward(m._h, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), B,
                                    j.data_ptr(), v.data_ptr(), _lib.stream_of(args[0])))
        return {"joints": j, "verts": v}
    _sentinel(call, ("fk", config))


@pytest.mark.parametrize("bits", IN_FILLS, ids=FILL_IDS)
def test_sentinel_trainer(bits):
    """tik_trainer_step (x, target, mask, loss), tik_trainer_eval (x, target,
    poses, loss) and tik_trainer_read (dst) on a trainer whose every pointer
    sits in a slab, against a second trainer called on plain tensors."""
    from temporal_inverse_kinematics_amd import _lib
    L = me.lib()
    N, T = 3, 9
    x, y = me.train_batch(N, T, 61)
    mask = (torch.rand((N * 1, 512), generator=torch.Generator().manual_seed(5)) < 0.3).float().cuda()
    xe, ye = me.train_batch(5, 17, 62)
    res = []
    for p in (Plain(), Slabs(bits)):
        tr = me.new_trainer()
        st = _lib.stream_of(x)
        out = {}
        xi, yi, mi, loss = p.inp(x, "x"), p.inp(y, "target"), p.inp(mask, "mask"), p.out((1,), "loss")
        _lib.check(L.tik_trainer_step(tr._h.h, xi.data_ptr(), N, T, yi.data_ptr(), mi.data_ptr(), 0, loss.data_ptr(), st))
        out["loss"] = loss
        xi, yi = p.inp(xe, "eval x"), p.inp(ye, "eval target")
        ep, el = p.out(tuple(ye.shape), "eval poses"), p.out((1,), "eval loss")
        _lib.check(L.tik_trainer_eval(tr._h.h, xi.data_ptr(), 5, 17, yi.data_ptr(), ep.data_ptr(), el.data_ptr(), st))
        out["eval_poses"], out["eval_loss"] = ep, el
        for i, (name, shape, kind) in enumerate(tr._names):
            for what in ((0, 1, 2, 3) if kind == 0 else (0,)):
                dst = p.out(shape if len(shape) else (1,), f"read {name} {what}")
                _lib.check(L.tik_trainer_read(tr._h.h, i, what, dst.data_ptr(), st))
                out[(name, what)] = dst
        p.check(("trainer", hex(bits)))
        res.append(out)
    me.assert_same(res[1], res[0], ("trainer", hex(bits)))
