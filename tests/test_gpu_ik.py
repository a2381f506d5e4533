"""GPU parity of the HIP IK path (through libtik.so) against the golden fixtures
made by the reference and against the CPU oracle. Tolerance: 1e-4 abs on the
66-d poses (BASELINE.json north_star); features/blocks 1e-4 abs on O(1-5)
activations (fp32 MFMA, BN folded)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import stgcn as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module", params=["bf16x3", "bf16x3-xchunk", "fp32"])
def model(request):
    """bf16x3 (the default: 6-product bf16 split, fp32 range), the same in
    sub-batches of at most 3 windows (the 2 GiB-per-tensor chunking of large
    batches, exercised at test sizes), and exact fp32 MFMA."""
    import os
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    prec, _, path = request.param.partition("-")
    m = synthetic_model(win_size=64, device="cuda", precision=prec)
    if path:
        env = {"xchunk": {"TIK_X_CHUNK": "3"}}[path]
        os.environ.update(env)
        try:
            m.regressor.tik_handle()   # the path is fixed when the handle is created
        finally:
            for k in env:
                del os.environ[k]
    return m


@pytest.fixture(scope="module")
def sd(model):
    return {k: v.detach().cpu().numpy() for k, v in model.regressor.state_dict().items()}


@pytest.mark.parametrize("T", [64, 65, 9, 17])
def test_model_vs_golden(model, T):
    m = golden("model.npz")
    x = torch.from_numpy(m[f"T{T}|x"]).cuda()
    with torch.no_grad():
        y = model(x)["poses"].cpu().numpy()
        f = model.regressor.backbone_features(x).cpu().numpy()
    assert y.shape == m[f"T{T}|y"].shape
    assert np.abs(f - m[f"T{T}|feat"]).max() < TOL
    assert np.abs(y - m[f"T{T}|y"]).max() < TOL


@pytest.mark.parametrize("N,T", [(1, 1), (1, 2), (3, 3), (2, 5), (5, 31), (2, 100), (37, 64)])
def test_model_ragged_vs_oracle(model, sd, N, T):
    from temporal_inverse_kinematics_amd import synthetic as syn
    x = syn.synthetic_windows(N, T, seed=1000 + T)
    with torch.no_grad():
        y = model(torch.from_numpy(x).cuda())["poses"].cpu().numpy()
    ref = orc.pose_regressor(x, sd)["poses"]
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() < TOL


def test_model_full_batch_consistency(model, sd):
    """Config #2 size (1024 x 64): every window equals its solo solve (batch
    independence), sampled windows match the oracle, and a checksum of the
    per-window sums is deterministic across two launches (bitwise)."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    x = syn.synthetic_windows(1024, 64, seed=0)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y1 = model(xd)["poses"]
        y2 = model(xd)["poses"]
        solo = torch.cat([model(xd[i:i + 1])["poses"] for i in (0, 511, 1023)])
    assert torch.equal(y1, y2)
    # a solo window may take the other GEMM path (split-K): same sums, other order
    assert (y1[[0, 511, 1023]] - solo).abs().max().item() < 2e-5
    pick = [0, 1, 255, 700, 1023]
    ref = orc.pose_regressor(x[pick], sd)["poses"]
    assert np.abs(y1.cpu().numpy()[pick] - ref).max() < TOL
    assert torch.isfinite(y1).all()


def test_run_inference_sample(model):
    from temporal_inverse_kinematics_amd.inference import run_inference, synthetic_model
    r = golden("run_inference.npz")
    y64 = run_inference(model, r["seq"])
    assert y64.dtype == np.float32 and y64.shape == (231, 66)
    assert np.abs(y64 - r["win64"]).max() < TOL
    m9 = synthetic_model(win_size=9, device="cuda", precision=model.regressor.tik_precision)
    y9 = run_inference(m9, r["seq"])
    assert np.abs(y9 - r["win9"]).max() < TOL


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_blocks_vs_golden(prec):
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.models import StGcnBlock
    b = golden("blocks.npz")
    for tag in ["conv_l0", "iden_l1", "conv_s2_l2", "zero"]:
        cin, cout, s, residual = [int(v) for v in b[f"{tag}|cfg"]]
        blk = StGcnBlock(cin, cout, (3, 1), stride=s, residual=bool(residual))
        sdb = syn.block_state_dict("", cin, cout, s, residual=bool(residual), seed=5)
        blk.load_state_dict({k: torch.from_numpy(v) for k, v in sdb.items()}, strict=False)
        blk = blk.cuda().eval()
        blk.tik_precision = prec
        A = torch.from_numpy(b["A"] * b[f"{tag}|imp"]).cuda()
        for T in [9, 16]:
            with torch.no_grad():
                y, _ = blk(torch.from_numpy(b[f"{tag}|T{T}|x"]).cuda(), A)
            assert np.abs(y.cpu().numpy() - b[f"{tag}|T{T}|y"]).max() < TOL, (tag, T)


def test_gconv_vs_golden():
    from temporal_inverse_kinematics_amd.st_gcn import ConvTemporalGraphical
    g = golden("gconv.npz")
    A = torch.from_numpy(g["A"]).cuda()
    for tag in ["k5_t1", "k5_t3", "k5_t3d2"]:
        cin, cout, tk, ts, tp, td, bias = [int(v) for v in g[f"{tag}|cfg"]]
        op = ConvTemporalGraphical(cin, cout, A.shape[0], tk, ts, tp, td, bool(bias))
        st = {"conv.weight": torch.from_numpy(g[f"{tag}|conv.weight"])}
        if bias:
            st["conv.bias"] = torch.from_numpy(g[f"{tag}|conv.bias"])
        op.load_state_dict(st)
        op = op.cuda()
        with torch.no_grad():
            y, _ = op(torch.from_numpy(g[f"{tag}|x"]).cuda(), A)
        assert np.abs(y.cpu().numpy() - g[f"{tag}|y"]).max() < 1e-5, tag


def test_aa_to_rotmat_vs_kornia():
    from temporal_inverse_kinematics_amd.rotation import angle_axis_to_rotation_matrix
    k = golden("kornia.npz")
    R = angle_axis_to_rotation_matrix(torch.from_numpy(k["aa"]).cuda()).cpu().numpy()
    assert np.abs(R - k["R"]).max() < 2e-6


def test_window_gather_vs_reference():
    from temporal_inverse_kinematics_amd.windowing import gather_windows
    w = golden("windowing.npz")
    seq = torch.from_numpy(w["ids_in"]).cuda()
    got = gather_windows(seq, 9).cpu().numpy()
    assert np.abs(got - w["ids_items"]).max() < 1e-6
    arr20 = torch.from_numpy(w["arr20"]).cuda()
    with pytest.raises(ValueError):
        gather_windows(arr20, 64, idx0=5, n=1)
    got = gather_windows(arr20, 16, relative_pose=False).cpu().numpy()
    for idx in [0, 1, 10, 18, 19]:
        assert np.array_equal(got[idx], w[f"sw|20|{idx}|8"])


def test_cpu_tensor_refused(model):
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 9, 17, 3))


@pytest.mark.parametrize("prec", ["bf16x3"])
def test_concurrent_streams_bitwise(prec):
    """Four model handles on four HIP streams running concurrently give the
    same poses, bit for bit, as the serial runs (regression: layer 0's graph
    mix once read its constants as broadcast LDS loads and returned wrong
    elements when other IK kernels shared the CUs)."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    S = 4
    x = torch.from_numpy(syn.synthetic_windows(1024, 64, seed=0)).cuda()
    parts = list(x.chunk(S))
    with torch.no_grad():
        models = [synthetic_model(win_size=64, device="cuda", precision=prec).regressor for _ in range(S)]
        ref = [models[i](parts[i])["poses"].clone() for i in range(S)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(S)]
        for _ in range(12):
            ev = torch.cuda.Event()
            ev.record()
            outs = []
            for i in range(S):
                with torch.cuda.stream(streams[i]):
                    streams[i].wait_event(ev)
                    outs.append(models[i](parts[i])["poses"])
            for s in streams:
                torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            for i in range(S):
                assert torch.equal(outs[i], ref[i])


def test_two_stream_split_bitwise():
    """Large batches run as two parts on two HIP streams (a workspace per part,
    fork/join events): poses bit-identical to the one-stream run, including
    odd batches."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    precision = "bf16x3"
    split = _model_with_env(precision)
    one = _model_with_env(precision, TIK_SPLIT=0)
    for n in (1024, 1001, 513):
        x = torch.from_numpy(syn.synthetic_windows(n, 64, seed=n + 1)).cuda()
        with torch.no_grad():
            assert torch.equal(split(x)["poses"], one(x)["poses"]), n


def _model_with_env(precision="bf16x3", **env):
    """A model whose handle is built under `env` (the switches are read at
    handle creation)."""
    import os
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        m = synthetic_model(win_size=64, device="cuda", precision=precision).regressor
        m.tik_handle()   # env hooks are read at handle creation
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return m


@pytest.mark.parametrize("precision", ["bf16x3"])
def test_two_stream_split_with_chunks_bitwise(precision):
    """the split interacts with the sub-batching. With
    TIK_X_CHUNK=600 a 1001-window batch runs as a split chunk (600 windows,
    two halves) and an unsplit tail chunk (401 windows, below the 32768-frame
    threshold); a 1500-window batch as two split chunks and a 300-window tail.
    Poses are bit-identical to one unchunked stream."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    chunked = _model_with_env(precision, TIK_X_CHUNK=600)
    one = _model_with_env(precision, TIK_SPLIT=0)
    for n in (1001, 1500):
        x = torch.from_numpy(syn.synthetic_windows(n, 64, seed=n + 7)).cuda()
        with torch.no_grad():
            assert torch.equal(chunked(x)["poses"], one(x)["poses"]), n


@pytest.mark.parametrize("precision", ["bf16x3"])
def test_two_stream_split_repeated_bitwise(precision):
    """the default two-stream split path, repeated 40
    times back to back (the halves overlap differently on every run), stays
    bit-identical to the one-stream result."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    split = _model_with_env(precision)
    one = _model_with_env(precision, TIK_SPLIT=0)
    x = torch.from_numpy(syn.synthetic_windows(1024, 64, seed=11)).cuda()
    with torch.no_grad():
        ref = one(x)["poses"].clone()
        outs = [split(x)["poses"].clone() for _ in range(40)]
    torch.cuda.synchronize()
    for i, y in enumerate(outs):
        assert torch.equal(y, ref), i


def test_concurrent_streams_layer0_gcn_bitwise():
    """The kernel that once failed under concurrency (gcn0: layer 0's data_bn +
    3->64 conv + graph mix from the raw keypoints; on the bf16x3 path every
    forward runs it) runs on four HIP streams at once, beside itself:
    bit-identical to serial runs."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    S = 4
    x = torch.from_numpy(syn.synthetic_windows(1024, 64, seed=5)).cuda()
    parts = list(x.chunk(S))
    models = [_model_with_env("bf16x3", TIK_SPLIT=0) for _ in range(S)]
    with torch.no_grad():
        ref = [models[i](parts[i])["poses"].clone() for i in range(S)]
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(S)]
        for _ in range(10):
            ev = torch.cuda.Event()
            ev.record()
            outs = []
            for i in range(S):
                with torch.cuda.stream(streams[i]):
                    streams[i].wait_event(ev)
                    outs.append(models[i](parts[i])["poses"])
            for s in streams:
                torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            for i in range(S):
                assert torch.equal(outs[i], ref[i])


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_stggcn18_forward_vs_golden(prec):
    """the reference's PoseRegressor.forward calls
    self.backbone(x) (pose_trainer.py:101); StgGcn18.forward
    (st_gcn_aaai18.py:113-133) runs on its own backbone-only handle and
    matches the golden features; the head applied to them gives the golden
    poses, i.e. the reference's own forward composes with the engine."""
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    m = golden("model.npz")
    model = synthetic_model(win_size=64, device="cuda", precision=prec)
    model.regressor.backbone.tik_precision = prec
    for T in (64, 65, 9):
        x = torch.from_numpy(m[f"T{T}|x"]).cuda()
        with torch.no_grad():
            feat = model.regressor.backbone(x)
            n, w, c = feat.shape
            y = model.regressor.pose_regressor(feat.reshape(n * w, c)).reshape(n, w, -1)
        assert feat.shape == m[f"T{T}|feat"].shape
        assert np.abs(feat.cpu().numpy() - m[f"T{T}|feat"]).max() < TOL, T
        assert np.abs(y.cpu().numpy() - m[f"T{T}|y"]).max() < TOL, T


def test_checkpoint_poses_vs_golden(tmp_path):
    """a Lightning-shaped checkpoint of the seeded weights
    ({'state_dict': {'regressor.' + k}, 'hparams': Namespace}) loaded with
    IKPoseTrainer.load_from_checkpoint (strict) solves the golden windows."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams
    sd = syn.ik_state_dict(orc.graph_A("coco", "uniform", 2, 1), seed=0)
    path = tmp_path / "checkpoint_epoch=98-val_loss=0.02.ckpt"
    torch.save({"state_dict": {"regressor." + k: torch.from_numpy(v) for k, v in sd.items()},
                "hparams": default_hparams(64)}, path)
    model = IKPoseTrainer.load_from_checkpoint(str(path)).cuda().eval()
    m = golden("model.npz")
    for T in (64, 9):
        with torch.no_grad():
            y = model(torch.from_numpy(m[f"T{T}|x"]).cuda())["poses"].cpu().numpy()
        assert np.abs(y - m[f"T{T}|y"]).max() < TOL, T


def test_moveai_to_coco_device_bit_exact():
    """VERDICT r2 item 10 (§8f row 2): the moveai_3d -> COCO conversion of
    inference.py:121-133 as one device gather, bit-identical to the reference's
    own output on the shipped sample (golden keypoints.npz)."""
    from temporal_inverse_kinematics_amd.keypoints import moveai3d_to_coco_device
    k = golden("keypoints.npz")
    got = moveai3d_to_coco_device(torch.from_numpy(k["moveai_joints"].astype(np.float32)).cuda(),
                                  k["moveai_names"].tolist()).cpu().numpy()
    assert got.dtype == np.float32
    assert np.array_equal(got, k["coco_seq"])
    with pytest.raises(RuntimeError):
        moveai3d_to_coco_device(torch.zeros(3, 22, 3), k["moveai_names"].tolist())


def test_bf16x3_batch_invariant_bitwise():
    """On the default bf16x3 path every output row is computed with the same
    operations in the same order whatever the batch (row-local GEMM tiles, a
    fixed K partition of the head): windows solved inside a 1024-window batch
    (two streams), inside a 37-window batch and alone are bit-identical."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    m = synthetic_model(win_size=64, device="cuda", precision="bf16x3").regressor
    x = torch.from_numpy(syn.synthetic_windows(1024, 64, seed=21)).cuda()
    with torch.no_grad():
        full = m(x)["poses"].clone()
        part = m(x[:37])["poses"].clone()
        assert torch.equal(part, full[:37])
        for i in (0, 36, 511, 1023):
            assert torch.equal(m(x[i:i + 1])["poses"], full[i:i + 1]), i


@pytest.mark.parametrize("N", [4000, 8192])
def test_bf16x3_past_2gib_and_config3_batch(N):
    """VERDICT r3 item 3, on the default arithmetic: at T=64 one xgemm call
    holds at most 3853 windows (every fp32 activation tensor a DMA reads stays
    below 2 GiB: 32-bit buffer offsets; L2's z is 557,056 B per window), so
    4000 windows run as two chunks and BASELINE config #3's 8192-window global
    batch (inference.py:43-54 scaled) as three, on one GPU. Windows on both
    sides of each chunk boundary equal their solo solves bit for bit (the
    bf16x3 path is batch-invariant), sampled windows match the oracle, and
    every pose is finite."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    m = synthetic_model(win_size=64, device="cuda", precision="bf16x3").regressor
    x = syn.synthetic_windows(N, 64, seed=N)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y = m(xd)["poses"]
        pick = [0, 3852, 3853, 3854, 3855, N - 1] + ([7705, 7706, 7707] if N > 7706 else [])
        solo = torch.cat([m(xd[i:i + 1])["poses"] for i in pick])
    assert torch.isfinite(y).all()
    assert torch.equal(y[pick], solo)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    ref = orc.pose_regressor(x[pick[:4]], sd)["poses"]
    assert np.abs(y[pick[:4]].cpu().numpy() - ref).max() < TOL


@pytest.mark.parametrize("n,T", [(1024, 64), (37, 64), (3, 17), (70, 65), (2, 9), (1, 1), (5, 31)])
def test_xblock_whole_blocks_vs_layered(n, T):
    """Blocks 0 and 1 as whole-block kernels (xblock.hip: z kept in LDS, block
    0's output as bf16x3 planes, weights in registers; the default) against the
    layered G + T launches (TIK_XBLK=0) and the oracle: the same bf16x3
    products in the same K order, the same mix and epilogue arithmetic, and
    block 0's output as exact bf16x3 planes, so the poses are bit-identical —
    at the bench size, with partial last tiles, windows shorter than a tile,
    single frames and T=65; every pose finite."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    xb = _model_with_env("bf16x3", TIK_SPLIT=0)
    lay = _model_with_env("bf16x3", TIK_SPLIT=0, TIK_XBLK=0)
    x = syn.synthetic_windows(n, T, seed=n * 7 + T)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        a = xb(xd)["poses"].clone()
        b = lay(xd)["poses"]
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a - b).abs().max())
    sd = {k: v.detach().cpu().numpy() for k, v in xb.state_dict().items()}
    pick = list(range(min(n, 3)))
    ref = orc.pose_regressor(x[pick], sd)["poses"]
    assert np.abs(a.cpu().numpy()[pick] - ref).max() < TOL


@pytest.mark.parametrize("n,T", [(1024, 64), (37, 64), (3, 17), (70, 65), (2, 9), (1, 1), (5, 31)])
def test_xgraph_vs_tiled(n, T):
    """The gcn of the 128 / 256-channel blocks as the weight-stationary
    persistent kernel (xgraph.hip: weights in registers, joint-major MFMA
    blocks, graph mix in registers; the default) against the tiled XG128 kernel
    (TIK_XGW=0): the same bf16x3 products in the same K order and the same mix
    order, so the poses are bit-identical — at the bench size, partial last
    frame groups, windows shorter than a group, single frames and T=65."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    xg = _model_with_env("bf16x3", TIK_SPLIT=0)
    tl = _model_with_env("bf16x3", TIK_SPLIT=0, TIK_XGW=0)
    x = torch.from_numpy(syn.synthetic_windows(n, T, seed=n * 5 + T)).cuda()
    with torch.no_grad():
        a = xg(x)["poses"].clone()
        b = tl(x)["poses"]
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("n,T", [(1024, 64), (3, 16), (5, 48), (2, 9), (1, 16), (7, 128), (257, 32), (33, 96)])
def test_xtws_vs_tiled_and_oracle(n, T):
    """The temporal conv of the 128-channel stride-1 blocks (L3, L4) as the
    weight-stationary halo kernel (xtws.hip, the default: weights in VGPRs, the
    10-frame halo of an 8-frame tile split once for all 3 taps) against the
    tiled XT128 kernel (TIK_XTWS=0) and the oracle. Both accumulate in (K
    block, tap) order with the same products, so they are bitwise equal: at
    the bench size, one tile per window (both halo
    frames zero), three tiles per window, T=9 (L3 has 5 frames: not a
    multiple of 8, the tiled kernel runs), a single tile (grid of one
    workgroup), 8 tiles per window, and batches whose tiles do not divide
    evenly over the workgroups."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    xw = _model_with_env("bf16x3", TIK_SPLIT=0, TIK_XTWS=255)
    tl = _model_with_env("bf16x3", TIK_SPLIT=0, TIK_XTWS=0)
    xh = syn.synthetic_windows(n, T, seed=n * 7 + T)
    x = torch.from_numpy(xh).cuda()
    with torch.no_grad():
        a = xw(x)["poses"].clone()
        b = tl(x)["poses"]
        fa = xw.backbone_features(x)
        fb = tl.backbone_features(x)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(fa, fb), float((fa - fb).abs().max())
    sd = {k: v.detach().cpu().numpy() for k, v in xw.state_dict().items()}
    idx = [0, n - 1]
    ref = orc.pose_regressor(xh[idx], sd)["poses"]
    assert np.abs(a[idx].cpu().numpy() - ref).max() < TOL


@pytest.mark.parametrize("n,T", [(1024, 64), (3, 16), (5, 48), (2, 9), (1, 16), (7, 128), (257, 32), (33, 96), (37, 64)])
@pytest.mark.parametrize("split", ["0", "1"])
def test_xtws_fused_gcn_vs_layered(n, T, split):
    """the next block's spatial half (gcn 1x1 conv + graph
    mix + BN + ReLU, st_gcn_aaai18.py:211 of block l + 1) inside block l's
    temporal-conv launch (xtws.hip FG, the default for L3 -> G4 and L4 -> G5:
    the tile's output rows go from LDS through block l + 1's gcn, no XGW
    launch re-reads them from HBM) against separate XTW + XGW launches
    (TIK_XFG=0). Same products, K order and mix order as xgraph.hip: the
    poses and features are bitwise equal — at the bench size, one / three /
    eight tiles per window, T=9 (L3 has 5 frames: no xtws, no fusion), a
    single tile, uneven tile counts per workgroup; one stream and the
    two-part split (the second z buffer per part)."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    fu = _model_with_env("bf16x3", TIK_SPLIT=split)
    ly = _model_with_env("bf16x3", TIK_SPLIT=split, TIK_XFG=0)
    xh = syn.synthetic_windows(n, T, seed=n * 11 + T)
    x = torch.from_numpy(xh).cuda()
    with torch.no_grad():
        a = fu(x)["poses"].clone()
        b = ly(x)["poses"]
        fa = fu.backbone_features(x)
        fb = ly.backbone_features(x)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(fa, fb), float((fa - fb).abs().max())
    assert torch.equal(a, b), float((a - b).abs().max())
    sd = {k: v.detach().cpu().numpy() for k, v in fu.state_dict().items()}
    idx = [0, n - 1]
    ref = orc.pose_regressor(xh[idx], sd)["poses"]
    assert np.abs(a[idx].cpu().numpy() - ref).max() < TOL


def test_run_test_end_to_end_and_cli(tmp_path):
    """inference.run_test (`/root/reference/inference.py:110-145`) end to end on
    the reference's shipped moveai sample (data/sample_3d_poses/
    dance_contemporary.npz: its joints_3d and joint_3d_names, kept in
    tests/golden/keypoints.npz and written back here in the file's layout):
    moveai -> COCO on the device, IK over every frame, against the goldens the
    reference itself produced (keypoints.npz coco_seq, run_inference.npz
    win64); then the same through the CLI (`python -m
    temporal_inverse_kinematics_amd.inference file.npz --out poses.npy`)."""
    import subprocess
    import sys
    from temporal_inverse_kinematics_amd.inference import run_test
    k, r = golden("keypoints.npz"), golden("run_inference.npz")
    src = tmp_path / "cam01_track00.npz"
    np.savez(src, joints_3d=k["moveai_joints"].astype(np.float32), joint_3d_names=k["moveai_names"])
    out = run_test(str(src), win_size=64)
    assert np.array_equal(out["coco"], k["coco_seq"].astype(np.float32))
    assert out["poses"].shape == (231, 66) and np.isfinite(out["poses"]).all()
    assert np.abs(out["poses"] - r["win64"]).max() < TOL
    dst = tmp_path / "poses.npy"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "temporal_inverse_kinematics_amd.inference", str(src), "--out", str(dst)],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "solved 231 frames" in p.stdout
    assert np.array_equal(np.load(dst), out["poses"])


@pytest.mark.parametrize("n,T", [(64, 64), (5, 17), (2, 9)])
def test_xblock_workspace_all_64_channel_backbone(n, T):
    """with blocks 0 and 1 whole (xblock.hip) block 0's
    output goes into the z workspace as bf16x3 planes, 384 B per pixel, more
    than any later 64-channel layer's fp32 z. A backbone of 64-channel layers
    only (a stride-2 64 -> 64 layer after the two whole blocks) must size z
    for it: the default path equals the layered one (TIK_XBLK=0) bit for bit
    and the float64 oracle."""
    import os
    from temporal_inverse_kinematics_amd import synthetic as syn
    from temporal_inverse_kinematics_amd.models import StgConfig, StgGcn18, StgLayerConfig
    layers = [(3, 64, 1), (64, 64, 1), (64, 64, 2), (64, 64, 1)]
    A = orc.graph_A("coco", "uniform", 2, 1)
    sd = syn.ik_state_dict(A, seed=3, layers=layers)
    bsd = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
    cfg = StgConfig([StgLayerConfig(a, b, s, True) for a, b, s in layers], 3)

    def make(**env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            m = StgGcn18(cfg, {"layout": "coco", "strategy": "uniform", "max_hop": 2, "dilation": 1})
            r = m.load_state_dict({k: torch.from_numpy(v) for k, v in bsd.items()}, strict=False)
            assert not [k for k in r.missing_keys if "num_batches_tracked" not in k] and not r.unexpected_keys, r
            m = m.cuda().eval()
            m.tik_handle()
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        return m
    xb, lay = make(TIK_SPLIT="0"), make(TIK_SPLIT="0", TIK_XBLK="0")
    x = syn.synthetic_windows(n, T, seed=n + T)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        a = xb(xd).clone()
        b = lay(xd)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a - b).abs().max())
    ref = orc.backbone(x[:2], sd, layers=layers)
    assert np.abs(a[:2].cpu().numpy() - ref.reshape(a[:2].shape)).max() < TOL


_LAYERS_32_96 = [(3, 32, 1), (32, 32, 1), (32, 96, 2), (96, 96, 1)]
_models_32_96_cache = []


def _models_32_96():
    """(bf16x3 backbone, fp32 backbone, state dict) of the 32/96-channel net, built once."""
    if not _models_32_96_cache:
        from temporal_inverse_kinematics_amd import synthetic as syn
        from temporal_inverse_kinematics_amd.models import StgConfig, StgGcn18, StgLayerConfig
        A = orc.graph_A("coco", "uniform", 2, 1)
        sd = syn.ik_state_dict(A, seed=5, layers=_LAYERS_32_96)
        bsd = {k[len("backbone."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("backbone.")}
        cfg = StgConfig([StgLayerConfig(a, b, s, True) for a, b, s in _LAYERS_32_96], 3)
        nets = []
        for prec in ("bf16x3", "fp32"):
            m = StgGcn18(cfg, {"layout": "coco", "strategy": "uniform", "max_hop": 2, "dilation": 1})
            r = m.load_state_dict(bsd, strict=False)
            assert not [k for k in r.missing_keys if "num_batches_tracked" not in k] and not r.unexpected_keys, r
            m = m.cuda().eval()
            m.tik_precision = prec
            nets.append(m)
        _models_32_96_cache.append((nets[0], nets[1], sd))
    return _models_32_96_cache[0]


@pytest.mark.parametrize("n,T", [(1, 1), (3, 9), (9, 16)])
def test_backbone_32_and_96_channels(n, T):
    """Layer widths that are multiples of 32 but not of 64 run the tiled
    kernels no default net reaches: the temporal conv on 64-column tiles with
    a partial last column tile (xgemm_kernel<64, EPI_BIAS>: layer 0's residual
    conv from the raw keypoints, an identity residual on 32 and on 96
    channels, a two-segment stride-2 conv 32 -> 96) and the tiled gcn on 32
    and 96 columns. Rows: 17 (one partial tile), 459 (window edges at T' = 5),
    2448 (many tiles, a partial last one). Every window against the float64
    oracle and against the fp32 path (cgemm.hip, an independent kernel)."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    bf, fp, sd = _models_32_96()
    x = syn.synthetic_windows(n, T, seed=n + T)
    xd = torch.from_numpy(x).cuda()
    with torch.no_grad():
        a = bf(xd).cpu().numpy()
        b = fp(xd).cpu().numpy()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.shape == (n, (T - 1) // 2 + 1, 17 * 96)
    ref = orc.backbone(x, sd, layers=_LAYERS_32_96).reshape(a.shape)
    err_o, err_f = np.abs(a - ref).max(), np.abs(a - b).max()
    print(f"32/96-channel backbone (n={n}, T={T}): max|bf16x3-oracle|={err_o:.3e} max|bf16x3-fp32|={err_f:.3e}")
    assert err_o < TOL, err_o
    assert err_f < TOL, err_f
