"""Block 0's whole-block kernel (xblock.hip) walks tiles of 14 output frames
(16 input frames: all 16 frame lanes of its VALU gcn live), block 1 tiles of
10. Checked against the layered G + T launches (TIK_XBLK=0), which run the
same arithmetic in the same order, so the backbone features (a function of
block 1's output alone, which in turn reads block 0's planes) and the poses
are compared with torch.equal. The library has no entry point that returns a
single block's output, so the features stand in for it."""
import numpy as np
import pytest
import torch

from oracle import stgcn as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4   # tests/test_gpu_ik.py's oracle tolerance


def _model_with_env(**env):
    """A bf16x3 model whose handles are built under `env` (the switches are
    read at handle creation)."""
    import os
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        m = synthetic_model(win_size=64, device="cuda", precision="bf16x3").regressor
        m.tik_handle()
        m.backbone.tik_handle()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return m


@pytest.fixture(scope="module")
def models():
    """One fresh model (and handles) per setting, one stream."""
    return {"xblk": _model_with_env(TIK_SPLIT=0),
            "layered": _model_with_env(TIK_SPLIT=0, TIK_XBLK=0)}


def _windows(n, T):
    from temporal_inverse_kinematics_amd import synthetic as syn
    return syn.synthetic_windows(n, T, seed=n * 7 + T)


# (windows, frames). Around block 1's 10-frame tile: below one tile; exactly one;
# two with a partial second; tiles that straddle window edges (the zero-row taps
# at a tile boundary). The same around block 0's 14-frame tile: (1, 13), (1, 14),
# (1, 15), (1, 27), (2, 14), (3, 15), (2, 29). T = 64 and 65. (9, 64) is 42 / 58
# tiles, one per workgroup; (90, 64) is 412 / 576 tiles, so that on 256 CUs some
# workgroups walk one tile and others two (block 0), or two and three (block 1);
# (120, 64) gives block 0 two and three
SHAPES = [(1, 9), (1, 10), (1, 17), (3, 10), (2, 21), (5, 13), (1, 13), (1, 14), (1, 15), (1, 27), (2, 14), (3, 15),
          (2, 29), (3, 64), (3, 65), (9, 64), (90, 64), (120, 64)]


@pytest.mark.parametrize("n,T", SHAPES)
def test_xb0_tile14_vs_layered(models, n, T):
    x = torch.from_numpy(_windows(n, T)).cuda()
    with torch.no_grad():
        out = {k: (m.backbone_features(x).clone(), m(x)["poses"].clone()) for k, m in models.items()}
    f, p = out["xblk"]
    fo, po = out["layered"]
    assert torch.isfinite(p).all()
    assert torch.equal(f, fo), float((f - fo).abs().max())
    assert torch.equal(p, po), float((p - po).abs().max())


def test_xb0_tile14_vs_oracle(models):
    """The existing oracle tolerance on one case (windows that end inside a tile)."""
    xh = _windows(5, 13)
    with torch.no_grad():
        p = models["xblk"](torch.from_numpy(xh).cuda())["poses"].cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in models["xblk"].state_dict().items()}
    ref = orc.pose_regressor(xh[:3], sd)["poses"]
    assert np.abs(p[:3] - ref).max() < TOL


def test_xb0_tile14_split_batch():
    """Two streams: with TIK_X_CHUNK=600 a 1024-window batch runs as a split
    chunk (two halves of 300 windows, each its own block-0 launch on its own
    stream) and an unsplit tail; the poses equal the one-stream layered path's."""
    split = _model_with_env(TIK_SPLIT=1, TIK_X_CHUNK=600)
    lay = _model_with_env(TIK_SPLIT=0, TIK_XBLK=0)
    x = torch.from_numpy(_windows(1024, 64)).cuda()
    with torch.no_grad():
        a = split(x)["poses"].clone()
        b = lay(x)["poses"].clone()
    assert torch.equal(a, b), float((a - b).abs().max())
