"""Validation, fit loop and resumable checkpoints of GpuTrainer on the GPU.

The eval pass (tik_trainer_eval: eval-mode BatchNorm folded on the device into
the trainer's fp32 GEMM operands) against the float64 oracle
(oracle/stgcn.py pose_regressor, pinned to the reference's model.npz) on the
synthetic weights, whose running statistics are not the batch statistics;
that it follows the live weights, leaves the training state untouched, and
gives a window the same poses whatever else is in the batch; the
multi-workgroup loss reduction; exact resume from a checkpoint; the epoch
loop and the command line.

Bounds: poses 1e-4 absolute (the project's standing IK bound), the loss 1e-5
relative to the float64 mean of (oracle poses - target)^2 (the train loss's
bound in test_gpu_train.py), the reduction alone 1e-6 relative; everything
about state and determinism is bitwise.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import stgcn as orc
from oracle import train as otr

pytestmark = pytest.mark.gpu

STRIDES = [s for _, _, s in otr.IK_LAYERS]
CKPT_RE = re.compile(r"^checkpoint_epoch=(\d+)-val_loss=(\d+\.\d\d)\.ckpt$")


@pytest.fixture(scope="module")
def lib():
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    return True


@pytest.fixture(scope="module")
def sd():
    from temporal_inverse_kinematics_amd import synthetic as syn
    return syn.ik_state_dict(orc.graph_A("coco", "uniform", 2, 1), seed=0)


def _model(sd, win=9):
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams
    m = IKPoseTrainer(default_hparams(win_size=win))
    own = m.regressor.state_dict()
    m.regressor.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k in own}, strict=False)
    return m


def _trainer(sd, lr=1e-4, win=9):
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    return GpuTrainer(_model(sd, win), lr=lr)


def _out_frames(T):
    for s in STRIDES:
        T = (T - 1) // s + 1
    return T


def _batch(N, T, seed):
    from temporal_inverse_kinematics_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    x = syn.synthetic_windows(N, T, seed=seed)
    tgt = rng.normal(0, 0.5, (N, _out_frames(T), 66)).astype(np.float32)
    return x, tgt


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np_state(tr):
    return {k: v.cpu().numpy() for k, v in tr.state_dict().items()}


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), what


def _same_trainers(a, b):
    """Weights, buffers, counters, both Adam moments and steps, bitwise."""
    assert a.steps == b.steps
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        _same(sa[k].cpu(), sb[k].cpu(), k)
    for k in otr.param_names():
        for what in ("exp_avg", "exp_avg_sq"):
            _same(a.tensor(k, what), b.tensor(k, what), (k, what))


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("N,T", [(1, 1), (1, 9), (8, 9), (5, 17), (3, 64), (2, 65)])
def test_eval_vs_oracle(lib, sd, N, T):
    tr = _trainer(sd, win=T)
    x, tgt = _batch(N, T, seed=100 + T + N)
    ref = orc.pose_regressor(x, sd)["poses"]
    got = tr.predict(_cuda(x))["poses"]
    assert tuple(got.shape) == (N, _out_frames(T), 66)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
    print(f"eval ({N},{T}): max |poses - oracle| = {err:.3e}")
    assert err <= 1e-4
    out = tr.validation_step({"keypoints_3d": _cuda(x), "poses": _cuda(tgt)}, 0)
    assert out["val_loss"] is out["pose_mse"] and out["val_loss"].is_cuda and out["val_loss"].dim() == 0
    want = np.mean((ref.astype(np.float64) - tgt.astype(np.float64)) ** 2)
    print(f"eval ({N},{T}): loss {float(out['val_loss']):.9g} vs oracle {want:.9g}")
    np.testing.assert_allclose(float(out["val_loss"]), want, rtol=1e-5)
    assert tr.steps == 0


# ------------------------------------------------------------------ 2. the current weights
def test_eval_sees_current_weights(lib, sd):
    tr = _trainer(sd, lr=1e-3)
    x, tgt = _batch(8, 9, seed=21)
    xe, _ = _batch(4, 9, seed=22)
    before = tr.predict(_cuda(xe))["poses"].cpu().numpy()
    for i in range(3):
        tr.step(_cuda(x), _cuda(tgt), seed=i)
    after = tr.predict(_cuda(xe))["poses"].cpu().numpy()
    ref = orc.pose_regressor(xe, _np_state(tr))["poses"]
    assert np.abs(after.astype(np.float64) - ref).max() <= 1e-4
    assert np.abs(after - before).max() > 1e-3          # a stale fold would repeat `before`
    # one weight tensor written from outside: derived layouts and the eval set follow
    name = "backbone.st_gcn_networks.3.gcn.conv.weight"
    tr.write_tensor(name, tr.tensor(name) * 1.5)
    written = tr.predict(_cuda(xe))["poses"].cpu().numpy()
    ref = orc.pose_regressor(xe, _np_state(tr))["poses"]
    assert np.abs(written.astype(np.float64) - ref).max() <= 1e-4
    assert np.abs(written - after).max() > 1e-3
    # ... and a running statistic (a buffer)
    name = "backbone.st_gcn_networks.0.tcn.0.running_var"
    tr.write_tensor(name, tr.tensor(name) * 4.0)
    again = tr.predict(_cuda(xe))["poses"].cpu().numpy()
    ref = orc.pose_regressor(xe, _np_state(tr))["poses"]
    assert np.abs(again.astype(np.float64) - ref).max() <= 1e-4
    assert np.abs(again - written).max() > 1e-3
    # ... and a dense adjacency (outside the COCO hop<=2 pattern the sparse graph mix unrolls)
    A = tr.tensor("backbone.A")
    tr.write_tensor("backbone.A", 0.5 * A + 0.01)
    dense = tr.predict(_cuda(xe))["poses"].cpu().numpy()
    ref = orc.pose_regressor(xe, _np_state(tr))["poses"]
    assert np.abs(dense.astype(np.float64) - ref).max() <= 1e-4


# ------------------------------------------------------------------ 3. read-only
def test_eval_is_read_only(lib, sd):
    a, b = _trainer(sd, lr=1e-3), _trainer(sd, lr=1e-3)
    x, tgt = _batch(8, 9, seed=31)
    xe, te = _batch(3, 17, seed=32)
    la, lb = [], []
    la.append(a.step(_cuda(x), _cuda(tgt), seed=7))
    lb.append(b.step(_cuda(x), _cuda(tgt), seed=7))
    O0 = a.saved("O", 0, (8, 9, 17, 64)).clone()
    a.validation_step({"keypoints_3d": _cuda(xe), "poses": _cuda(te)}, 0)
    a.predict(_cuda(xe))
    _same(a.saved("O", 0, (8, 9, 17, 64)), O0, "saved O after eval")
    assert a.steps == 1
    la.append(a.step(_cuda(x), _cuda(tgt), seed=8))
    lb.append(b.step(_cuda(x), _cuda(tgt), seed=8))
    for p, q in zip(la, lb):
        _same(p, q, "loss")
    ga, gb = a.grads(), b.grads()
    for k in ga:
        _same(ga[k], gb[k], k)
    _same_trainers(a, b)


# ------------------------------------------------------------------ 4. batch invariance, determinism
def test_eval_batch_invariant_and_deterministic(lib, sd):
    tr = _trainer(sd)
    x40, t40 = _batch(40, 9, seed=41)
    at = [3, 17, 22, 30, 39]
    x5 = np.ascontiguousarray(x40[at])
    p5 = tr.predict(_cuda(x5))["poses"]
    for j in range(5):
        _same(tr.predict(_cuda(x5[j:j + 1]))["poses"][0], p5[j], f"window {j} alone")
    p40 = tr.predict(_cuda(x40))["poses"]
    for j, i in enumerate(at):
        _same(p40[i], p5[j], f"window {j} inside 40")
    batch = {"keypoints_3d": _cuda(x40), "poses": _cuda(t40)}
    l0 = tr.validation_step(batch, 0)["val_loss"]
    l1 = tr.validation_step(batch, 0)["val_loss"]
    assert l0.data_ptr() != l1.data_ptr()
    _same(l0, l1, "val_loss")


# ------------------------------------------------------------------ 5. the reduction at size
def test_eval_loss_reduction_many_workgroups(lib, sd):
    tr = _trainer(sd, win=1)
    x, tgt = _batch(2048, 1, seed=51)
    poses = tr.predict(_cuda(x))["poses"].cpu().numpy().astype(np.float64)
    want = np.mean((poses - tgt.astype(np.float64)) ** 2)
    got = float(tr.validation_step({"keypoints_3d": _cuda(x), "poses": _cuda(tgt)}, 0)["val_loss"])
    print(f"mse over {poses.size} elements: {got:.9g} vs float64 {want:.9g}")
    np.testing.assert_allclose(got, want, rtol=1e-6)


# ------------------------------------------------------------------ 6. resume
def test_resume_is_exact(lib, sd, tmp_path):
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer
    from temporal_inverse_kinematics_amd.trainer import GpuTrainer
    batches = [{"keypoints_3d": _cuda(x), "poses": _cuda(t)} for x, t in (_batch(8, 9, seed=60 + i) for i in range(4))]
    a = _trainer(sd, lr=1e-3)
    la = [a.training_step(batches[i], i)["loss"] for i in range(4)]
    b = _trainer(sd, lr=1e-3)
    for i in range(2):
        b.training_step(batches[i], i)
    path = b.save_checkpoint(tmp_path / "two.ckpt", epoch=5)
    c = GpuTrainer.from_checkpoint(path)
    assert c.steps == 2 and c.lr == 1e-3
    lc = [c.training_step(batches[i], i)["loss"] for i in (2, 3)]
    _same(lc[0], la[2], "loss 3")
    _same(lc[1], la[3], "loss 4")
    _same_trainers(a, c)
    assert int(c.state_dict()["backbone.data_bn.num_batches_tracked"]) == 4

    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["epoch"] == 5 and ck["global_step"] == 2 and isinstance(ck["hparams"], dict)
    assert "regressor.backbone.data_bn.num_batches_tracked" in ck["state_dict"]
    m = IKPoseTrainer.load_from_checkpoint(path)
    _same(m.regressor.state_dict()["pose_regressor.3.weight"], b.tensor("pose_regressor.3.weight").cpu(), "weights")
    names = otr.param_names()
    assert [n for n, _ in m.regressor.named_parameters()] == names
    params = [torch.nn.Parameter(torch.zeros(tuple(b.tensor(n).shape))) for n in names]
    opt = torch.optim.Adam(params)
    opt.load_state_dict(ck["optimizer_states"][0])
    assert opt.param_groups[0]["lr"] == 1e-3
    for p, n in zip(params, names):
        _same(opt.state[p]["exp_avg"], b.tensor(n, "exp_avg").cpu(), n)
        _same(opt.state[p]["exp_avg_sq"], b.tensor(n, "exp_avg_sq").cpu(), n)
        assert float(opt.state[p]["step"]) == 2.0

    del ck["optimizer_states"]
    torch.save(ck, tmp_path / "weights_only.ckpt")
    w = GpuTrainer.from_checkpoint(tmp_path / "weights_only.ckpt")
    assert w.steps == 0
    for n in names[:3] + names[-2:]:
        assert not w.tensor(n, "exp_avg").any() and not w.tensor(n, "exp_avg_sq").any()
    _same(w.tensor("pose_regressor.0.weight"), b.tensor("pose_regressor.0.weight"), "weights of a weights-only file")


# ------------------------------------------------------------------ 7. fit
def _sequences(lens, seed=0):
    """As tests/test_gpu_train_data.py builds them."""
    rng = np.random.default_rng(seed)
    out = []
    for i, F in enumerate(lens):
        t = np.linspace(0, 2 * np.pi, F, dtype=np.float32)[:, None]
        base = rng.normal(0, 0.3, (1, 156)).astype(np.float32)
        amp = rng.normal(0, 0.2, (1, 156)).astype(np.float32)
        poses = (base + amp * np.sin(t + i)).astype(np.float32)
        out.append({"poses": poses, "betas": rng.normal(0, 1, 10).astype(np.float32),
                    "gender": ["male", "female", "neutral"][i % 3]})
    return out


@pytest.fixture(scope="module")
def smplx(lib):
    from temporal_inverse_kinematics_amd.smplx_fk import load_smplx_models
    return load_smplx_models(None, "cuda", 9)


def _datasets(smplx):
    from temporal_inverse_kinematics_amd.training_data import AmassDataset
    return (AmassDataset(smplx, _sequences([40, 50, 45]), 9, "coco"),
            AmassDataset(smplx, _sequences([30, 35], seed=1), 9, "coco"))


@pytest.fixture(scope="module")
def full_run(lib, sd, smplx, tmp_path_factory):
    """The uninterrupted 3-epoch run the fit tests compare against."""
    d = tmp_path_factory.mktemp("full")
    tr = _trainer(sd, lr=1e-3)
    train, val = _datasets(smplx)
    hist = tr.fit(train, val, max_epochs=3, batch_size=32, ckpt_dir=d)
    return tr, hist, d


def test_fit_writes_checkpoints_and_history(full_run):
    tr, hist, d = full_run
    files = sorted(os.listdir(d))
    assert len(files) == 3 and all(CKPT_RE.match(f) for f in files), files
    assert [r["epoch"] for r in hist] == [0, 1, 2]
    for r in hist:
        assert set(r) == {"epoch", "train/pose_mse", "val_loss", "ckpt"}
        assert np.isfinite(r["train/pose_mse"]) and np.isfinite(r["val_loss"])
        assert os.path.basename(r["ckpt"]) == f"checkpoint_epoch={r['epoch']}-val_loss={r['val_loss']:.2f}.ckpt"
        assert os.path.exists(r["ckpt"])
    assert tr.steps == 3 * 5                              # 135 windows in batches of 32


def test_fit_keeps_top_k(lib, sd, smplx, full_run, tmp_path):
    _, ref_hist, _ = full_run
    tr = _trainer(sd, lr=1e-3)
    train, val = _datasets(smplx)
    hist = tr.fit(train, val, max_epochs=3, batch_size=32, ckpt_dir=tmp_path, save_top_k=2)
    assert [r["val_loss"] for r in hist] == [r["val_loss"] for r in ref_hist]
    best = sorted(hist, key=lambda r: (r["val_loss"], r["epoch"]))[:2]
    want = sorted(f"checkpoint_epoch={r['epoch']}-val_loss={r['val_loss']:.2f}.ckpt" for r in best)
    assert sorted(os.listdir(tmp_path)) == want


def test_fit_resume_is_exact(lib, sd, smplx, full_run, tmp_path):
    ref, ref_hist, _ = full_run
    tr = _trainer(sd, lr=1e-3)
    train, val = _datasets(smplx)
    h1 = tr.fit(train, val, max_epochs=1, batch_size=32, ckpt_dir=tmp_path)
    assert len(h1) == 1 and {k: v for k, v in h1[0].items() if k != "ckpt"} == \
        {k: v for k, v in ref_hist[0].items() if k != "ckpt"}
    tr2 = _trainer(sd, lr=1e-3)                           # a fresh process would start like this
    train, val = _datasets(smplx)
    h2 = tr2.fit(train, val, max_epochs=3, batch_size=32, ckpt_dir=tmp_path, resume_ckpt=h1[0]["ckpt"], save_top_k=2)
    assert [r["epoch"] for r in h2] == [1, 2]
    for r, q in zip(h2, ref_hist[1:]):
        assert r["train/pose_mse"] == q["train/pose_mse"] and r["val_loss"] == q["val_loss"]
    _same_trainers(ref, tr2)
    # the interrupted run's file counts toward save_top_k: the two best of all three epochs stay
    best = sorted(ref_hist, key=lambda r: (r["val_loss"], r["epoch"]))[:2]
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(r["ckpt"]) for r in best)


def test_fit_without_validation_set(lib, sd, smplx, tmp_path):
    tr = _trainer(sd, lr=1e-3)
    train, _ = _datasets(smplx)
    hist = tr.fit(train, None, max_epochs=1, batch_size=64, ckpt_dir=tmp_path)
    assert hist[0]["val_loss"] == hist[0]["train/pose_mse"] and len(os.listdir(tmp_path)) == 1


def test_validation_epoch_end_is_mean_of_batch_means(lib, sd, smplx):
    from temporal_inverse_kinematics_amd.trainer import calc_mean_losses
    tr = _trainer(sd)
    _, val = _datasets(smplx)
    n = len(val)
    outs = [tr.validation_step(val.get_batch(np.arange(lo, min(lo + 32, n))), b)
            for b, lo in enumerate(range(0, n, 32))]
    assert len(outs) == 3
    end = tr.validation_epoch_end(outs)
    want = calc_mean_losses(outs, ["pose_mse", "val_loss"])
    _same(end["val_loss"], want["val_loss"], "val_loss")
    assert set(end) == {"val_loss", "log"} and set(end["log"]) == {"val/pose_mse", "val/val_loss"}
    _same(end["log"]["val/pose_mse"], want["pose_mse"], "pose_mse")
    mean = np.mean([float(o["val_loss"]) for o in outs])
    np.testing.assert_allclose(float(end["val_loss"]), mean, rtol=1e-6)
    _same(tr.validate(val, 32)["val_loss"], end["val_loss"], "validate")


# ------------------------------------------------------------------ 8. command line
def test_run_train_cli(lib, tmp_path):
    from temporal_inverse_kinematics_amd.trainer import run_train
    paths = []
    for i, s in enumerate(_sequences([40, 36], seed=3)):
        p = tmp_path / f"seq{i}.npz"
        np.savez(p, poses=s["poses"], betas=s["betas"], gender=np.array(s["gender"]))
        paths.append(str(p))
    (tmp_path / "train.csv").write_text("\n".join(paths) + "\n")
    (tmp_path / "valid.csv").write_text(paths[1] + "\n")
    rng = np.random.default_rng(4)
    np.savez(tmp_path / "smplx_shapes.npz", betas=rng.normal(0, 1, (3, 10)).astype(np.float32),
             genders=np.array(["male", "female", "neutral"]))
    rc = run_train(["--amass", str(tmp_path), "--data_dir", str(tmp_path), "--max_epoch", "1", "--bs", "32",
                    "--win_size", "9", "--synthetic_smplx"])
    assert rc == 0
    files = os.listdir(tmp_path / "model_ckps")
    assert len(files) == 1 and CKPT_RE.match(files[0]), files


# ------------------------------------------------------------------ 9. errors
def test_eval_and_restore_errors(lib, sd):
    from temporal_inverse_kinematics_amd import _lib
    tr = _trainer(sd)
    x, tgt = _batch(4, 9, seed=91)
    with pytest.raises(ValueError, match="target poses"):
        tr.validation_step({"keypoints_3d": _cuda(x), "poses": _cuda(tgt[:, :, :65])}, 0)
    with pytest.raises(ValueError, match="target poses"):
        tr.evaluate(_cuda(x), _cuda(tgt[:3]))
    with pytest.raises(RuntimeError, match="GPU only"):
        tr.predict(torch.from_numpy(x))
    with pytest.raises(RuntimeError, match="GPU only"):
        tr.evaluate(_cuda(x), torch.from_numpy(tgt))
    with pytest.raises(ValueError, match="keypoints"):
        tr.predict(_cuda(x[:, :, :16]))
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            tr.predict(_cuda(x).to(dt))
        with pytest.raises(TypeError, match="float32"):
            tr.evaluate(_cuda(x), _cuda(tgt).to(dt))
        with pytest.raises(TypeError, match="float32"):
            tr.write_tensor("pose_regressor.3.bias", torch.zeros(66, device="cuda", dtype=dt))
    lib_ = _lib.load()
    i = tr._index["backbone.data_bn.running_mean"]
    src = torch.zeros(51, device="cuda")
    with pytest.raises(ValueError, match="is a buffer"):
        _lib.check(lib_.tik_trainer_write(tr._h.h, i, 2, src.data_ptr(), None))
    with pytest.raises(ValueError, match="is a buffer"):
        tr.write_tensor("backbone.data_bn.running_mean", src, "exp_avg")
    with pytest.raises(ValueError, match="steps must be >= 0"):
        _lib.check(lib_.tik_trainer_set_steps(tr._h.h, -1))
    assert tr.steps == 0
    with pytest.raises(ValueError, match="without a target"):
        out = torch.zeros((), device="cuda")
        _lib.check(lib_.tik_trainer_eval(tr._h.h, _cuda(x).data_ptr(), 4, 9, None, None, out.data_ptr(), None))
