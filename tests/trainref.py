"""Helpers shared by the training-step tests (test_gpu_train.py,
test_gpu_train_adam.py, test_train_oracle64_host.py): the seeded batch of a
shape, and the two error metrics of a gradient against the float64 oracle's.
Not a test module (pytest does not collect it)."""
import numpy as np

from oracle import train as otr

U = 2.0 ** -24                              # float32 unit roundoff
ZERO_GRAD = ("tcn.2.bias", "residual.0.bias")
STRIDES = [s for _, _, s in otr.IK_LAYERS]


def frames(T):
    """Frames entering layer 0 .. 7 and leaving layer 7."""
    t = [T]
    for s in STRIDES:
        t.append((t[-1] - 1) // s + 1)
    return t


def weights(seed=0):
    """The seeded PoseRegressor state dict (numpy)."""
    from oracle import stgcn as orc
    from temporal_inverse_kinematics_amd import synthetic as syn
    return syn.ik_state_dict(orc.graph_A("coco", "uniform", 2, 1), seed=seed)


def model(sd, win):
    """An IKPoseTrainer holding the state dict `sd`."""
    import torch
    from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams
    m = IKPoseTrainer(default_hparams(win_size=win))
    own = m.regressor.state_dict()
    m.regressor.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k in own}, strict=False)
    return m


def batch(N, T, seed):
    """(x (N,T,17,3), target (N,T',66), dropout mask (N*T',512)) fp32, seeded."""
    from temporal_inverse_kinematics_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    x = syn.synthetic_windows(N, T, seed=seed)
    Tp = frames(T)[-1]
    tgt = rng.normal(0, 0.5, (N, Tp, 66)).astype(np.float32)
    mask = (rng.random((N * Tp, 512)) < 0.3).astype(np.float32)
    return x, tgt, mask


def slices(name, a):
    """(number of slices, -1) view of a gradient: pose_regressor.*.weight by row,
    conv weights by output channel (dim 0 of every tensor with ndim >= 2);
    edge_importance.{i} and every vector as one slice."""
    a = np.asarray(a, np.float64)
    if a.ndim >= 2 and "edge_importance" not in name:
        return a.reshape(a.shape[0], -1)
    return a.reshape(1, -1)


def tensor_error(g, g64):
    """E = max|g - g64| and its floor F = u * max|g64| (the float32 resolution of
    the largest element: it matters only where the other side is exact)."""
    g64 = np.asarray(g64, np.float64)
    return float(np.abs(np.asarray(g, np.float64) - g64).max()), U * float(np.abs(g64).max())


def slice_errors(name, g, g64):
    """e(s) = ||g[s] - g64[s]||_2 per slice and the floor F_s = u * ||g64||_2 of
    the whole tensor / sqrt(number of slices)."""
    a, r = slices(name, g), slices(name, g64)
    return np.linalg.norm(a - r, axis=1), U * float(np.linalg.norm(r)) / np.sqrt(r.shape[0])
