"""The float64 training oracle (oracle.train with dtype=torch.float64) pinned to
the fp32 one, which tests/test_oracle.py pins to the reference's own run
(tests/golden/train.npz). CPU only.

Both run one step on the same batch with the float64 run's ReLU / LeakyReLU
branches (oracle.train.branches), so what separates them is fp32 rounding
alone. Measured here (per-tensor max error relative to max|g|, the worst
tensor): (3,16) 1.4e-5, (8,9) 1.9e-5, (2,1) 3.6e-5, (1,2) 1.0e-4. The bound
for the two window-9 batches below is 4 x the (8,9) figure, the headroom for
another CPU's summation order; the loss agrees to 1e-6 relative. The biases
in front of a train-mode BatchNorm hold rounding noise only (their float64
gradient is ~1e-17): both below 1e-5 absolute, as in test_gpu_train.py."""
import numpy as np
import pytest
import torch

import trainref as tref
from conftest import golden
from oracle import train as otr

REF_ERR_T9 = 1.9e-5      # the (8,9) row of the table above
HEADROOM = 4.0


def _batches():
    g = golden("train.npz")
    yield "golden", (g["x"][0], g["target"][0], g["mask"][0])
    yield "(8,9,11)", tref.batch(8, 9, 11)


@pytest.mark.parametrize("tag", ["golden", "(8,9,11)"])
def test_float64_oracle_agrees_with_fp32(ik_weights, tag):
    x, tgt, mask = dict(_batches())[tag]
    br = otr.branches(ik_weights, x, mask, dtype=torch.float64)
    l64, g64, s64 = otr.train_steps(ik_weights, [(x, tgt, mask)], relu_masks=br, dtype=torch.float64)
    l32, g32, s32 = otr.train_steps(ik_weights, [(x, tgt, mask)], relu_masks=br)
    assert all(v.dtype == np.float64 for v in g64.values()) and all(v.dtype == np.float32 for v in g32.values())
    # the branches handed in are the float64 run's own: its natural step's gradients, to float64 rounding
    _, g64n, _ = otr.train_steps(ik_weights, [(x, tgt, mask)], dtype=torch.float64)
    for k in g64:
        assert np.abs(g64[k] - g64n[k]).max() <= 1e-11 * max(np.abs(g64n[k]).max(), 1e-3), k
    print(f"\n{tag}: loss fp32 {l32[0]:.9g} float64 {l64[0]:.12g} rel {abs(l32[0] - l64[0]) / l64[0]:.2e}")
    assert abs(l32[0] - l64[0]) <= 1e-6 * l64[0]
    worst = 0.0
    for k in otr.param_names():
        if k.endswith(tref.ZERO_GRAD):
            print(f"  {k}: zero-gradient bias, max|g64| {np.abs(g64[k]).max():.1e} max|g32| {np.abs(g32[k]).max():.1e}")
            assert np.abs(g64[k]).max() <= 1e-5 and np.abs(g32[k]).max() <= 1e-5, k
            continue
        E, _ = tref.tensor_error(g32[k], g64[k])
        e, _ = tref.slice_errors(k, g32[k], g64[k])
        n = np.linalg.norm(tref.slices(k, g64[k]), axis=1)
        rel = E / np.abs(g64[k]).max()
        worst = max(worst, rel)
        print(f"  {k}: max err / max|g| {rel:.2e}; worst slice L2 err / slice norm "
              f"{(e[n > 0] / n[n > 0]).max(initial=0):.2e}")
        assert rel <= HEADROOM * REF_ERR_T9, (k, rel)
    print(f"  worst tensor {worst:.2e} (bound {HEADROOM * REF_ERR_T9:.1e})")
    for k, v in s64.items():
        if "running" in k:
            np.testing.assert_allclose(s32[k], v, rtol=1e-5, atol=1e-6, err_msg=k)
