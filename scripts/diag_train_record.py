"""A record of what the trainer's C ABI computes, for comparing two builds of
libtik.so bit for bit (TIK_LIB selects the library; run each in a fresh process
and diff the two outputs). One line per record, each the sha256 of the bytes.

On one handle with fixed seeds: the entry names; three steps at (8,9) with a
given dropout mask, three at (3,64) with the seeded device mask, one more at
(8,9) (the workspace grows, then is reused), steps at (1,2) and (5,1). The loss
of every step; after each group every entry's value, gradient, exp_avg and
exp_avg_sq, and the saved activations 0 and 2..6 of blocks 0, 2 and 7. Then
tik_trainer_eval's poses and loss at (4,9) and (2,17), and again after a
tik_trainer_write of a dense backbone.A. Then a second handle with the three
synthetic body models and kp_weight 0.5 (tik_trainer_step_kp): two steps at (8,9)
against FK keypoints of the target poses, mixed genders; the loss, both of its
terms (last_loss_parts) and the state after them.

    python scripts/diag_train_record.py > record.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temporal_inverse_kinematics_amd import synthetic as syn  # noqa: E402
from temporal_inverse_kinematics_amd.models import IKPoseTrainer, default_hparams  # noqa: E402
from temporal_inverse_kinematics_amd.smplx_fk import load_smplx_models  # noqa: E402
from temporal_inverse_kinematics_amd.trainer import GpuTrainer  # noqa: E402

V = 17


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).tobytes())
    return h.hexdigest()


def main():
    m = IKPoseTrainer(default_hparams(win_size=9))
    sd = syn.ik_state_dict(m.regressor.backbone.graph.A, seed=0)
    own = m.regressor.state_dict()
    m.regressor.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if k in own}, strict=False)
    tr = GpuTrainer(m, lr=1e-3)
    layers = [(ci, co, s) for (ci, co, _), s in zip(syn.IK_LAYERS, m.regressor.backbone.strides)]
    print(f"names {len(tr._names)} {hashlib.sha256(chr(10).join(n for n, _, _ in tr._names).encode()).hexdigest()}")
    rng = np.random.default_rng(7)

    def frames(T):
        out = []
        for _, _, s in layers:
            out.append((T, (T - 1) // s + 1))
            T = out[-1][1]
        return out

    def batch(N, T):
        x = torch.from_numpy(syn.synthetic_windows(N, T, seed=100 * N + T)).cuda()
        y = torch.from_numpy(rng.normal(0, 0.5, (N, frames(T)[-1][1], 66)).astype(np.float32)).cuda()
        return x, y

    def state(tag, N, T, tr=tr):
        for what in ("value", "grad", "exp_avg", "exp_avg_sq"):
            print(f"{tag} state {what} {sha(*[tr.tensor(n, what) for n, _, k in tr._names if k == 0 or what == 'value'])}")
        fr = frames(T)
        for l in (0, 2, 7):
            co, (tin, tout) = layers[l][1], fr[l]
            for kind in ("O", "U", "H", "Z", "Y", "P"):
                shape = (N * fr[-1][1], 512) if kind == "P" else (N, tout if kind in "OU" else tin, V, co)
                print(f"{tag} saved layer {l} {kind} {sha(tr.saved(kind, l, shape))}")

    def steps(tag, N, T, n, given_mask):
        x, y = batch(N, T)
        for i in range(n):
            mask = None
            if given_mask:
                mask = torch.from_numpy((rng.random((N * frames(T)[-1][1], 512)) < 0.3).astype(np.float32)).cuda()
            loss = tr.step(x, y, dropout_mask=mask, seed=17 * N + i)
            print(f"{tag} step {tr.steps} loss {sha(loss)} {float(loss)!r}")
        state(tag, N, T)

    def evals(tag):
        for N, T in ((4, 9), (2, 17)):
            x, y = batch(N, T)
            poses, loss = tr.evaluate(x, y)
            print(f"{tag} eval ({N},{T}) poses {sha(poses)} loss {sha(loss)} {float(loss)!r}")

    steps("A (8,9) given mask", 8, 9, 3, True)
    steps("B (3,64) seeded mask", 3, 64, 3, False)
    steps("C (8,9) again", 8, 9, 1, True)
    steps("D (1,2)", 1, 2, 1, False)
    steps("E (5,1)", 5, 1, 1, False)
    evals("F")
    A = torch.from_numpy(rng.uniform(0.0, 0.2, (1, V, V)).astype(np.float32)).cuda()   # dense: leaves the hop <= 2 pattern
    tr.write_tensor("backbone.A", A)
    evals("G dense A")

    bodies = load_smplx_models("synthetic", "cuda", batch_size=8)
    trk = GpuTrainer(m, lr=1e-3, smplx_models=bodies, kp_weight=0.5)
    N, T = 8, 9
    To = frames(T)[-1][1]
    x, y = batch(N, T)
    gid = torch.from_numpy(rng.integers(0, 3, N).astype(np.int32))
    betas = torch.from_numpy(rng.normal(0, 1, (N, bodies["male"].num_betas)).astype(np.float32)).cuda()
    full = torch.zeros((N * To, 55, 3), device="cuda")
    full[:, :22] = y.reshape(N * To, 22, 3)
    rb = betas.repeat_interleave(To, 0).contiguous()
    kps = torch.zeros((N * To, V, 3), device="cuda")
    for g, name in enumerate(sorted(bodies)):
        sel = torch.nonzero(gid.cuda().repeat_interleave(To) == g).flatten()
        if len(sel):
            kps[sel] = bodies[name].joints(full[sel], rb[sel].contiguous(), select="coco")
    for i in range(2):
        loss = trk.step(x, y, seed=40 + i, target_keypoints=kps.reshape(N, To, V, 3), betas=betas, gender_id=gid)
        parts = trk.last_loss_parts
        print(f"H kp (8,9) step {trk.steps} loss {sha(loss)} {float(loss)!r} parts {sha(parts)} {parts.tolist()!r}")
    state("H kp (8,9)", N, T, trk)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
