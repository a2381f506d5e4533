"""The online IK step against the float64 oracle on white-noise frames.

Every case runs OnlineIK(...).run(seq) on both steps, the dataflow kernel
(csrc/online.hip, TIK_ONLINE=1, path == "dataflow" asserted) and the layered
forward on the whole window (TIK_ONLINE=0, "layered" asserted), over a white
sequence of F = 2 W + 5 frames (W = 2 (win // 2) + 1; 70 frames at win 64): the
fill with its left clamp, more than one ring period in the steady state (both
launch parities at every ring slot) and the flush. White frames share nothing
with their neighbours, so a wrong ring slot, clamp or frame order is not
softened (tests/test_stream_oracle_host.py: each such mistake is 1e5 times the
bar).

Bar (tests/onlineref.py), per pose row i:

    max|gpu_i - f64_i|  <=  MARGIN * rel32 * max|f64_i|,   everything finite

rel32 the float32 oracle's own relative error for the same weights, window size
and layers on a calibration sequence (floored at 2^-23), MARGIN = 4
(tests/fwdblocks.py). It is relative, so it also holds the hostile weight sets,
whose poses reach 1e31, and it is a property of the reference alone.

Cases (onlineref.configs()): hop2/std on the IK net at win 3, 9, 21, 22, 23
(around the 22-frame receptive field of pose row 0, where n_in stops being
clamped by tin in plan_dataflow) and 64; every fwdblocks weight set at win 9 and
22 (hop3 and the random full matrix run the dense 17x17 amix read, hop2_signed
zero and negative edge importance, the hostile sets BatchNorms with gamma
negative or 0 and running_var over [1e-6, 1e2]; sparse or dense is asserted on
the host with fwdblocks.is_sparse); three more architectures at win 9 and 22 on
hop2/std: 48-channel first layers (C % 32 == 16), three stride-1 layers
(32, 32, 256), and (64 s2, 16, 16 s2, 256): a stride-2 first layer (the
residual conv from raw rows at 2 t) and a 16-channel identity block.
tik_model_create took all three as given and coverage() keeps all three on the
dataflow kernel, so no architecture was swapped for a neighbour. use_graph
everywhere, plus eager launches at win 9.

A layer with residual=False (ONR_ZERO in online.hip, RES_ZERO in the fold) is
unreachable from the model path: fold_backbone (csrc/fold.h) passes residual = 1
for every layer and refuses a state dict whose residual conv does not match
(cin, cout, stride). Only tik_block_create can make such a block, and a stream
takes a model handle. That branch is not run here.

Also: history independence (a stream reset and started j frames into a
sequence, j = 0..2W, returns bit for bit the poses of the j = 0 run once it has
seen W frames: every ring phase and both parities against the same arithmetic);
TIK_ONLINE_GRID 1 and 3 on dense/hostile (bit-equal to the default grid);
non-finite frames are refused by tik_stream_push and leave no trace.

Measured on an MI355X: the worst row's max|gpu_i - f64_i| over
rel32 * max|f64_i|, in the unit of MARGIN, per case and step. Every case passed
at 4 on both steps as first written; the largest is 2.16, nothing was widened
and no step disagrees with the oracle beyond rounding, so nothing points at the
fold or the weight upload the two steps share. (The float32 oracle itself, same
unit: up to 1.59.) The dataflow kernel is at or below the layered step in every
case but one (s2first at win 9, 0.82 against 0.79).

    weights / net            win   dataflow  layered | MARGIN
    hop2/std      ik           3     0.93     2.16   | 4
    hop2/std      ik           9     0.80     1.66   | 4
    hop2/std      ik          21     0.74     1.70   | 4
    hop2/std      ik          22     0.65     1.64   | 4
    hop2/std      ik          23     0.65     1.64   | 4
    hop2/std      ik          64     0.64     1.44   | 4
    hop3/std      ik           9     0.79     1.79   | 4
    hop3/std      ik          22     0.69     1.77   | 4
    dense/std     ik           9     0.62     1.30   | 4
    dense/std     ik          22     0.62     1.38   | 4
    hop2_signed   ik           9     0.62     1.35   | 4
    hop2_signed   ik          22     0.61     1.44   | 4
    hop2/hostile  ik           9     1.02     1.76   | 4
    hop2/hostile  ik          22     0.92     1.60   | 4
    dense/hostile ik           9     0.69     1.53   | 4
    dense/hostile ik          22     0.58     1.29   | 4
    hop2/std      c48          9     0.52     0.70   | 4
    hop2/std      c48         22     0.54     0.77   | 4
    hop2/std      s1x3         9     0.49     1.16   | 4
    hop2/std      s1x3        22     0.68     1.19   | 4
    hop2/std      s2first      9     0.82     0.79   | 4
    hop2/std      s2first     22     0.57     0.72   | 4
    hop2/std      ik, eager    9     0.80     1.66   | 4
    dense/hostile ik, grid 1   9     0.69      -     | 4
    dense/hostile ik, grid 3   9     0.69      -     | 4

The win 64 case costs about 5 s, nearly all of it the float64 oracle (rel32's
calibration sequence is 2 W + 5 = 135 windows of 65 frames); every other case
is under a second with its reference.
"""
import numpy as np
import pytest
import torch

import fwdblocks as fb
import onlineref as onl

pytestmark = pytest.mark.gpu

STEPS = {"dataflow": "1", "layered": "0"}
CONFIGS = onl.configs()
IDS = ["-".join(map(str, c)) for c in CONFIGS]

_models = {}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from temporal_inverse_kinematics_amd import _build
    _build.build()
    yield
    _models.clear()


def model(graph, kind, arch):
    """An IKPoseTrainer over ARCHS[arch] with the configuration's weights, loaded
    through the model classes (backbone.A included). One alive at a time."""
    key = (graph, kind, arch)
    if key not in _models:
        _models.clear()
        from temporal_inverse_kinematics_amd.models import IKPoseTrainer, PoseRegressor, default_hparams

        class Reg(PoseRegressor):
            LAYERS = onl.ARCHS[arch]

        class Trainer(IKPoseTrainer):
            def __init__(self, hp):
                torch.nn.Module.__init__(self)
                self.hparams = hp
                self.regressor = Reg(hp)

        m = Trainer(default_hparams(9))
        sd = onl.weights(graph, kind, arch)
        res = m.regressor.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)
        assert not [k for k in res.missing_keys if "num_batches_tracked" not in k] and not res.unexpected_keys, res
        _models[key] = m.cuda().eval()
    return _models[key]


def stream(monkeypatch, m, win, step, use_graph=True, grid=None):
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    monkeypatch.setenv("TIK_ONLINE", STEPS[step])
    if grid is None:
        monkeypatch.delenv("TIK_ONLINE_GRID", raising=False)
    else:
        monkeypatch.setenv("TIK_ONLINE_GRID", str(grid))
    s = OnlineIK(m, win_size=win, use_graph=use_graph)
    assert s.path == step and s.win_size == win
    return s


def check(cfg, got, tag):
    """got against the configuration's float64 reference at the per-row bar."""
    ref = onl.case_reference(*cfg)
    assert got.shape == ref.shape and got.dtype == np.float32
    ok, row, el, ratio = onl.compare(got, ref, onl.case_rel32(*cfg))
    print(f"ONLINE-ORACLE {'/'.join(map(str, cfg))} {tag}: {ratio:.2f}")
    assert ok, (f"{cfg} {tag}: pose row {row} of {ref.shape[0]}, element {el}: gpu {got[row, el]!r}, f64 {ref[row, el]!r}; "
                f"{ratio:.2f} x the float32 oracle's noise, the bar is {fb.MARGIN}")
    return ratio


@pytest.mark.parametrize("step", list(STEPS))
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_online_vs_oracle(cfg, step, monkeypatch):
    graph, kind, arch, win = cfg
    sd = onl.weights(graph, kind, arch)
    sparse = fb.SPARSE[graph]
    assert all(fb.is_sparse(sd, l) == sparse for l in range(len(onl.ARCHS[arch])))
    s = stream(monkeypatch, model(graph, kind, arch), win, step)
    seq = onl.case_sequence(win)
    got = s.run(seq)
    check(cfg, got, step)
    assert np.array_equal(s.run(seq), got)      # reset, and a second pass over the same ring


@pytest.mark.parametrize("step", list(STEPS))
def test_eager_launches(step, monkeypatch):
    cfg = ("hop2", "std", "ik", 9)
    m = model(*cfg[:3])
    got = stream(monkeypatch, m, 9, step, use_graph=False).run(onl.case_sequence(9))
    check(cfg, got, step + "-eager")
    assert np.array_equal(got, stream(monkeypatch, m, 9, step).run(onl.case_sequence(9)))


@pytest.mark.parametrize("step", list(STEPS))
def test_history_independence(step, monkeypatch):
    """win 9 (W = 9): a stream started at frame j of a 60-frame white sequence,
    j = 0..2W. From its push 2h on, the window holds only real frames, and the
    pose equals the j = 0 run's pose of the same frame bit for bit, whatever the
    ring slot and launch parity the frames landed on."""
    win, h = 9, 4
    W = 2 * h + 1
    seq = onl.white_sequence(60, 1)
    s = stream(monkeypatch, model("hop2", "std", "ik"), win, step)

    def pushes(j):
        s.reset()
        return [s.push(fr) for fr in seq[j:]]

    base = pushes(0)
    assert [p is None for p in base[:h + 1]] == [True] * h + [False]
    ref = onl.reference(onl.weights(), seq, win)
    got = np.stack(base[2 * h:])                         # poses of frames h .. 59 - h, all from whole windows
    ok, row, el, ratio = onl.compare(got, ref[h:60 - h], onl.case_rel32("hop2", "std", "ik", win))
    assert ok, (row, el, ratio)
    for j in range(1, 2 * W + 1):
        run = pushes(j)
        assert len(run) == 60 - j
        for q in range(2 * h, len(run)):                 # the run has seen W frames: j .. j + q
            assert np.array_equal(run[q], base[j + q]), (step, j, q)
        assert not np.array_equal(run[h], base[j + h])   # during the fill the clamp shows: another window


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_sizes(grid, monkeypatch):
    """Any number of workgroups runs every task in order: the dense, hostile set at
    one and three workgroups gives the default grid's poses bit for bit. (The
    layered step has no such grid; its dense/hostile case is in test_online_vs_oracle.)"""
    cfg = ("dense", "hostile", "ik", 9)
    m, seq = model(*cfg[:3]), onl.case_sequence(9)
    base = stream(monkeypatch, m, 9, "dataflow").run(seq)
    got = stream(monkeypatch, m, 9, "dataflow", grid=grid).run(seq)
    check(cfg, got, f"dataflow-grid{grid}")
    assert np.array_equal(got, base)


@pytest.mark.parametrize("step", list(STEPS))
def test_non_finite_frames_are_refused(step, monkeypatch):
    """A NaN and then an Inf offered at index 10: ValueError, naming the value; the
    frame is not appended, so every later pose is bit for bit that of a stream
    never offered them; flush does not repeat a refused frame; run() afterwards
    equals a fresh stream's."""
    m, seq = model("hop2", "std", "ik"), onl.case_sequence(9)
    clean = stream(monkeypatch, m, 9, step).run(seq)
    check(("hop2", "std", "ik", 9), clean, step + "-clean")
    s = stream(monkeypatch, m, 9, step)
    s.reset()
    out = []
    for i, fr in enumerate(seq):
        if i == 10:
            for bad, name in ((np.nan, "NaN"), (np.inf, "infinite"), (-np.inf, "infinite")):
                f = np.array(fr)
                f[5, 1] = bad
                f[16, 2] = np.nan                        # a later one: the first is named
                with pytest.raises(ValueError, match=rf"OnlineIK.push: tik_stream_push: frame value 16 \(joint 5, coordinate 1\) is {name}"):
                    s.push(f)
        p = s.push(fr)
        if p is not None:
            out.append(p)
    bad = np.full((17, 3), np.nan, np.float32)
    with pytest.raises(ValueError, match="frame value 0 "):
        s.push(bad)                                      # refused last: flush repeats the last frame the ring took
    out += s.flush()
    assert np.array_equal(np.stack(out), clean)
    assert np.array_equal(s.run(seq), clean)
