"""Host test of the online-IK comparator (tests/onlineref.py), on the oracle's own
arrays: the per-row bar of tests/test_gpu_stream_oracle.py passes what is right and
fails what is subtly wrong.

1. online_window is the reference's own window (orc.inference_item) wherever that
   gives one, the ring of ring_windows gives the same windows push by push, and
   reference() is orc.run_inference for the default layers, bit for bit.
2. The float32 oracle passes compare at MARGIN on every configuration of the GPU
   test (weight set or architecture, window size), on the case's own sequence.
3. Each indexing mistake, applied in numpy to the windows before the float64
   oracle, fails compare on every configuration: two ring slots swapped, the left
   clamp off by one, the root from joints 11 and 11. The newest frame replaced by
   the previous one fails wherever the pose reads the newest frame at all: pose
   row 0 reads the first field() window positions only (22 for the IK net, 4 and 10
   for the two short nets), so at W = 2h+1 above that the pushed frame is stored
   for later poses and not read by this one. There the mistake is asserted to move
   nothing (what the dataflow step relies on); the swapped slots and the clamp are
   the indexing checks that bite at every size.
4. The newest frame read from two bf16 planes instead of three stays INSIDE the
   bar on every configuration, so it is not asserted to fail anywhere: one frame of
   up to 23 contributes 2^-17 of its values, and through eight layers and the head
   that is below the float32 oracle's own noise. From one plane it fails at win 3
   and 9 wherever the newest frame is read (the comparator does see a precision
   loss of one frame, from 2^-9 on).

Measured (error over the float32 oracle's noise, the unit of MARGIN = 4):
2. at most 1.59 (hop2/std win 9). 3. swapped slots 2.0e5 to 8.2e5, clamp 9.1e4 to
7.1e5, root 1.4e5 to 1.0e6, newest-is-previous 298 (win 21) to 3.4e5 where read,
below 2e-9 where not. 4. two planes 1.01 at win 3, 0.06 to 0.50 at win 9, below
1e-3 from win 21 on; one plane 542 at win 3, 52 to 177 at win 9.
"""
import numpy as np
import pytest

import fwdblocks as fb
import onlineref as onl
from oracle import stgcn as orc

CONFIGS = onl.configs()
IDS = ["-".join(map(str, c)) for c in CONFIGS]


def _rows(win):
    """The poses an injection is evaluated on: the fill (clamp), the first steady
    pushes, a row one ring period on (slot 0 at window position 0) and the flush."""
    h = win // 2
    W, F = 2 * h + 1, onl.case_frames(win)
    return sorted(r for r in {0, 1, h, h + 1, h + W, h + W + 1, F - 1} if r < F)


def _injected(cfg, inject):
    graph, kind, arch, win = cfg
    rows = _rows(win)
    xs = onl.ring_windows(onl.case_sequence(win), win // 2, rows, inject)
    got = onl.poses_of_windows(onl.weights(graph, kind, arch), xs, onl.ARCHS[arch])
    return onl.compare(got, onl.case_reference(*cfg)[rows], onl.case_rel32(*cfg), rows)


def _reads_newest(cfg):
    return 2 * (cfg[3] // 2) + 1 <= onl.field(onl.ARCHS[cfg[2]])


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("win,F", [(3, 11), (9, 23), (9, 9), (22, 51), (22, 23), (9, 5), (22, 14)])
def test_online_window_is_the_oracles_window(win, F):
    """F >= W: every frame. Shorter sequences, which the stream accepts: the oracle
    raises for some frames and returns a truncated window for others (its slice
    runs past the padded end); where it gives a whole window, that one."""
    seq, h = onl.white_sequence(F, 3), win // 2
    whole = 0
    for i in range(F):
        try:
            w = orc.inference_item(seq, i, win)
        except ValueError:
            assert F < 2 * h + 1
            continue
        mine = onl.online_window(seq, i, h)
        assert mine.shape == (2 * h + 1, onl.V, 3) and mine.dtype == np.float32
        if w.shape[0] < 2 * h + 1:
            assert F < 2 * h + 1
            continue
        whole += 1
        assert np.array_equal(mine, w), (win, F, i)
    assert whole == F or F < 2 * h + 1
    assert whole > 0


@pytest.mark.parametrize("win,F", [(3, 11), (9, 23), (22, 51), (9, 5), (2, 1)])
def test_ring_gives_the_same_windows(win, F):
    seq, h = onl.white_sequence(F, 4), win // 2
    want = np.stack([onl.online_window(seq, i, h) for i in range(F)])
    assert np.array_equal(onl.ring_windows(seq, h), want)
    assert np.array_equal(onl.ring_windows(seq, h, rows=[F - 1, 0]), want[[F - 1, 0]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_is_run_inference(dtype):
    sd = onl.weights()
    for win, F in ((9, 70), (22, 30)):
        seq = onl.white_sequence(F, 5)
        assert np.array_equal(onl.reference(sd, seq, win, dtype=dtype), orc.run_inference(seq, sd, win, dtype=dtype))
    assert np.array_equal(onl.case_reference("hop2", "std", "ik", 9), orc.run_inference(onl.case_sequence(9), sd, 9))


def test_sequences_fields_and_adjacencies():
    """White frames share nothing (adjacent frames as far apart as any two); the
    calibration sequence is none of the test sequences; field() of the nets; each
    weight set's mix is what fwdblocks says."""
    s = onl.case_sequence(22)
    assert s.shape == (51, 17, 3) and s.dtype == np.float32 and abs(float(s.std()) - 0.3) < 0.02
    assert np.abs(s[1:] - s[:-1]).mean() > 0.3
    assert onl.case_sequence(64).shape[0] == 70 and onl.case_frames(23) == 51 and onl.case_frames(3) == 11
    for win in onl.WINS + (onl.BIG_WIN,):
        c = onl.calibration(win)
        assert c.shape[0] == 2 * (2 * (win // 2) + 1) + 5
        assert not np.array_equal(c[:5], onl.white_sequence(c.shape[0], 0)[:5])
    assert [onl.field(onl.ARCHS[a]) for a in ("ik", "c48", "s1x3", "s2first")] == [22, 21, 4, 10]
    for g, kind in fb.WEIGHT_SETS:
        for l in range(fb.NL):
            assert fb.is_sparse(onl.weights(g, kind), l) == fb.SPARSE[g]
    for a in ("c48", "s1x3", "s2first"):
        assert all(fb.is_sparse(onl.weights(arch=a), l) for l in range(len(onl.ARCHS[a])))


def test_compare_is_per_row_and_refuses_non_finite():
    ref = np.array([[1.0, -2.0, 0.5], [1e3, 2e3, -4e3]])
    rel = 1e-6
    ok, row, el, ratio = onl.compare(ref * (1 + 3e-6), ref, rel)
    assert ok and 2.9 < ratio < 3.1
    got = ref.copy()
    got[0, 2] += 9e-6          # 4.5 of row 0's unit (2e-6), nothing in row 1's (4e-3)
    ok, row, el, ratio = onl.compare(got, ref, rel)
    assert not ok and (row, el) == (0, 2) and 4.4 < ratio < 4.6
    got = ref.copy()
    got[1, 0] += 9e-6
    assert onl.compare(got, ref, rel)[0]
    for bad in (np.nan, np.inf):
        got = ref.copy()
        got[1, 1] = bad
        ok, row, el, ratio = onl.compare(got, ref, rel)
        assert not ok and (row, el) == (1, 1)
    assert onl.compare(ref, ref, rel, rows=[7, 9])[1] in (7, 9)


# ---------------------------------------------------------------- the bar
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_float32_oracle_passes(cfg):
    graph, kind, arch, win = cfg
    rel = onl.case_rel32(*cfg)
    assert fb.EPS32 <= rel < 2e-6, rel      # float32 noise, whatever the poses' scale
    r32 = onl.reference(onl.weights(graph, kind, arch), onl.case_sequence(win), win, onl.ARCHS[arch], np.float32)
    ok, row, el, ratio = onl.compare(r32, onl.case_reference(*cfg), rel)
    print(f"ONLINE-HOST f32 oracle {cfg}: rel32={rel:.2e} max|f64|={np.abs(onl.case_reference(*cfg)).max():.2e} worst={ratio:.2f} at row {row}")
    assert ok, (cfg, row, el, ratio)


@pytest.mark.parametrize("inject", onl.INDEXING)
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_indexing_mistakes_fail(cfg, inject):
    ok, row, el, ratio = _injected(cfg, inject)
    print(f"ONLINE-HOST {inject} {cfg}: {ratio:.3g} at row {row}")
    if inject == "newest_is_previous" and not _reads_newest(cfg):
        assert ok and ratio < 1e-3, (cfg, inject, ratio)     # the pose does not read the pushed frame
    else:
        assert not ok and ratio > 10 * fb.MARGIN, (cfg, inject, row, ratio)


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[3] <= 9 and _reads_newest(c)], ids=lambda c: "-".join(map(str, c)))
def test_newest_frame_from_fewer_planes(cfg):
    """One plane fails; two planes are measured and stay inside the bar (docstring, 4.)."""
    ok2, _, _, r2 = _injected(cfg, "newest_two_planes")
    ok1, row, _, r1 = _injected(cfg, "newest_one_plane")
    print(f"ONLINE-HOST planes {cfg}: two {r2:.3g}, one {r1:.3g} at row {row}")
    assert not ok1, (cfg, r1)
    assert r2 < r1 / 16
