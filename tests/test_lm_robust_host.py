"""Refinement on imperfect detections, what needs no GPU: the float64 reference's own conditions on the two scenarios
of tests/lm_robust_ref.py (checked here before any GPU test relies on them), the stream's hold-last fill
(csrc/stream_plan.h, compiled into a stand-alone program as tests/test_stream_plan_host.py does) against numpy, and the
Python argument checks.

Figures of the float64 run, worst keypoint distance per frame to the clean truth (m): plain LM with the outlier
0.31 .. 0.45, sigma = 0.1 0.010 .. 0.037 (ratio <= 0.082 on every frame), clean keypoints below 0.01."""
import os
import subprocess

import numpy as np
import pytest

import lm_robust_ref as RR
from test_fk_fold_host import CLANG, CSRC

TIK_E_INVALID = -1


# ---------------------------------------------------------------- the reference's own conditions
def test_outlier_scenario_reference():
    c = RR.case_outlier()
    print(f"worst keypoint distance per frame: plain {c['d_plain']}, sigma={RR.SIGMA} {c['d_robust']}, "
          f"ratio {c['d_robust'] / c['d_plain']}")
    assert np.isfinite(c["hist"]).all() and (np.diff(c["hist"], axis=0) <= 0).all()
    assert (c["d_plain"] >= 0.3).all()
    assert (c["d_robust"] <= 0.25 * c["d_plain"]).all()


def test_missing_scenario_reference():
    c = RR.case_missing()
    print(f"missing rule against weights 0: max |pose difference| = {np.abs(c['th'] - c['th_w']).max()}")
    assert np.array_equal(c["th"], c["th_w"]) and np.array_equal(c["hist"], c["hist_w"])
    assert np.array_equal(c["th"][4], c["th0"][4].astype(np.float64)) and (c["hist"][:, 4] == 0).all()
    assert np.isfinite(c["hist"]).all() and (np.diff(c["hist"], axis=0) <= 0).all()
    assert (c["hist"][-1, [0, 1, 2, 3, 5]] < c["hist"][0, [0, 1, 2, 3, 5]]).all()


# ---------------------------------------------------------------- the fill rule
# argv = in out; in: records of int32 op, 51 float32 frame, 17 float32 conf; op 0 = a push with confidences
# (fill_frame, then accept_frame where it passed), 1 = a plain push (check_frame, accept_frame), 2 = reset
# out: per record int32 code, 51 float32 the frame the stream would take, 17 float32 its confidences
SRC = r'''
#include <cstdio>
#include "stream_plan.h"
using namespace tik_stream_plan;
int main(int argc, char** argv) {
    FILE* fi = argc == 3 ? fopen(argv[1], "rb") : nullptr;
    FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
    if (!fo) return 2;
    LastSeen last;
    int op;
    float frame[FRAME], conf[V];
    while (fread(&op, sizeof op, 1, fi) == 1 && fread(frame, sizeof(float), FRAME, fi) == (size_t)FRAME &&
           fread(conf, sizeof(float), V, fi) == (size_t)V) {
        float of[FRAME] = {}, oc[V] = {};
        int rc = 0;
        if (op == 2) {
            last.clear();
        } else if (op == 1) {
            rc = check_frame(frame);
            if (!rc) {
                accept_frame(last, frame);
                for (int i = 0; i < FRAME; ++i) of[i] = frame[i];
                for (int k = 0; k < V; ++k) oc[k] = 1.f;
            }
        } else {
            rc = fill_frame(frame, conf, last, of, oc);
            if (!rc) accept_frame(last, of);
            else {   // a refusal may have written part of the outputs
                for (int i = 0; i < FRAME; ++i) of[i] = 0.f;
                for (int k = 0; k < V; ++k) oc[k] = 0.f;
            }
        }
        fwrite(&rc, sizeof rc, 1, fo);
        fwrite(of, sizeof(float), FRAME, fo);
        fwrite(oc, sizeof(float), V, fo);
    }
    fclose(fo);
    return 0;
}
'''


def numpy_stream(ops, frames, conf):
    """The rule restated: -> (codes, frames taken, their confidences), zeros where refused or reset."""
    seen, held = np.zeros(17, bool), np.zeros((17, 3), np.float32)
    codes, of, oc = [], np.zeros_like(frames), np.zeros_like(conf)
    for i, op in enumerate(ops):
        rc = 0
        if op == 2:
            seen[:] = False
        elif op == 1:
            if not np.isfinite(frames[i]).all():
                rc = TIK_E_INVALID
            else:
                seen[:], held[:], of[i], oc[i] = True, frames[i], frames[i], 1
        else:
            missing = (conf[i] == 0) | ~np.isfinite(frames[i]).all(1)
            if not (np.isfinite(conf[i]).all() and (conf[i] >= 0).all()) or (missing & ~seen).any():
                rc = TIK_E_INVALID
            else:
                of[i] = np.where(missing[:, None], held, frames[i])
                oc[i] = np.where(missing, 0, conf[i])
                seen[:], held[:] = True, of[i]
        codes.append(rc)
    return np.array(codes), of, oc


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang is not available")
def test_fill_rule_against_numpy(tmp_path):
    rng = np.random.default_rng(24)
    n = 24
    frames = rng.normal(0, 0.5, (n, 17, 3)).astype(np.float32)
    conf = rng.uniform(0.2, 1.0, (n, 17)).astype(np.float32)
    ops = np.zeros(n, np.int32)
    conf[0, 3] = 0                       # never seen: refused
    frames[2, 9] = np.nan                # 1 was complete: keypoint 9 held
    conf[3, 9] = 0                       # and held again: the value of frame 1
    frames[4, 5, 1] = np.inf             # one infinite coordinate with positive confidence
    conf[5, 2] = -0.5                    # refused
    conf[6, 2] = np.nan                  # refused
    conf[7, 2] = np.inf                  # refused
    frames[8], conf[8] = np.nan, 0       # nothing detected at all: the whole frame held
    ops[10] = 1                          # a plain push
    ops[11], frames[11, 0, 0] = 1, np.nan   # a plain push with a NaN: refused as ever
    conf[12, 11] = 0
    ops[14] = 2                          # reset
    conf[15, 4] = 0                      # not seen since the reset: refused
    frames[17, 4] = np.nan               # 16 was complete
    conf[20:23, 16] = 0                  # three frames in a row
    with open(tmp_path / "in.bin", "wb") as f:
        for i in range(n):
            f.write(ops[i].tobytes() + frames[i].tobytes() + conf[i].tobytes())
    src = tmp_path / "fill_main.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "fill_main")
    r = subprocess.run([CLANG, "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    rec = np.dtype([("rc", "<i4"), ("frame", "<f4", (17, 3)), ("conf", "<f4", (17,))])
    got = np.fromfile(tmp_path / "out.bin", dtype=rec)
    codes, of, oc = numpy_stream(ops, frames, conf)
    assert len(got) == n
    assert np.array_equal(got["rc"], codes), (got["rc"], codes)
    assert sorted(np.flatnonzero(codes)) == [0, 5, 6, 7, 11, 15]
    assert np.isfinite(got["frame"]).all()
    assert np.array_equal(got["frame"], of) and np.array_equal(got["conf"], oc)
    # the same through the sequence helper the GPU tests use, on the stretch it covers (frame 1 complete, no refusal)
    filled, c = RR.hold_last(frames[1:5], conf[1:5])
    assert np.array_equal(filled, of[1:5]) and np.array_equal(c, oc[1:5])


# ---------------------------------------------------------------- Python argument checks
def test_python_argument_checks():
    assert RR.check_robust_args(0.0) == (0.0, 0) and RR.check_robust_args(0.1, True) == (0.1, RR.REFINE_SKIP_NONFINITE)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            RR.check_robust_args(bad)
        with pytest.raises(ValueError):
            RR.check_stream_robust(3, bad)
        with pytest.raises(ValueError):
            RR.check_fused_options(True, bad, False)
    assert RR.check_fused_options(True, 0.1, True) == (0.1, True) and RR.check_fused_options(False, 0.0, False) == (0.0, False)
    with pytest.raises(ValueError, match="fused=True"):
        RR.check_fused_options(False, 0.1, False)
    with pytest.raises(ValueError, match="fused=True"):
        RR.check_fused_options(False, 0.0, True)
    with pytest.raises(ValueError, match="refine > 0"):
        RR.check_stream_robust(0, 0.1)
    assert RR.check_stream_robust(0, 0.0) == 0.0 and RR.check_stream_robust(2, 0.1) == 0.1
    ok = RR.check_conf(np.linspace(0, 1, 17))
    assert ok.dtype == np.float32 and ok.shape == (17,)
    assert RR.check_conf(np.ones((5, 17)), 5).shape == (5, 17)
    neg, nan = np.ones(17), np.ones(17)
    neg[3], nan[16] = -1e-3, np.nan
    for bad in (np.ones(16), np.ones((17, 1)), np.ones((2, 17)), neg, nan):
        with pytest.raises(ValueError):
            RR.check_conf(bad)
    with pytest.raises(ValueError):
        RR.check_conf(np.ones((4, 17)), 5)


def test_refine_poses_refuses_before_the_device():
    """Either option with fused=False: ValueError from the argument checks, no body model needed."""
    from temporal_inverse_kinematics_amd.refine import refine_poses
    th, kps = np.zeros((2, 66), np.float32), np.zeros((2, 17, 3), np.float32)
    for kw in (dict(robust_sigma=0.1), dict(skip_nonfinite=True), dict(fused=True, robust_sigma=-1.0)):
        with pytest.raises(ValueError):
            refine_poses(th, kps, None, **kw)
