"""Config #5: streaming sliding-window (stride 1) online IK, hipGraph-captured
step, per-frame latency (push of one frame -> its solved pose on the host).

    python bench_stream.py [--frames 10000] [--warmup 100] [--win 64] [--refine N [--smooth W] [--robust S] [--conf]]

--refine N: the stream refines every pose with N Levenberg-Marquardt iterations
(one more launch in the recorded step, streaming.OnlineIK(refine=N)) against the
synthetic SMPL-X body; --smooth W also ties it to the previous refined pose,
--robust S gives its data term the Geman-McClure scale S (metres), --conf pushes
every frame with 17 confidences (tik_stream_push_conf; about one keypoint in 50
missing, the others U(0.5, 1)).

bench.py --full reuses measure_online() for its "online" key.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def measure_online(frames=10000, warmup=100, win=64, use_graph=True, precision="bf16x3", refine=0, smooth=0.0, robust=0.0,
                   conf=False):
    """Push `frames` frames of the sample sequence (noised repeats) one at a
    time through OnlineIK and time each push (frame in -> pose on the host)."""
    import numpy as np
    from temporal_inverse_kinematics_amd import _build, synthetic as syn
    from temporal_inverse_kinematics_amd.inference import synthetic_model
    from temporal_inverse_kinematics_amd.streaming import OnlineIK
    _build.build()
    seq0 = syn.load_sample_coco()
    reps = -(-frames // seq0.shape[0])
    rng = np.random.default_rng(0)
    seq = np.concatenate([seq0 + rng.normal(0, 0.01, seq0.shape).astype(np.float32) for _ in range(reps)])[:frames]
    m = synthetic_model(win_size=win, device="cuda", precision=precision)
    body = None
    if refine:
        from temporal_inverse_kinematics_amd.smplx_fk import SMPLX
        body = SMPLX(syn.synthetic_smplx_constants(seed=1), batch_size=1)
    s = OnlineIK(m, use_graph=use_graph, refine=refine, smplx_model=body, smooth_weight=smooth, robust_sigma=robust)
    cf = None
    if conf:   # frame 0 complete (nothing is missing before it was seen), then about 2 % of the keypoints missing
        cf = rng.uniform(0.5, 1.0, (frames, 17)).astype(np.float32)
        cf[1:][rng.random((frames - 1, 17)) < 0.02] = 0.0
    for i in range(warmup):
        s.push(seq[i % seq.shape[0]])
    s.reset()
    lat = np.empty(frames)
    for i in range(frames):
        t0 = time.perf_counter()
        if cf is None:
            s.push(seq[i])
        else:
            s.push(seq[i], cf[i])
        lat[i] = time.perf_counter() - t0
    lat_us = lat * 1e6
    return {"metric": "online IK per-frame latency (p50)", "value": round(float(np.percentile(lat_us, 50)), 2),
            "unit": "us", "higher_is_better": False, "p99_us": round(float(np.percentile(lat_us, 99)), 2),
            "mean_us": round(float(lat_us.mean()), 2), "frames_per_s": round(frames / lat.sum(), 1),
            "n_gpus": 1, "dtype": ("f32: gcn and temporal convs via bf16x3 MFMA (3 bf16 planes, 6 products, fp32 accumulate), "
                                             "joint 16, graph mix and head in fp32 FMAs") if s.path == "dataflow" else precision, "step": s.path,
            "config": {"workload": f"stride-1 sliding window, win_size={win} (T={2 * (win // 2) + 1}), B=1, "
                                   f"{'hipGraph replay' if use_graph else 'eager launches'} per frame"
                                   + (" (one dataflow kernel, only the frames pose row 0 depends on)"
                                      if s.path == "dataflow" else " (layered forward on the whole window)"),
                       "frames": frames, "warmup": warmup,
                       **({"refine_iters": refine, "smooth_weight": smooth} if refine else {}),
                       **({"robust_sigma": robust} if robust else {}), **({"conf_per_push": True} if conf else {})}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--win", type=int, default=64)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "fp32"])
    ap.add_argument("--refine", type=int, default=0, help="LM iterations per push (0: the plain stream)")
    ap.add_argument("--smooth", type=float, default=0.0, help="with --refine: the weight of the tie to the previous refined pose")
    ap.add_argument("--robust", type=float, default=0.0, help="with --refine: the robust scale in metres (0: the plain square)")
    ap.add_argument("--conf", action="store_true", help="push every frame with 17 confidences, some of them 0")
    a = ap.parse_args()
    print(json.dumps(measure_online(a.frames, a.warmup, a.win, not a.no_graph, a.precision, a.refine, a.smooth, a.robust, a.conf)))


if __name__ == "__main__":
    main()
