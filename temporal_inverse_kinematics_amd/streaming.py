"""Online (streaming) IK — BASELINE.json config #5.

The reference is offline: `inference.run_inference` (inference.py:37-67)
solves a recorded sequence with one edge-padded window per frame. Online,
frame c is solvable once frame c+h has arrived (h = win_size//2); each
`push` appends a frame to a device ring, gathers the window centred h frames
back and solves it (`tik_stream_*`). Output for frame c is identical to
run_inference's (within fp32 rounding). The default step is one dataflow
kernel (csrc/online.hip) over only the frames pose row 0 depends on, its convs
in bf16x3 MFMA arithmetic (`path == "dataflow"`); TIK_ONLINE=0 selects the
layered forward over the whole window.

`refine=N` adds N Levenberg-Marquardt iterations per push (one more launch in
the recorded step: the fused kernel of SMPLX.refine_frames, one workgroup, on
the frame the step just solved and its own keypoints from the device ring), so
`push` returns a pose whose FK joints sit on the keypoints; `smooth_weight > 0`
also ties each refined pose to the previous refined one, the causal
counterpart of refine.refine_smooth. Nobody has measured a good smooth_weight
on real detections: there is no tuned default, 0 means no tie.

Imperfect detections: `push(frame, conf)` takes 17 confidences. A keypoint with
confidence 0 or a non-finite coordinate is missing: the network gets the last
value the stream accepted for it (hold-last, a stated rule that nobody has
measured on real detections), and the refinement weighs the frame's keypoints
by conf * joint_weight (a missing hip: the whole frame by 0). `robust_sigma > 0`
gives the refinement's data term the Geman-McClure scale of
SMPLX.refine_frames; there is no tuned value, 0 is off. A plain `push(frame)`
behaves as before, its refusal of a NaN included.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib


def check_refine_args(refine, smplx_model, betas, prior_weight, smooth_weight, lam0, joint_weight):
    """OnlineIK's refinement arguments -> (iters, mu, smooth, lam0, betas float32 (nb,) or None, weights float32
    (17,) or None). ValueError for refine > 0 without a body model and for a bad weight; the library is not asked."""
    from .smplx_fk import REFINE_KPS, check_refine_scalars
    iters, mu, smooth, lam0 = check_refine_scalars(refine, prior_weight, smooth_weight, lam0)
    if iters == 0:
        return 0, mu, smooth, lam0, None, None
    if smplx_model is None or not hasattr(smplx_model, "_h"):
        raise ValueError("refine > 0 needs smplx_model, the smplx_fk.SMPLX body whose FK joints are pulled onto the keypoints")
    b = w = None
    if betas is not None:
        b = np.ascontiguousarray(betas, dtype=np.float32)
        if b.shape != (smplx_model.num_betas,) or not np.isfinite(b).all():
            raise ValueError(f"betas must be ({smplx_model.num_betas},) finite values, got shape {b.shape}")
    if joint_weight is not None:
        w = np.ascontiguousarray(joint_weight, dtype=np.float32)
        if w.shape != (REFINE_KPS,) or not (w >= 0).all():
            raise ValueError(f"joint_weight must be ({REFINE_KPS},) non-negative values (COCO order), got shape {w.shape}")
    return iters, mu, smooth, lam0, b, w


def check_stream_robust(iters: int, robust_sigma) -> float:
    """OnlineIK's robust_sigma -> float: >= 0 and finite (smplx_fk.check_robust_args), and > 0 only on a refining
    stream (the robust term lives in the refine launch). ValueError otherwise; the library is not asked."""
    from .smplx_fk import check_robust_args
    sigma, _ = check_robust_args(robust_sigma)
    if sigma > 0.0 and iters == 0:
        raise ValueError("robust_sigma > 0 needs refine > 0: the robust term belongs to the refinement launch")
    return sigma


def check_conf(conf, frames: Optional[int] = None) -> np.ndarray:
    """The confidences of a push, (17,), or with `frames` those of a sequence, (frames,17): finite and >= 0 -> them
    as contiguous float32. ValueError otherwise (a wrong shape, a negative value, a NaN, an Inf); the library is
    not asked."""
    c = np.ascontiguousarray(conf, dtype=np.float32)
    want = (17,) if frames is None else (int(frames), 17)
    if c.shape != want:
        raise ValueError(f"conf must be {want} confidences (COCO order), got shape {c.shape}")
    if not (np.isfinite(c).all() and (c >= 0).all()):
        raise ValueError("conf must be finite and >= 0 (0 = the keypoint is missing)")
    return c


class OnlineIK:
    def __init__(self, model, win_size: Optional[int] = None, use_graph: bool = True, refine: int = 0, smplx_model=None,
                 betas=None, prior_weight: float = 1e-2, smooth_weight: float = 0.0, lam0: float = 1e-2, joint_weight=None,
                 robust_sigma: float = 0.0):
        iters, mu, smooth, lam0, b, w = check_refine_args(refine, smplx_model, betas, prior_weight, smooth_weight, lam0,
                                                          joint_weight)
        sigma = check_stream_robust(iters, robust_sigma)
        reg = getattr(model, "regressor", model)
        self.win_size = int(win_size if win_size is not None else model.hparams.win_size)
        self.h = self.win_size // 2
        self._model = model
        lib = _lib.load()
        handle = reg.tik_handle()
        # the stream owns its workspace and holds a library reference on the
        # model handle, so later batch calls (which may grow the handle's
        # workspace) or a handle rebuilt after a weight change leave it intact;
        # the Python reference below only documents that ownership
        self._handle_ref = reg._tik
        s = _lib.ctypes.c_void_p()
        _lib.check(lib.tik_stream_create(handle, self.win_size, int(use_graph), _lib.ctypes.byref(s)), "OnlineIK")
        self._s = s.value
        self._destroy = lib.tik_stream_destroy
        self._pose = np.zeros(66, np.float32)
        self._last = None
        # per-push overhead: the frame goes through one preallocated buffer and both
        # ctypes pointers are made once (building them per call cost ~8 us of a ~60 us push)
        self._push_fn = lib.tik_stream_push
        self._fbuf = np.zeros(51, np.float32)
        self._fptr = self._fbuf.ctypes.data_as(_lib._F)
        # a second frame buffer: the one a push filled is kept as the last frame, the other takes the next
        self._obuf = np.zeros(51, np.float32)
        self._optr = self._obuf.ctypes.data_as(_lib._F)
        self._pptr = self._pose.ctypes.data_as(_lib._F)
        self.path = "dataflow" if _lib.check(lib.tik_stream_path(self._s)) == 1 else "layered"
        self.refine = iters
        self._raw = np.zeros(66, np.float32)
        self._have_pose = False
        if iters > 0:
            # the stream holds a library reference on the body model too; the copies of betas and weights are its own
            self._smplx = smplx_model
            _lib.check(lib.tik_stream_set_refine(self._s, smplx_model._h, None if b is None else b.ctypes.data_as(_lib._F),
                                                 None if w is None else w.ctypes.data_as(_lib._F), iters, mu, smooth, lam0),
                       "OnlineIK")
            if sigma > 0.0:
                _lib.check(lib.tik_stream_set_robust(self._s, sigma), "OnlineIK")
        self.robust_sigma = sigma
        # a push with confidences: two more preallocated buffers, as for the frame
        self._push_conf_fn = lib.tik_stream_push_conf
        self._cbuf = np.ones(17, np.float32)
        self._cptr = self._cbuf.ctypes.data_as(_lib._F)
        self._last_conf = None

    def __del__(self):
        try:
            if getattr(self, "_s", None):
                self._destroy(self._s)
        except Exception:
            pass

    def reset(self):
        _lib.check(_lib.load().tik_stream_reset(self._s))
        self._last = None
        self._last_conf = None
        self._have_pose = False

    @property
    def raw(self) -> Optional[np.ndarray]:
        """The network's own (66,) pose of the last push that returned one (what it would have returned
        with refine=0), or None before the first."""
        if not self._have_pose:
            return None
        _lib.check(_lib.load().tik_stream_raw_pose(self._s, self._raw.ctypes.data_as(_lib._F)), "OnlineIK.raw")
        return self._raw.copy()

    def push(self, frame: np.ndarray, conf=None) -> Optional[np.ndarray]:
        """frame (17,3) -> the (66,) pose of the frame h pushes back (refined when refine > 0), or None while filling.
        A frame with a NaN or an Inf in it raises ValueError and is not appended: the
        stream goes on as if it had never been offered.
        conf (17,) finite and >= 0 (tik_stream_push_conf): keypoint k is missing where conf[k] is 0 or one of its
        coordinates is not finite. The network gets the last value the stream accepted for it (hold-last; a stated
        rule, nobody has measured it on real detections), and a refining stream weighs keypoint k of the frame by
        conf[k] * joint_weight[k], all 17 by 0 where conf[11] or conf[12] is 0. ValueError, nothing appended: a bad
        conf, and a missing keypoint that has not been seen since the stream was created or reset."""
        f = np.asarray(frame, dtype=np.float32)
        if f.size != 51:
            raise ValueError("expected one (17,3) COCO frame")
        if conf is not None:
            conf = check_conf(conf)
        self._fbuf[:] = f.reshape(-1)
        if conf is None:
            rc = self._push_fn(self._s, self._fptr, self._pptr)
        else:
            self._cbuf[:] = conf
            rc = self._push_conf_fn(self._s, self._fptr, self._cptr, self._pptr)
        if rc == _lib.TIK_E_INVALID:
            # a NaN or Inf in the frame: it was not appended (include/tik.h), so flush must not repeat it
            _lib.check(rc, "OnlineIK.push")
        # the last frame the ring took (flush repeats it): the two buffers change places, no copy
        self._last = self._fbuf
        self._last_conf = None if conf is None else conf.copy()
        self._fbuf, self._obuf, self._fptr, self._optr = self._obuf, self._fbuf, self._optr, self._fptr
        if rc < 0:
            _lib.check(rc, "OnlineIK.push")
        if rc == 1:
            self._have_pose = True
        return self._pose.copy() if rc == 1 else None

    def flush(self):
        """Poses of the last h frames (right edge padding = repeat the last accepted frame, with its confidences:
        a keypoint missing in it is filled again with the value the stream holds)."""
        out = []
        for _ in range(self.h):
            p = self.push(self._last.reshape(17, 3), self._last_conf)
            if p is not None:
                out.append(p)
        return out

    def run(self, seq: np.ndarray, conf=None) -> np.ndarray:
        """Whole sequence through the online path: (F,17,3) -> (F,66). conf: None or (F,17), one row per push."""
        if conf is not None:
            conf = check_conf(conf, len(seq))
        self.reset()
        out = []
        for i, fr in enumerate(seq):
            p = self.push(fr, None if conf is None else conf[i])
            if p is not None:
                out.append(p)
        out += self.flush()
        return np.stack(out)[: seq.shape[0]]
