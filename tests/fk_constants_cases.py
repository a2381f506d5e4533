"""Malformed SMPL-X constant sets that tik_fk_create must refuse on the host,
shared by tests/test_fk_fold_host.py (the fold header alone) and
tests/test_host.py (the library's C ABI). The first five are reads past the end
of a std::vector in the single-file version of the FK host code."""
import numpy as np

SMALL = dict(seed=1, num_verts=64, num_faces=40)   # the smallest model the generator allows

# case -> the tensor whose name the refusal must carry
CASES = {
    "rank-2 exprdirs": "exprdirs",
    "rank-1 dynamic_lmk_faces_idx": "dynamic_lmk_faces_idx",
    "null-data v_template": "v_template",
    "posedirs one value short": "posedirs",
    "null-data faces": "faces",
    "lbs_weights (V,54)": "lbs_weights",
    "pose_mean with 164 values": "pose_mean",
    "parents[3] = 5": "parents",
    "lmk_faces_idx holding F": "lmk_faces_idx",
    "extra_verts holding V": "extra_verts",
}
ABI_CASES = list(CASES)[:6]


def small_constants():
    from temporal_inverse_kinematics_amd import synthetic as syn
    return syn.synthetic_smplx_constants(**SMALL)


def tensor_items(c, null=()):
    """-> [(name, float32 array, has data)] in the dict's order."""
    return [(k, np.ascontiguousarray(v, dtype=np.float32), k not in null) for k, v in c.items()]


def malformed(c, case):
    """-> (tensor items, the tensor's name); every case is built with the contour flag set."""
    c = {k: np.array(v) for k, v in c.items()}
    name = CASES[case]
    V, F = c["v_template"].shape[0], c["faces"].shape[0]
    null = ()
    if case == "rank-2 exprdirs":
        c[name] = c[name].reshape(V, -1)
    elif case == "rank-1 dynamic_lmk_faces_idx":
        c[name] = c[name].ravel()
    elif case in ("null-data v_template", "null-data faces"):
        null = (name,)
    elif case == "posedirs one value short":
        c[name] = c[name].ravel()[:-1]
    elif case == "lbs_weights (V,54)":
        c[name] = c[name][:, :54]
    elif case == "pose_mean with 164 values":
        c[name] = c[name].ravel()[:164]
    elif case == "parents[3] = 5":
        c[name][3] = 5
    elif case == "lmk_faces_idx holding F":
        c[name][7] = F
    elif case == "extra_verts holding V":
        c[name][2] = V
    else:
        raise ValueError(case)
    return tensor_items(c, null), name
