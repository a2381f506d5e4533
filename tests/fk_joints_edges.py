"""The mesh-free joints workload shared by tests/test_gpu_fk_joints.py (in the
pytest process, under TIK_POISON) and tests/fk_joints_guard_child.py (in a
child process, under TIK_GUARD=1). Not a test module. Built on tests/memedge.py:
its inputs (fk_inputs), constants (fk_consts) and release hook."""
import torch

import memedge as me

# 1, 3, 37: a workgroup per column (the small-launch mapping); 193: four body tiles, the last with
# one body, past the launcher's threshold for all joints (3 tiles x 18 column groups)
BATCHES = (1, 3, 37, 193)
RESERVE = 64
CONFIGS = ("sparse", "dense")          # memedge.FK_CONFIGS entries: nzw pairs / the dense WT rows
SELECTS = (None, "coco", (143, 5, 60, 60, 0, 127))


def joints_family(config, reserve=RESERVE):
    """SMPLX.joints at B = 1, 3, 37, 193 for every selection, on a handle whose mesh
    workspace was reserved for 64 bodies (reserve=None: the joints path grows
    its own buffers to each batch exactly) -> {(B, selection): joints}."""
    from temporal_inverse_kinematics_amd import _lib
    m = me.fk_model(config)
    if reserve:
        _lib.check(_lib.load().tik_fk_reserve(m._h, reserve), "tik_fk_reserve")
    out = {}
    for B in BATCHES:
        args = [torch.from_numpy(a).cuda() for a in me.fk_inputs(B)]
        for sel in SELECTS:
            n = m.num_joints if sel is None else 17 if sel == "coco" else len(sel)
            out[(B, str(sel))] = m.joints(*args, select=sel, out=me.nan_like((B, n, 3)))
        torch.cuda.synchronize()
    me.release(m)
    return out
