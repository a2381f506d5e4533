// fk_metrics.h — the arguments of fk_metrics_kernel (fk_metrics.hip): the pose metrics of a frame (MPJPE, Procrustes-
// aligned MPJPE, mean per-joint angle error, the weight sum), one workgroup per frame. Shared by tik_fk_pose_metrics.
#pragma once
#include "lm_refine.h"

namespace tik {

#ifndef TIK_METRICS_SWEEPS
#define TIK_METRICS_SWEEPS 6           // cyclic Jacobi sweeps over the 4x4 matrix of the alignment
#endif
constexpr int FKM_SWEEPS = TIK_METRICS_SWEEPS;
constexpr int FKM_COLS = 4;            // out columns: mpjpe, pa_mpjpe, mpjae, weight

struct FkMetricsArgs : LmRefineArgs {  // B workgroups; poses, kps, betas, joint_w as in LmRefineArgs but for poses_ld
    const int* rows;                   // workgroup b works on frame rows[b]; null: frame b. Not range-checked.
    const float* target_poses;         // row f at target_poses + f target_ld, or null (mpjae = NaN)
    float* out;                        // (frame, 4)
    float* joints_out;                 // (frame, 17, 3) root-relative FK keypoints, or null
    int poses_ld, target_ld;
    int skip;                          // non-zero: TIK_REFINE_SKIP_NONFINITE
};

// Host: every check of tik_fk_pose_metrics (include/tik.h) in the entry point's order, then the arguments.
// TIK_E_INVALID names the value; nothing on the device is touched.
int fk_metrics_args(const tik_fk* fk, const char* who, const float* poses, int poses_ld, const float* kps, const float* betas,
                    int betas_ld, const float* joint_w, int joint_w_ld, const float* target_poses, int target_ld,
                    const int* sel17, const int* rows, int B, int flags, float* out, float* joints_out, FkMetricsArgs& a);
// a.B workgroups. -> TIK_OK or TIK_E_HIP
int fk_metrics_launch(const FkMetricsArgs& a, void* stream);

}  // namespace tik
