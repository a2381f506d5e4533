// fk_kploss.h — the arguments of fk_kploss_kernel (fk_kploss.hip): the keypoint loss of a frame and its gradient with
// respect to the pose, one workgroup per frame. Shared by tik_fk_keypoint_loss and the training step's keypoint
// term (train_step.cpp), which checks every body model before its first launch and fills the pointers later.
#pragma once
#include "lm_refine.h"

namespace tik {

struct FkKpLossArgs : LmRefineArgs {   // B workgroups; poses, kps, betas, joint_w as in LmRefineArgs but for poses_ld
    const int* rows;                   // workgroup b works on frame rows[b]; null: frame b. Not range-checked.
    float* loss;                       // [frame], or null
    float* grad;                       // row f at grad + f grad_ld, or null
    int poses_ld, grad_ld;
    float grad_scale;
    int accumulate;                    // non-zero: grad += grad_scale g, else grad = grad_scale g
};

// Host: every check of tik_fk_keypoint_loss (include/tik.h) in the entry point's order, then the arguments.
// TIK_E_INVALID names the value; nothing on the device is touched.
int fk_kploss_args(const tik_fk* fk, const char* who, const float* poses, int poses_ld, const float* kps, const float* betas,
                   int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, const int* rows, int B, float* loss,
                   float* grad, int grad_ld, float grad_scale, int accumulate, FkKpLossArgs& a);
// a.B workgroups. -> TIK_OK or TIK_E_HIP
int fk_kploss_launch(const FkKpLossArgs& a, void* stream);

}  // namespace tik
