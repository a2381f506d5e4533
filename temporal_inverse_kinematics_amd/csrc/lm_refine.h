// lm_refine.h — the arguments of lm_refine_kernel (lm_refine.hip): the whole Levenberg-Marquardt refinement of
// a frame in one launch, one workgroup per frame. Shared by tik_fk_refine (a batch of frames) and the online
// stream's recorded step (stream_step.cpp: one frame, sources and sinks read from the stream's own buffers).
#pragma once
#include <hip/hip_runtime.h>

#include "fk.h"

struct tik_fk;

namespace tik {

constexpr int LMR_N = 66;      // unknowns: the pose values of joints 0..21
constexpr int LMR_COLS = 17;   // keypoints (COCO order)
constexpr int LMR_M = 3 * LMR_COLS;
constexpr int LMR_DOF = 22;
// COCO-17 as SMPL-X joints (training_data.SMPLX_TO_COCO): the selection of a stream, and of a null sel17
constexpr int LMR_COCO_SMPLX[LMR_COLS] = {55, 57, 56, 59, 58, 16, 17, 18, 19, 20, 21, 1, 2, 4, 5, 7, 8};

// Inside a stream's step (count non-null; B = 1): where the frame comes from and where the pose goes.
struct LmRefineStream {
    const int* count;    // frames pushed so far, this step's included: the frame refined is c = count - 1 - h
    const float* ring;   // W frames of 51 floats; frame c at slot c % W
    int W, h;
    const float* conf_host;   // pinned: the 17 confidences of this push (ones for a plain tik_stream_push)
    float* cring;        // W rows of 17 confidences beside the ring, the same slots; the kernel stores frame count - 1's
    float* prev;         // (66) the previous refined pose
    int* have;           // non-zero once prev holds one (cleared by tik_stream_reset)
    float* pose_host;    // pinned: the refined pose, then
    int* done_host;      // pinned: the frame count, written last (tik_stream_push spins on it)
};

struct LmRefineArgs : FkSelArgs {   // B frames; n_sel = 17, sel = the keypoints' joints; ajt unused
    int nb, ns;                      // betas used, row length of jd (nb + ne)
    int maxdepth, iters;
    float mu, smooth, lam0;
    const float* poses;              // (B,66) start (a stream: the network's pose of this step)
    const float* prior;              // (B,66) or null = poses
    const float* prev;               // (B,66) or null
    const float* kps;                // (B,17,3)
    const float* betas;              // row b at betas + b betas_ld, or null (the mean shape)
    const float* joint_w;            // row b at joint_w + b joint_w_ld, or null (ones)
    int betas_ld, joint_w_ld;
    const float *pose_mean, *jt, *jd;
    const int *parents, *depth;
    const unsigned long long* anc;
    float *out_poses, *out_cost, *dbg_jac, *dbg_r;
    float sigma;                     // robust scale in metres; 0: the plain weighted square
    int flags;                       // TIK_REFINE_* (include/tik.h)
    float* dbg_w;                    // (B,17) or null: the IRLS weights of the first linearisation
    int nv;                         // keypoints that are a vertex of the body (the others are chain joints)
    signed char slot[LMR_COLS];      // column s: its vertex slot, or -1
    LmRefineStream st;
};

// Host: the model's part of the arguments (selection, tables, LM scalars), range-checked in the style of
// lm_check_range. sel17: 17 joint indices, or null = LMR_COCO_SMPLX. TIK_E_INVALID names the value.
int lm_refine_model_args(const tik_fk* fk, const char* who, const int* sel17, int iters, float mu, float smooth, float lam0,
                         LmRefineArgs& a);
// The robust scale of an entry point (`who`): >= 0 and finite, else TIK_E_INVALID
int lm_refine_check_sigma(const char* who, float sigma);
// B workgroups; a's pointers must be set. -> TIK_OK or TIK_E_HIP
int lm_refine_launch(const LmRefineArgs& a, void* stream);

}  // namespace tik
