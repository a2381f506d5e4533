// fk_kploss.hip — the keypoint loss of a pose and its gradient with respect to the pose in ONE launch
// (tik_fk_keypoint_loss, and the keypoint term of the training step): one workgroup of LM_T = 256 threads per frame,
// everything about the frame in LDS and registers. Per frame f (= rows[b], or b):
//
//   r       = rel(FK keypoints(th_f, beta_f)) - rel(kps_f)            rel(x) = x - mean of columns 11 / 12
//   loss[f] = 1/2 sum_k w_k |r_k|^2                                   (the data term of lm_refine.hip's cost)
//   g[q]    = sum_i w_i J[i][q] r[i]       i < 51, q < 66             (J^T W r, J with root-relative rows)
//   grad[f][q] = grad_scale g[q], or fmaf(grad_scale, g[q], grad[f][q]) with accumulate
//
// Phases, all of lm_refine_dev.h (the pieces of lm_refine_kernel, the same instructions):
//   0  frame_setup: pose, rel(kps), weights, betas, the selection and its skinning entries, the rest joints   2 barriers
//   1  fk_eval: Rodrigues, the chain by tree depth, the vertex keypoints' blend and skinning, r    maxdepth + 6 barriers
//   2  loss: wave 0, lane k's w_k |r_k|^2, one fixed butterfly (weighted_sq); lane 0 writes
//   3  linearize: dR and omega per dof, the 3x3 blocks of J (51,66) in LDS, rel on its rows                   3 barriers
//   4  thread q < 66: g[q], one FMA chain over the 51 rows in ascending order, (J[i][q] w_i) r_i per term
//      (lm_accumulate_body's term); the thread writes grad[f][q]
// Phases 3 and 4 only with grad. One FK state and no lm_dev.h slabs: lds_frame_floats(K, 1) floats of LDS, 30464 B
// with 4 skinning entries per vertex and 40880 B with the dense table (lm_refine_kernel: 48220 and 58636 B). The slab of
// robust row weights (Lds::ow, 208 B) is lm_refine_kernel's; here it is carved and not used.
// Every sum has a fixed order, no atomics, every output element has one writer, and a workgroup sees only its
// own frame: a frame's bits do not depend on B, on its place in the batch or on rows.
#include <cmath>

#include "fk_kploss.h"
#include "fk_model.h"
#include "lm_refine_dev.h"

namespace tik {

__global__ __launch_bounds__(LM_T) void fk_kploss_kernel(FkKpLossArgs a) {
    using namespace lmr;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const size_t f = a.rows ? (size_t)a.rows[blockIdx.x] : (size_t)blockIdx.x;
    const int K = skin_count(a);
    const Lds s(smem, K, 1);
    int dj, par;
    frame_setup(a, s, a.poses + f * a.poses_ld, nullptr, nullptr, false, a.kps + f * M, nullptr, false, f, K, 1, dj, par);
    float* S = s.state(0);
    fk_eval(a, s, S, s.th, dj, par, K);
    if (a.loss && tid < 64) {
        const float l = 0.5f * weighted_sq(s, S);
        if (tid == 0) a.loss[f] = l;
    }
    if (!a.grad) return;
    linearize(a, s, S, s.th, par, K);
    if (tid < N) {
        float g = 0.f;
        for (int i = 0; i < M; ++i) g = fmaf(s.J[i * N + tid] * s.rw[i], S[ST_R + i], g);
        float* o = a.grad + f * a.grad_ld + tid;
        *o = a.accumulate ? fmaf(a.grad_scale, g, *o) : a.grad_scale * g;
    }
}

int fk_kploss_args(const tik_fk* fk, const char* who, const float* poses, int poses_ld, const float* kps, const float* betas,
                   int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, const int* rows, int B, float* loss,
                   float* grad, int grad_ld, float grad_scale, int accumulate, FkKpLossArgs& a) {
    using namespace tik_host;
    if (!fk || !poses || !kps) return fail(TIK_E_INVALID, "%s: null pointer", who);
    if (!loss && !grad) return fail(TIK_E_INVALID, "%s: loss and grad are both null", who);
    if (B <= 0) return fail(TIK_E_INVALID, "%s: B must be positive, got %d", who, B);
    if (poses_ld < LMR_N) return fail(TIK_E_INVALID, "%s: poses_ld must be >= %d, got %d", who, LMR_N, poses_ld);
    if (grad && grad_ld < LMR_N) return fail(TIK_E_INVALID, "%s: grad_ld must be >= %d, got %d", who, LMR_N, grad_ld);
    if (!std::isfinite(grad_scale)) return fail(TIK_E_INVALID, "%s: grad_scale must be finite, got %g", who, (double)grad_scale);
    if (betas && betas_ld != 0 && betas_ld < fk->nb)
        return fail(TIK_E_INVALID, "%s: betas_ld must be 0 (one row for all frames) or >= %d, got %d", who, fk->nb, betas_ld);
    if (joint_w && joint_w_ld != 0 && joint_w_ld != LMR_COLS)
        return fail(TIK_E_INVALID, "%s: joint_w_ld must be 0 (shared) or 17 (per frame), got %d", who, joint_w_ld);
    LmRefineArgs m;
    if (int rc = lm_refine_model_args(fk, who, sel17, 0, 1.f, 0.f, 1.f, m)) return rc;   // the LM scalars are unused
    a = FkKpLossArgs{};
    static_cast<LmRefineArgs&>(a) = m;
    a.B = B;
    a.poses = poses; a.poses_ld = poses_ld; a.kps = kps;
    a.betas = betas; a.betas_ld = betas_ld; a.joint_w = joint_w; a.joint_w_ld = joint_w_ld;
    a.rows = rows; a.loss = loss; a.grad = grad; a.grad_ld = grad_ld; a.grad_scale = grad_scale; a.accumulate = accumulate ? 1 : 0;
    return TIK_OK;
}

int fk_kploss_launch(const FkKpLossArgs& a, void* stream) {
    return lm_launch(fk_kploss_kernel, a.B, lmr::lds_frame_floats(a.nz > 0 ? a.nz : 55, 1), stream, a);
}

}  // namespace tik

extern "C" int tik_fk_keypoint_loss(tik_fk_t fk, const float* poses, int poses_ld, const float* kps, const float* betas,
                                    int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, const int* rows, int B,
                                    float* loss, float* grad, int grad_ld, float grad_scale, int accumulate, void* stream) {
    tik::FkKpLossArgs a;
    if (int rc = tik::fk_kploss_args(fk, "tik_fk_keypoint_loss", poses, poses_ld, kps, betas, betas_ld, joint_w, joint_w_ld, sel17,
                                     rows, B, loss, grad, grad_ld, grad_scale, accumulate, a))
        return rc;
    return tik::fk_kploss_launch(a, stream);
}
