// train_model.h — the trainer handle, shared by train_model.cpp (create: plan on
// the host, then one upload; destroy, the entry table, read / write, debug),
// train_step.cpp (the training step) and train_eval.cpp (the eval pass).
#pragma once
#include "cgemm.h"
#include "common.h"
#include "misc.h"
#include "train.h"
#include "train_plan.h"

namespace tik_train {

struct TrainLayer : PlanLayer {     // a block's descriptor and its device buffers
    DevBuf wgf, wgb, wtf, wtb, wrf, wrb, aeff;     // derived GEMM layouts
    DevBuf wg_e, b2_e, wt_e, bT_e, wr_e;            // eval set: eval-mode BatchNorm folded into wgf / wtf / wrf and the biases
    DevBuf Y, Z, H, U, Q, O;                        // saved activations
    DevBuf st1, st2, st3;                           // [4][C] mean, invstd, scale, shift
    int tin = 0, tout = 0;                          // of the step's batch shape (reserve)
};

}  // namespace tik_train

struct tik_trainer {
    tik_train::TrainPlan plan;          // entry table, offsets, head dimensions (hp / hb emptied after the upload)
    std::vector<tik_train::TrainLayer> L;
    tik_host::DevBuf P, G, M, Vv, B;
    long long np = 0;                   // values in P (and in G, M, Vv)
    bool zero_pending = false;          // gA/gB reallocated: zero them on the step's stream
    tik_host::DevBuf w1b, w2b;          // W1^T [feat][512], W2^T [512][ldp]
    // workspace
    int N = 0, T = 0;
    std::vector<tik_train::Frames> fr;  // the frame chain of (N, T); sized once at create
    tik_host::DevBuf x4, x0, st0, k, Ph, Dh, Oh, dOh, dD, mask, loss, partf, gA, gB, tS, tU, tQ, tH, tZ, tY, col, up;
    tik_host::DevBuf kpl;               // the per-frame keypoint losses of the last step (rows_h; tik_trainer_step_kp)
    tik_host::DevArray<double> partd;
    tik_host::DevIBuf cmap0;
    long long partf_cap = 0, partd_cap = 0;
    long long steps = 0;
    tik_host::DevArray<tik::PermDesc> perm;   // weight re-layout descriptors
    long long perm_blocks = 0;
    bool debug = false;                 // TIK_TRAIN_DEBUG at create: keep each block's input gradient of the last step
    int debug_layer = -1;               // TIK_TRAIN_DEBUG_LAYER at create (0..L-1): keep that block's gS, dU, dH (post-ReLU), dZ, dY
    std::vector<tik_host::DevBuf> dbg_dx;
    tik_host::DevBuf dbg_b[5];
    float lr = 1e-4f, eps = 1e-8f, momentum = 0.1f;
    // Adam's betas in double, as torch.optim.Adam holds them: the bias corrections 1 - beta^steps
    // and the weights 1 - beta come from these, never from a value already rounded to fp32
    // (1 - 0.999f is 1.3e-5 off 0.001, which moves sqrt(bc2), and so every update, by 6e-6)
    double beta1 = 0.9, beta2 = 0.999;
    // eval pass (tik_trainer_eval): the folded eval set is valid for weight version
    // `folded_at`; step() and tik_trainer_write bump `version`
    long long version = 1, folded_at = 0;
    bool derive_stale = false;        // a written value: the derived GEMM layouts follow before the next use
    bool mix_sparse = false;          // A (hence A_eff) lies inside the COCO hop<=2 pattern
    tik_host::DevBuf dbn_e;           // [2][4*V] folded data_bn scale, shift on the padded columns
    tik_host::DevArray<tik::FoldDesc> fold;   // eval-set descriptors
    long long fold_blocks = 0;
    struct {                          // the eval pass's own workspace, grown on demand
        std::vector<tik_train::Frames> fr;
        tik_host::DevBuf x4, x0, z, a0, a1, ph, oh;
        tik_host::DevArray<double> part;
    } ev;
};

namespace tik_train {

inline tik::Seg seg32(const float* src, const float* w, int cin, int ld, int kt, int stride, int pad, int tin, int ldw) {
    tik::Seg s{src, w, cin, ld, kt, stride, pad, tin, ldw};
    return s;
}

// A one-segment fp32 implicit GEMM, out[M][ldo] = seg . w^T (+ bias), no activation;
// a second segment, a residual, the graph epilogue or split-K are set on the result.
inline tik::CgemmArgs gemm_args(long long M, int Nc, int Vj, int tout, const tik::Seg& seg, const float* bias, float* out,
                                int ldo) {
    tik::CgemmArgs a{};
    a.M = (int)M; a.Nc = Nc; a.V = Vj; a.tout = tout;
    a.seg[0] = seg;
    a.nseg = 1; a.bias = bias; a.out = out; a.ldo = ldo; a.act = tik::ACT_NONE;
    return a;
}

// GEMM-side layouts from the flat parameters, after create and every update
// (train_step.cpp; the eval pass calls it after a tik_trainer_write)
int derive(tik_trainer* t, hipStream_t st);

}  // namespace tik_train
