// train_step.cpp — the training step: IKPoseTrainer.training_step
// (pose_trainer.py:146-155) + the Lightning backward + torch.optim.Adam step
// (configure_optimizers, pose_trainer.py:196-197), on the device.
//
// One step = train-mode forward (BatchNorm on batch statistics with the
// running-stat update, the head's Dropout(0.7), st_gcn_aaai18.py:119-133,
// 208-214, pose_trainer.py:89-92,94-133), nn.MSELoss against the target
// poses (PoseLosses, pose_trainer.py:42-50), the backward of every
// operation, and one Adam update of every parameter (lr = hparams.lr,
// betas (0.9, 0.999), eps 1e-8, no weight decay).
//
// After every update the GEMM-side layouts are re-derived from the flat
// parameters (temporal taps innermost for the forward, transposed /
// tap-flipped for the input gradients, A_eff = A * edge_importance). GEMMs
// (forward convs, input gradients) run on the fp32 implicit-GEMM kernel
// (cgemm.hip); weight gradients on train_wgrad.hip's row-split MFMA kernel
// beside the graph mix; BatchNorm and activation kernels in train_bn.hip,
// the head, losses and Adam in train_head.hip, the re-layouts in
// train_batch.hip (interface: train.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fk_kploss.h"
#include "train_model.h"

using namespace tik_host;
using namespace tik_train;

// one batched launch over a descriptor table built once (pointers are fixed)
int tik_train::derive(tik_trainer* t, hipStream_t st) {
    if (!t->perm.p) {
        const TrainPlan& p = t->plan;
        const float* P = t->P.p;
        std::vector<tik::PermDesc> d;
        auto add = [&](float* dst, const float* src, const float* src2, int d0, int d1, int d2, long long ds0,
                       long long ds1, long long ds2, long long soff, long long ss0, long long ss1, long long ss2) {
            tik::PermDesc q{dst, src, src2, d0, d1, d2, ds0, ds1, ds2, soff, ss0, ss1, ss2, 0};
            d.push_back(q);
        };
        for (TrainLayer& l : t->L) {
            const int ci = l.cin, cp = l.cinp, co = l.cout;
            // wgf[co][cp] <- W[co][ci]; wgb[ci][co] <- W[co][ci]
            add(l.wgf.p, P + l.wg, nullptr, co, ci, 1, cp, 1, 0, 0, ci, 1, 0);
            add(l.wgb.p, P + l.wg, nullptr, ci, co, 1, co, 1, 0, 0, 1, ci, 0);
            // wtf[co][tap][c] <- W[co][c][tap]; wtb[c][tap'][co] <- W[co][c][2 - tap']
            add(l.wtf.p, P + l.wt, nullptr, co, 3, co, 3LL * co, co, 1, 0, 3LL * co, 1, 3);
            add(l.wtb.p, P + l.wt, nullptr, co, 3, co, 3LL * co, co, 1, 2, 3, -1, 3LL * co);
            if (l.res == RES_CONV) {
                add(l.wrf.p, P + l.wr, nullptr, co, ci, 1, cp, 1, 0, 0, ci, 1, 0);
                add(l.wrb.p, P + l.wr, nullptr, ci, co, 1, co, 1, 0, 0, 1, ci, 0);
            }
            // A_eff = A * edge_importance (st_gcn_aaai18.py:129)
            add(l.aeff.p, t->B.p + p.A, P + l.E, V * V, 1, 1, 1, 0, 0, 0, 1, 0, 0);
        }
        // W1^T [feat][512] <- W1[512][feat]; W2^T [512][ldp] <- W2[pose][512]
        add(t->w1b.p, P + p.w1, nullptr, p.feat, HIDDEN, 1, HIDDEN, 1, 0, 0, 1, p.feat, 0);
        add(t->w2b.p, P + p.w2, nullptr, HIDDEN, p.pose_dim, 1, p.ldp, 1, 0, 0, 1, HIDDEN, 0);
        t->perm_blocks = tik::permute_batch_blocks(d.data(), (int)d.size());
        if (const int rc = t->perm.upload(d)) return rc;
    }
    HIP_TRY(tik::launch_permute_batch(t->perm.p, (int)t->perm.n, t->perm_blocks, st));
    return TIK_OK;
}

namespace {

constexpr float DROPOUT_P = 0.7f;   // pose_trainer.py:91

int reserve(tik_trainer* t, int N, int T) {
    if (N == t->N && T == t->T) return TIK_OK;
    int rc;
    frame_chain(t->plan, T, t->fr.data());
    for (size_t i = 0; i < t->L.size(); ++i) {
        TrainLayer& l = t->L[i];
        l.tin = t->fr[i].tin;
        l.tout = t->fr[i].tout;
        const long long pin = (long long)N * l.tin * V, pout = (long long)N * l.tout * V;
        if ((rc = l.Y.reserve(pin * l.cout)) || (rc = l.Z.reserve(pin * l.cout)) || (rc = l.H.reserve(pin * l.cout)) ||
            (rc = l.U.reserve(pout * l.cout)) || (rc = l.O.reserve(pout * l.cout)))
            return rc;
        if (l.res == RES_CONV && (rc = l.Q.reserve(pout * l.cout))) return rc;
    }
    const StepSizes s = step_sizes(t->plan, t->fr.data(), N, T);
    const int ldp = t->plan.ldp;
    t->partf_cap = s.partf_cap;
    t->partd_cap = s.partd_cap;
    if ((rc = t->x4.reserve(s.p0 * 4)) || (rc = t->x0.reserve(s.p0 * 4)) || (rc = t->Ph.reserve(s.rows_h * HIDDEN)) ||
        (rc = t->Dh.reserve(s.rows_h * HIDDEN)) || (rc = t->Oh.reserve(s.rows_h * ldp)) ||
        (rc = t->dOh.reserve(s.rows_h * ldp)) || (rc = t->dD.reserve(s.rows_h * HIDDEN)) ||
        (rc = t->mask.reserve(s.rows_h * HIDDEN)) || (rc = t->partf.reserve(t->partf_cap)) ||
        (rc = t->partd.reserve(t->partd_cap)) || (rc = t->gA.reserve(s.big)) || (rc = t->gB.reserve(s.big)) ||
        (rc = t->tS.reserve(s.big)) || (rc = t->tU.reserve(s.big)) || (rc = t->tQ.reserve(s.big)) ||
        (rc = t->tH.reserve(s.big)) || (rc = t->tZ.reserve(s.big)) || (rc = t->tY.reserve(s.big)) ||
        (rc = t->col.reserve(s.colsz)) || (rc = t->up.reserve(s.big)) || (rc = t->kpl.reserve(s.rows_h)))
        return rc;
    // the gradient ping-pong buffers start zeroed (stream-ordered, in step()); their
    // padding column (layer 0's 4th input channel) is never read: bn_bwd_finalize
    // zeroes it through cmap0 = -1
    t->zero_pending = true;
    t->N = N;
    t->T = T;
    return TIK_OK;
}

// fp32 implicit GEMM: 128x128 tiles when they fill the chip (>= 256
// workgroups) and the output is wider than 64 channels, else 64x64 tiles (the
// training batches are 10-40k rows: 128x128 tiles would leave CUs idle, and
// half of each tile would be empty on the 64-channel blocks)
int gemm(const tik::CgemmArgs& a, hipStream_t st) {
    const long long t128 = (long long)((a.M + 127) / 128) * ((a.Nc + 127) / 128);
    const int cfg = (a.Nc > 64 && t128 >= 256) ? tik::CFG_T128x128 : tik::CFG_H64x64;
    HIP_TRY(tik::launch_cgemm(a, cfg, st, tik::PREC_F32));
    return TIK_OK;
}

// a head GEMM on few rows: split-K over the step's fp32 partial buffer
int gemm_splitk(tik_trainer* t, tik::CgemmArgs a, hipStream_t st) {
    a.ksplit = tik::splitk_for(a, 64, 64, 16, 64);
    a.partial = t->partf.p;
    HIP_TRY(tik::launch_cgemm(a, tik::CFG_H64x64, st, tik::PREC_F32));
    return TIK_OK;
}

// train-mode BatchNorm statistics of X [R][C] -> stat, running stats updated
int bn_stats(tik_trainer* t, const float* X, long long R, int C, const int* cmap, long long g, long long b,
             long long rm, long long rv, float* stat, hipStream_t st) {
    int nc = 0;
    HIP_TRY(tik::launch_colstats(X, nullptr, nullptr, nullptr, R, C, t->partd.p, (int)(t->partd_cap / (2LL * C)), &nc,
                                 st));
    HIP_TRY(tik::launch_bn_fwd_finalize(t->partd.p, nc, R, C, cmap, t->P.p + g, t->P.p + b, t->B.p + rm, t->B.p + rv,
                                        t->momentum, BN_EPS, stat, st));
    return TIK_OK;
}

// BatchNorm backward: grads of gamma/beta into G, dx into out (when non-null)
// (Mr: the output of a ReLU between this BatchNorm and Gr, whose backward is folded in)
int bn_back(tik_trainer* t, const float* Gr, const float* X, long long R, int C, const int* cmap, long long g,
            long long b, const float* stat, float* out, hipStream_t st, const float* Mr = nullptr) {
    int nc = 0;
    HIP_TRY(tik::launch_colstats(X, Gr, Mr, stat, R, C, t->partd.p, (int)(t->partd_cap / (2LL * C)), &nc, st));
    HIP_TRY(tik::launch_bn_bwd_finalize(t->partd.p, nc, R, C, cmap, t->P.p + g, stat, t->G.p + g, t->G.p + b,
                                        t->k.p, st));
    if (out) HIP_TRY(tik::launch_bn_bwd_apply(out, Gr, Mr, X, stat, t->k.p, R, C, st));
    return TIK_OK;
}

int colsum(tik_trainer* t, const float* X, long long R, int C, float* dst, hipStream_t st) {
    int nc = 0;
    HIP_TRY(tik::launch_colstats(X, nullptr, nullptr, nullptr, R, C, t->partd.p, (int)(t->partd_cap / (2LL * C)), &nc,
                                 st));
    HIP_TRY(tik::launch_colsum_finalize(t->partd.p, nc, C, dst, st));
    return TIK_OK;
}

int wgrad(tik_trainer* t, const float* A, int lda, const float* Bm, int ldb, int M, int Nn, long long R, float* C,
          int ldc, hipStream_t st, const tik::WgradTaps& g = tik::WgradTaps()) {
    HIP_TRY(tik::launch_wgrad(A, lda, Bm, ldb, M, Nn, R, C, ldc, t->partf.p, t->partf_cap, st, g));
    return TIK_OK;
}

int forward_block(tik_trainer* t, TrainLayer& l, const float* X, int ldx, hipStream_t st) {
    const int N = t->N, co = l.cout;
    const long long pin = (long long)N * l.tin * V, pout = (long long)N * l.tout * V;
    float* P = t->P.p;
    int rc;
    // gcn 1x1 conv + bias (gconv_origin.py:61), then the graph mix (:64)
    if ((rc = gemm(gemm_args(pin, co, V, l.tin, seg32(X, l.wgf.p, l.cinp, ldx, 1, 1, 0, l.tin, l.cinp), P + l.bg, l.Y.p, co), st)))
        return rc;
    HIP_TRY(tik::launch_mix(l.Z.p, l.Y.p, l.aeff.p, 0, (long long)N * l.tin, co, st));
    // tcn.0 BatchNorm (batch statistics) + tcn.1 ReLU (st_gcn_aaai18.py:178-179)
    if ((rc = bn_stats(t, l.Z.p, pin, co, nullptr, l.g1, l.b1, l.rm1, l.rv1, l.st1.p, st))) return rc;
    HIP_TRY(tik::launch_affine(l.H.p, l.Z.p, l.st1.p + 2 * co, l.st1.p + 3 * co, nullptr, nullptr, nullptr, pin, co, 1,
                               st));
    // tcn.2 temporal conv (3x1, stride s, pad 1) + bias (:180-185)
    if ((rc = gemm(gemm_args(pout, co, V, l.tout, seg32(l.H.p, l.wtf.p, co, co, 3, l.stride, 1, l.tin, 3 * co), P + l.bt, l.U.p, co), st)))
        return rc;
    if ((rc = bn_stats(t, l.U.p, pout, co, nullptr, l.g2, l.b2, l.rm2, l.rv2, l.st2.p, st))) return rc;
    // residual (:191-204) and the block's ReLU (:212-214)
    if (l.res == RES_CONV) {
        if ((rc = gemm(gemm_args(pout, co, V, l.tout, seg32(X, l.wrf.p, l.cinp, ldx, 1, l.stride, 0, l.tin, l.cinp), P + l.br, l.Q.p, co), st)))
            return rc;
        if ((rc = bn_stats(t, l.Q.p, pout, co, nullptr, l.g3, l.b3, l.rm3, l.rv3, l.st3.p, st))) return rc;
        HIP_TRY(tik::launch_affine(l.O.p, l.U.p, l.st2.p + 2 * co, l.st2.p + 3 * co, l.Q.p, l.st3.p + 2 * co,
                                   l.st3.p + 3 * co, pout, co, 1, st));
    } else {
        HIP_TRY(tik::launch_affine(l.O.p, l.U.p, l.st2.p + 2 * co, l.st2.p + 3 * co, X, nullptr, nullptr, pout, co, 1,
                                   st));
    }
    return TIK_OK;
}

// dO: gradient of the block output [pout][co]; X: block input [pin][ldx];
// dX: its gradient [pin][ldx] (ldx = cinp; padding columns left untouched)
int backward_block(tik_trainer* t, int li, const float* X, int ldx, const float* dO, float* dX, hipStream_t st) {
    TrainLayer& l = t->L[li];
    const int N = t->N, co = l.cout, ci = l.cin;
    const long long pin = (long long)N * l.tin * V, pout = (long long)N * l.tout * V;
    float* Gd = t->G.p;
    int rc;
    // block ReLU: materialized (gS) only where the identity residual passes it
    // on; otherwise folded into the two BatchNorm backward passes
    const float* gS = dO;
    const float* mO = l.O.p;
    if (l.res == RES_IDEN) {
        HIP_TRY(tik::launch_relu_bwd(t->tS.p, dO, l.O.p, pout * co, st));
        gS = t->tS.p;
        mO = nullptr;
    }
    // tcn.3 BatchNorm -> dU ; residual BatchNorm -> dQ
    if ((rc = bn_back(t, gS, l.U.p, pout, co, nullptr, l.g2, l.b2, l.st2.p, t->tU.p, st, mO))) return rc;
    if (l.res == RES_CONV && (rc = bn_back(t, gS, l.Q.p, pout, co, nullptr, l.g3, l.b3, l.st3.p, t->tQ.p, st, mO)))
        return rc;
    // tcn.2: bias and weight gradients (im2col of H, [ci][tap] = the torch weight layout)
    if ((rc = colsum(t, t->tU.p, pout, co, Gd + l.bt, st))) return rc;
    {
        // implicit im2col of H through the conv's row map (C % 64 == 0 for every block)
        tik::WgradTaps g;
        g.C = co; g.kt = 3; g.s = l.stride; g.pad = 1; g.tin = l.tin; g.tout = l.tout; g.V = V;
        if (co % 64 == 0) {
            if ((rc = wgrad(t, t->tU.p, co, l.H.p, co, co, 3 * co, pout, Gd + l.wt, 3 * co, st, g))) return rc;
        } else {
            HIP_TRY(tik::launch_im2col(t->col.p, l.H.p, co, co, 3, l.stride, 1, N, l.tin, l.tout, V, st));
            if ((rc = wgrad(t, t->tU.p, co, t->col.p, 3 * co, co, 3 * co, pout, Gd + l.wt, 3 * co, st))) return rc;
        }
    }
    // residual conv: bias and weight gradients
    if (l.res == RES_CONV) {
        if ((rc = colsum(t, t->tQ.p, pout, co, Gd + l.br, st))) return rc;
        if (l.stride == 1) {
            if ((rc = wgrad(t, t->tQ.p, co, X, ldx, co, ci, pout, Gd + l.wr, ci, st))) return rc;
        } else if (ci % 64 == 0 && ldx == ci) {   // strided rows of X read in place (tap mode, kt = 1)
            tik::WgradTaps g;
            g.C = ci; g.kt = 1; g.s = l.stride; g.pad = 0; g.tin = l.tin; g.tout = l.tout; g.V = V;
            if ((rc = wgrad(t, t->tQ.p, co, X, ldx, co, ci, pout, Gd + l.wr, ci, st, g))) return rc;
        } else {
            HIP_TRY(tik::launch_im2col(t->col.p, X, ldx, l.cinp, 1, l.stride, 0, N, l.tin, l.tout, V, st));
            if ((rc = wgrad(t, t->tQ.p, co, t->col.p, l.cinp, co, ci, pout, Gd + l.wr, ci, st))) return rc;
        }
    }
    // tcn.2 input gradient: the transposed conv = stride-1 conv of the
    // (zero-upsampled) dU with the tap-flipped, transposed weights
    const float* du = t->tU.p;
    if (l.stride != 1) {
        HIP_TRY(tik::launch_upsample(t->up.p, t->tU.p, co, l.stride, N, l.tin, l.tout, V, st));
        du = t->up.p;
    }
    if ((rc = gemm(gemm_args(pin, co, V, l.tin, seg32(du, l.wtb.p, co, co, 3, 1, 1, l.tin, 3 * co), nullptr, t->tH.p, co), st)))
        return rc;
    // tcn.1 ReLU (folded) + tcn.0 BatchNorm -> dZ
    if ((rc = bn_back(t, t->tH.p, l.Z.p, pin, co, nullptr, l.g1, l.b1, l.st1.p, t->tZ.p, st, l.H.p))) return rc;
    // graph mix: dY = mix(dZ, A_eff^T); edge-importance gradient
    HIP_TRY(tik::launch_mix(t->tY.p, t->tZ.p, l.aeff.p, 1, (long long)N * l.tin, co, st));
    HIP_TRY(tik::launch_mix_grad(l.Y.p, t->tZ.p, (long long)N * l.tin, co, t->B.p + t->plan.A, Gd + l.E, t->partd.p,
                                 (int)(t->partd_cap / 289), st));
    // gcn conv: bias and weight gradients
    if ((rc = colsum(t, t->tY.p, pin, co, Gd + l.bg, st))) return rc;
    if ((rc = wgrad(t, t->tY.p, co, X, ldx, co, ci, pin, Gd + l.wg, ci, st))) return rc;
    // input gradient: dY Wg (+ the residual conv's transposed 1x1, or the identity residual)
    tik::CgemmArgs x = gemm_args(pin, ci, V, l.tin, seg32(t->tY.p, l.wgb.p, co, co, 1, 1, 0, l.tin, co), nullptr, dX, ldx);
    if (l.res == RES_CONV) {
        const float* dq = t->tQ.p;
        if (l.stride != 1) {
            HIP_TRY(tik::launch_upsample(t->up.p, t->tQ.p, co, l.stride, N, l.tin, l.tout, V, st));
            dq = t->up.p;
        }
        x.seg[1] = seg32(dq, l.wrb.p, co, co, 1, 1, 0, l.tin, co);
        x.nseg = 2;
    } else {
        x.resid = t->tS.p; x.ldr = co;
    }
    if ((rc = gemm(x, st))) return rc;
    if (li == t->debug_layer) {
        const float* src[5] = {t->tS.p, t->tU.p, t->tH.p, t->tZ.p, t->tY.p};
        const long long n[5] = {pout * co, pout * co, pin * co, pin * co, pin * co};
        for (int j = 0; j < 5; ++j) {
            if ((rc = t->dbg_b[j].reserve(n[j]))) return rc;
            HIP_TRY(hipMemcpyAsync(t->dbg_b[j].p, src[j], n[j] * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    return TIK_OK;
}

// The keypoint term of a step: one checked launch per body model (poses and grad still unset) and the weight.
struct KpTerm {
    int n = 0;
    tik::FkKpLossArgs a[3];
    float weight = 0.f;
    float* parts = nullptr;   // {pose_mse, kp_mse} on the device, or null
};

// After launch_mse wrote dOh: every model's launch on its rows of Oh (the gradient onto dOh unless the weight is
// 0), then loss_out = pose_mse + weight kp_mse.
int kp_term(tik_trainer* t, KpTerm& kp, long long rows, float* loss_out, hipStream_t st) {
    const int ldp = t->plan.ldp;
    HIP_TRY(hipMemsetAsync(t->kpl.p, 0, rows * sizeof(float), st));   // rows that no list names count as zero
    for (int i = 0; i < kp.n; ++i) {
        tik::FkKpLossArgs& a = kp.a[i];
        if (a.B == 0) continue;
        a.poses = t->Oh.p; a.poses_ld = ldp;
        a.loss = t->kpl.p;
        a.grad = kp.weight > 0.f ? t->dOh.p : nullptr; a.grad_ld = ldp;
        a.grad_scale = kp.weight * (2.f / (51.f * (float)rows));
        a.accumulate = 1;
        if (const int rc = tik::fk_kploss_launch(a, st)) return rc;
    }
    HIP_TRY(tik::launch_kp_loss_reduce(t->kpl.p, rows, kp.weight, loss_out, loss_out, kp.parts, st));
    return TIK_OK;
}

int step(tik_trainer* t, const float* x, int N, int T, const float* target, const float* user_mask,
         unsigned long long seed, float* loss_out, hipStream_t st, KpTerm* kp = nullptr) {
    const TrainPlan& p = t->plan;
    int rc;
    if ((rc = reserve(t, N, T))) return rc;
    if (t->zero_pending) {
        HIP_TRY(hipMemsetAsync(t->gA.p, 0, t->gA.n * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(t->gB.p, 0, t->gB.n * sizeof(float), st));
        t->zero_pending = false;
    }
    if (t->derive_stale) {   // a value written since the last step (tik_trainer_write)
        if ((rc = derive(t, st))) return rc;
        t->derive_stale = false;
    }
    t->version += 1;         // this step changes the weights and running statistics: the eval set refolds
    (void)hipGetLastError();   // the launchers return hipGetLastError(): an earlier call's leftover error must not become the first launch's
    const long long R0 = (long long)N * T, p0 = R0 * V;
    float* P = t->P.p;
    float* Gd = t->G.p;
    // data_bn (BatchNorm1d over the V*C channels, st_gcn_aaai18.py:119-125) on
    // 4-channel padded rows: column 4v+c is channel v*3+c
    HIP_TRY(tik::launch_pad_channels(x, p0, 3, 4, t->x4.p, st));
    if ((rc = bn_stats(t, t->x4.p, R0, 4 * V, t->cmap0.p, p.dg, p.db, p.rm0, p.rv0, t->st0.p, st))) return rc;
    HIP_TRY(tik::launch_affine(t->x0.p, t->x4.p, t->st0.p + 2 * 4 * V, t->st0.p + 3 * 4 * V, nullptr, nullptr, nullptr,
                               R0, 4 * V, 0, st));
    // backbone
    const float* X = t->x0.p;
    int ldx = 4;
    for (TrainLayer& l : t->L) {
        if ((rc = forward_block(t, l, X, ldx, st))) return rc;
        X = l.O.p;
        ldx = l.cout;
    }
    // head: Linear -> LeakyReLU -> Dropout(0.7) -> Linear (pose_trainer.py:89-92)
    const int Tp = t->L.back().tout;
    const long long rows = (long long)N * Tp;
    const int ri = (int)rows;
    const float* feat = t->L.back().O.p;
    if ((rc = gemm_splitk(t, gemm_args(rows, HIDDEN, 1, ri, seg32(feat, P + p.w1, p.feat, p.feat, 1, 1, 0, ri, p.feat), P + p.b1, t->Ph.p, HIDDEN), st)))
        return rc;
    const float* mask = user_mask;
    if (!mask) {
        HIP_TRY(tik::launch_dropout_mask(t->mask.p, rows * HIDDEN, 1.f - DROPOUT_P, seed, st));
        mask = t->mask.p;
    }
    const float scale = 1.f / (1.f - DROPOUT_P);
    HIP_TRY(tik::launch_leaky_dropout(t->Dh.p, t->Ph.p, mask, scale, rows * HIDDEN, st));
    if ((rc = gemm_splitk(t, gemm_args(rows, p.pose_dim, 1, ri, seg32(t->Dh.p, P + p.w2, HIDDEN, HIDDEN, 1, 1, 0, ri, HIDDEN), P + p.b2, t->Oh.p, p.ldp), st)))
        return rc;
    // MSE loss (PoseLosses, pose_trainer.py:42-50) and its gradient
    HIP_TRY(tik::launch_mse(t->Oh.p, p.ldp, target, rows, p.pose_dim, t->dOh.p, loss_out, st));
    if (kp && (rc = kp_term(t, *kp, rows, loss_out, st))) return rc;
    // head backward
    if ((rc = colsum(t, t->dOh.p, rows, p.ldp, t->tS.p, st))) return rc;
    HIP_TRY(hipMemcpyAsync(Gd + p.b2, t->tS.p, p.pose_dim * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = wgrad(t, t->dOh.p, p.ldp, t->Dh.p, HIDDEN, p.pose_dim, HIDDEN, rows, Gd + p.w2, HIDDEN, st))) return rc;
    if ((rc = gemm_splitk(t, gemm_args(rows, HIDDEN, 1, ri, seg32(t->dOh.p, t->w2b.p, p.ldp, p.ldp, 1, 1, 0, ri, p.ldp), nullptr, t->dD.p, HIDDEN), st)))
        return rc;
    HIP_TRY(tik::launch_leaky_dropout_bwd(t->dD.p, t->dD.p, t->Ph.p, mask, scale, rows * HIDDEN, st));
    if ((rc = colsum(t, t->dD.p, rows, HIDDEN, Gd + p.b1, st))) return rc;
    if ((rc = wgrad(t, t->dD.p, HIDDEN, feat, p.feat, HIDDEN, p.feat, rows, Gd + p.w1, p.feat, st))) return rc;
    float* gOut = t->gA.p;
    float* gIn = t->gB.p;
    if ((rc = gemm(gemm_args(rows, p.feat, 1, ri, seg32(t->dD.p, t->w1b.p, HIDDEN, HIDDEN, 1, 1, 0, ri, HIDDEN), nullptr, gOut, p.feat), st)))
        return rc;
    // backbone backward
    for (int i = (int)t->L.size() - 1; i >= 0; --i) {
        const float* Xi = i > 0 ? t->L[i - 1].O.p : t->x0.p;
        const int ldi = i > 0 ? t->L[i - 1].cout : 4;
        if ((rc = backward_block(t, i, Xi, ldi, gOut, gIn, st))) return rc;
        if (t->debug) {
            const size_t n = (size_t)N * t->L[i].tin * V * ldi;
            if ((rc = t->dbg_dx[i].reserve(n))) return rc;
            HIP_TRY(hipMemcpyAsync(t->dbg_dx[i].p, gIn, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        std::swap(gOut, gIn);
    }
    // data_bn gamma / beta gradients (no input gradient: x is data)
    if ((rc = bn_back(t, gOut, t->x4.p, R0, 4 * V, t->cmap0.p, p.dg, p.db, t->st0.p, nullptr, st))) return rc;
    // Adam
    t->steps += 1;
    const double bc1 = 1.0 - std::pow(t->beta1, (double)t->steps);
    const double bc2 = 1.0 - std::pow(t->beta2, (double)t->steps);
    HIP_TRY(tik::launch_adam(P, Gd, t->M.p, t->Vv.p, t->np, t->lr, t->beta1, t->beta2, t->eps, bc1, bc2, st));
    return derive(t, st);
}

}  // namespace

extern "C" int tik_trainer_step(tik_trainer_t t, const float* x, int N, int T, const float* target,
                                const float* dropout_mask, unsigned long long seed, float* loss, void* stream) {
    if (!t || !x || !target || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "tik_trainer_step: bad arguments");
    // checked up front, before any kernel updates running statistics
    if (!batch_fits_32bit(t->plan, N, T))
        return fail(TIK_E_INVALID, "tik_trainer_step: batch of %d x %d frames too large", N, T);
    if (N * T < 2) return fail(TIK_E_INVALID, "tik_trainer_step: BatchNorm needs more than one value per channel");
    return step(t, x, N, T, target, dropout_mask, seed, loss ? loss : t->loss.p, (hipStream_t)stream);
}

extern "C" int tik_trainer_step_kp(tik_trainer_t t, const float* x, int N, int T, const float* target,
                                   const float* dropout_mask, unsigned long long seed, const tik_kp_loss* kp, float* loss,
                                   float* loss_parts, void* stream) {
    const char* who = "tik_trainer_step_kp";
    if (!t || !x || !target || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "%s: bad arguments", who);
    if (!batch_fits_32bit(t->plan, N, T)) return fail(TIK_E_INVALID, "%s: batch of %d x %d frames too large", who, N, T);
    if (N * T < 2) return fail(TIK_E_INVALID, "%s: BatchNorm needs more than one value per channel", who);
    float* lo = loss ? loss : t->loss.p;
    if (!kp) {   // exactly the launches of tik_trainer_step
        if (loss_parts) return fail(TIK_E_INVALID, "%s: loss_parts needs a keypoint term", who);
        return step(t, x, N, T, target, dropout_mask, seed, lo, (hipStream_t)stream);
    }
    // every refusal before any kernel updates running statistics
    if (t->plan.pose_dim != tik::LMR_N)
        return fail(TIK_E_INVALID, "%s: the keypoint term needs pose_dim %d, the model has %d", who, tik::LMR_N, t->plan.pose_dim);
    if (kp->n_models < 1 || kp->n_models > 3) return fail(TIK_E_INVALID, "%s: n_models must be 1..3, got %d", who, kp->n_models);
    if (!kp->kps) return fail(TIK_E_INVALID, "%s: null kps", who);
    if (!(kp->weight >= 0.f) || !std::isfinite(kp->weight))
        return fail(TIK_E_INVALID, "%s: weight must be >= 0 and finite, got %g", who, (double)kp->weight);
    const long long R = (long long)N * frame_chain(t->plan, T, nullptr);
    KpTerm term;
    term.n = kp->n_models;
    term.weight = kp->weight;
    term.parts = loss_parts;
    long long named = 0;
    for (int i = 0; i < kp->n_models; ++i) {
        if (!kp->fk[i]) return fail(TIK_E_INVALID, "%s: fk[%d] is null", who, i);
        const bool all = kp->n_models == 1 && !kp->rows[0];
        if (!all && !kp->rows[i]) return fail(TIK_E_INVALID, "%s: rows[%d] is null", who, i);
        const long long n = all ? R : kp->n_rows[i];
        if (n < 0) return fail(TIK_E_INVALID, "%s: n_rows[%d] must be >= 0, got %lld", who, i, n);
        named += n;
        if (named > R) return fail(TIK_E_INVALID, "%s: the row lists name %lld rows, the batch has %lld", who, named, R);
        // poses, loss and grad are the trainer's own buffers, set at the launch; kps stands in for them in the check
        float* own = const_cast<float*>(kp->kps);
        if (const int rc = tik::fk_kploss_args(kp->fk[i], who, own, t->plan.ldp, kp->kps, kp->betas, kp->betas_ld, kp->joint_w, 0,
                                               nullptr, kp->rows[i], n > 0 ? (int)n : 1, own, nullptr, t->plan.ldp, 0.f, 1, term.a[i]))
            return rc;
        term.a[i].B = (int)n;
    }
    return step(t, x, N, T, target, dropout_mask, seed, lo, (hipStream_t)stream, &term);
}
