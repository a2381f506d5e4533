// train_eval.cpp — the eval pass on a trainer's live weights (tik_trainer_eval):
// eval-mode BatchNorm folded into the GEMM operands on the device, then the
// forward without dropout. Reads P / B / the derived layouts; writes only the
// eval set and the eval workspace.
#include <hip/hip_runtime.h>

#include "train_model.h"

using namespace tik_host;
using namespace tik_train;

namespace {

// The eval set from the live parameters, running statistics and derived
// layouts: one batched launch over a descriptor table built once.
int fold(tik_trainer* t, hipStream_t st) {
    if (!t->fold.p) {
        const TrainPlan& p = t->plan;
        const float* P = t->P.p;
        const float* B = t->B.p;
        std::vector<tik::FoldDesc> d;
        auto bn = [&](long long g, long long b, long long rm, long long rv) {
            return tik::BnRef{P + g, P + b, B + rm, B + rv};
        };
        auto add = [&](int kind, int rows, int cols, float* dst, const float* src, const float* aux, tik::BnRef b1,
                       tik::BnRef b2, const int* cmap) {
            tik::FoldDesc q{kind, rows, cols, dst, src, aux, b1, b2, cmap, 0};
            d.push_back(q);
        };
        const tik::BnRef none{nullptr, nullptr, nullptr, nullptr};
        add(tik::FOLD_DATA, 2, 4 * V, t->dbn_e.p, nullptr, nullptr, bn(p.dg, p.db, p.rm0, p.rv0), none, t->cmap0.p);
        for (TrainLayer& l : t->L) {
            const int co = l.cout;
            const tik::BnRef b1 = bn(l.g1, l.b1, l.rm1, l.rv1), b2 = bn(l.g2, l.b2, l.rm2, l.rv2);
            const bool rc_ = l.res == RES_CONV;
            const tik::BnRef b3 = rc_ ? bn(l.g3, l.b3, l.rm3, l.rv3) : none;
            add(tik::FOLD_SCALE, co, l.cinp, l.wg_e.p, l.wgf.p, nullptr, b1, none, nullptr);
            add(tik::FOLD_BIAS2, V, co, l.b2_e.p, P + l.bg, l.aeff.p, b1, none, nullptr);
            add(tik::FOLD_SCALE, co, 3 * co, l.wt_e.p, l.wtf.p, nullptr, b2, none, nullptr);
            add(tik::FOLD_BIAST, 1, co, l.bT_e.p, P + l.bt, rc_ ? P + l.br : nullptr, b2, b3, nullptr);
            if (rc_) add(tik::FOLD_SCALE, co, l.cinp, l.wr_e.p, l.wrf.p, nullptr, b3, none, nullptr);
        }
        t->fold_blocks = tik::fold_batch_blocks(d.data(), (int)d.size());
        if (const int rc = t->fold.upload(d)) return rc;
    }
    HIP_TRY(tik::launch_fold_batch(t->fold.p, (int)t->fold.n, t->fold_blocks, BN_EPS, st));
    return TIK_OK;
}

// Eval-mode forward on the live weights: pad, folded data_bn, two GEMM launches
// per block (gcn + graph mix + ReLU; temporal conv + residual + ReLU), the head
// without dropout. No split-K anywhere: a window's poses do not depend on
// what else is in the batch.
int eval(tik_trainer* t, const float* x, int N, int T, const float* target, float* poses, float* loss, hipStream_t st) {
    const TrainPlan& p = t->plan;
    int rc;
    if (t->derive_stale) {
        if ((rc = derive(t, st))) return rc;
        t->derive_stale = false;
    }
    // workspace: z (a block's graph-mix output), the activation ping-pong, the head
    Frames* const fr = t->ev.fr.data();
    frame_chain(p, T, fr);
    const EvalSizes s = eval_sizes(p, fr, N, T);
    const long long rows = s.rows;
    const int ri = (int)rows;
    if ((rc = t->ev.x4.reserve(s.p0 * 4)) || (rc = t->ev.x0.reserve(s.p0 * 4)) || (rc = t->ev.z.reserve(s.zsz)) ||
        (rc = t->ev.a0.reserve(s.asz)) || (rc = t->ev.a1.reserve(s.asz)) || (rc = t->ev.ph.reserve(rows * HIDDEN)) ||
        (rc = t->ev.oh.reserve(rows * p.pose_dim)) ||
        (rc = t->ev.part.reserve((size_t)tik::mse_eval_blocks(rows * p.pose_dim))))
        return rc;
    (void)hipGetLastError();   // as in the step: an earlier call's leftover error must not become the first launch's
    if (t->folded_at != t->version) {
        if ((rc = fold(t, st))) return rc;
        t->folded_at = t->version;
    }
    HIP_TRY(tik::launch_pad_channels(x, s.p0, 3, 4, t->ev.x4.p, st));
    HIP_TRY(tik::launch_affine(t->ev.x0.p, t->ev.x4.p, t->dbn_e.p, t->dbn_e.p + 4 * V, nullptr, nullptr, nullptr,
                               (long long)N * T, 4 * V, 0, st));
    const float* X = t->ev.x0.p;
    int ldx = 4;
    float* bufs[2] = {t->ev.a0.p, t->ev.a1.p};
    int which = 0;
    for (size_t i = 0; i < t->L.size(); ++i) {
        const TrainLayer& l = t->L[i];
        const int co = l.cout, tin = fr[i].tin, to = fr[i].tout;
        tik::CgemmArgs g = gemm_args((long long)N * tin * V, co, V, tin, seg32(X, l.wg_e.p, l.cinp, ldx, 1, 1, 0, tin, l.cinp),
                                     l.b2_e.p, t->ev.z.p, co);
        g.amix = l.aeff.p; g.act = tik::ACT_RELU;
        g.mix_sparse = t->mix_sparse ? 1 : 0;
        HIP_TRY(tik::launch_cgemm(g, tik::CFG_G272x64, st, tik::PREC_F32));
        tik::CgemmArgs u = gemm_args((long long)N * to * V, co, V, to, seg32(t->ev.z.p, l.wt_e.p, co, co, 3, l.stride, 1, tin, 3 * co),
                                     l.bT_e.p, bufs[which], co);
        if (l.res == RES_CONV) {
            u.seg[1] = seg32(X, l.wr_e.p, l.cinp, ldx, 1, l.stride, 0, tin, l.cinp);
            u.nseg = 2;
        } else {
            u.resid = X; u.ldr = ldx;
        }
        u.act = tik::ACT_RELU;
        HIP_TRY(tik::launch_cgemm(u, co >= 128 ? tik::CFG_T128x128 : tik::CFG_T256x64, st, tik::PREC_F32));
        X = bufs[which];
        ldx = co;
        which ^= 1;
    }
    // head: Linear + LeakyReLU (Dropout is the identity), Linear (pose_trainer.py:89-92)
    const float* P = t->P.p;
    tik::CgemmArgs h = gemm_args(rows, HIDDEN, 1, ri, seg32(X, P + p.w1, p.feat, p.feat, 1, 1, 0, ri, p.feat), P + p.b1,
                                 t->ev.ph.p, HIDDEN);
    h.act = tik::ACT_LEAKY;
    HIP_TRY(tik::launch_cgemm(h, tik::CFG_H64x64, st, tik::PREC_F32));
    float* O = poses ? poses : t->ev.oh.p;
    const tik::CgemmArgs o = gemm_args(rows, p.pose_dim, 1, ri, seg32(t->ev.ph.p, P + p.w2, HIDDEN, HIDDEN, 1, 1, 0, ri, HIDDEN),
                                       P + p.b2, O, p.pose_dim);
    HIP_TRY(tik::launch_cgemm(o, tik::CFG_H64x64, st, tik::PREC_F32));
    if (loss) HIP_TRY(tik::launch_mse_eval(O, p.pose_dim, target, rows, p.pose_dim, loss, t->ev.part.p, st));
    return TIK_OK;
}

}  // namespace

extern "C" int tik_trainer_eval(tik_trainer_t t, const float* x, int N, int T, const float* target, float* poses,
                                float* loss, void* stream) {
    if (!t || !x || N <= 0 || T <= 0 || (loss && !target))
        return fail(TIK_E_INVALID, "tik_trainer_eval: bad arguments (null handle or input, or a loss without a target)");
    if (!batch_fits_32bit(t->plan, N, T))
        return fail(TIK_E_INVALID, "tik_trainer_eval: batch of %d x %d frames too large", N, T);
    return eval(t, x, N, T, target, poses, loss, (hipStream_t)stream);
}
