// forward.cpp — the launch sequence of the IK forward pass and its workspaces.
//
// Forward of PoseRegressor (pose_trainer.py:94-133) on channels-last data:
//   xb  = data_bn(x)                                      st_gcn_aaai18.py:119-125
//   per block l (st_gcn_aaai18.py:208-214):
//     z   = ReLU( mix_A( x . Wg'^T ) + bias2[w][c] )      gcn + tcn.0 BN + ReLU (folded)
//     out = ReLU( sum_tap z[s t'+tap-1] . Wt'_tap^T + res + bT )   tcn.2 + tcn.3 BN + residual
//   feat = out_7 viewed (N*T', 17*256)                    st_gcn_aaai18.py:131-132
//   poses = (LeakyReLU(feat . W0^T + b0)) . W3^T + b3      pose_trainer.py:89-92
#include <hip/hip_runtime.h>

#include <algorithm>

#include "misc.h"
#include "model.h"
#include "xtws.h"

using namespace tik_host;

namespace tik_host {

static tik::Seg mkseg(const float* src, const float* w, const SplitW3& s3, int cin, int ld, int kt, int stride, int pad,
                      int tin, int ldw) {
    tik::Seg s{src, w, cin, ld, kt, stride, pad, tin, ldw};
    s.cin8 = s3.cin8; s.ldw8 = s3.ldw8;
    for (int i = 0; i < 3; ++i) s.wb[i] = s3.p[i].p;
    return s;
}

// ---------------------------------------------------------------- one block, cgemm.hip
int Layer::forward(const float* x, int ld, int N, int tin, float* z, float* out, hipStream_t st, int prec,
                   float* part) const {
    const int to = tout(tin, stride);
    tik::CgemmArgs g{};
    g.M = N * tin * V; g.Nc = cout; g.V = V; g.tout = tin;
    g.seg[0] = mkseg(x, wg.p, s3g, cinp, ld, 1, 1, 0, tin, cinp);
    g.nseg = 1;
    g.bias = bias2.p; g.out = z; g.ldo = cout; g.amix = amix.p; g.act = tik::ACT_RELU;
    g.mix_sparse = mix_sparse ? 1 : 0;
    const double px_in = (double)N * tin * V, px_out = (double)N * to * V;
    {
        const std::string lab = "G272x64.L" + std::to_string(index);
        ProfScope p(lab.c_str(), gcn_work(px_in, cin, cout, V), st);
        HIP_TRY(tik::launch_cgemm(g, tik::CFG_G272x64, st, prec));
    }

    tik::CgemmArgs t{};
    t.M = N * to * V; t.Nc = cout; t.V = V; t.tout = to;
    t.seg[0] = mkseg(z, wt.p, s3t, cout, cout, TK, stride, 1, tin, TK * cout);
    t.nseg = 1;
    if (res == RES_CONV) {
        t.seg[1] = mkseg(x, wr.p, s3r, cinp, ld, 1, stride, 0, tin, cinp);
        t.nseg = 2;
    } else if (res == RES_IDEN) {
        t.resid = x; t.ldr = ld;
    }
    t.bias = biasT.p; t.out = out; t.ldo = cout; t.act = tik::ACT_RELU;
    const bool big = cout >= 128;
    // 64-channel layers: 256x64 tiles for fp32; 128x64 for bf16x3 (two register
    // staging sets of a 256-row tile would cost a wave per SIMD)
    const int cfg = big ? tik::CFG_T128x128 : (prec == tik::PREC_F32 ? tik::CFG_T256x64 : tik::CFG_T128x64);
    const std::string lab = std::string(big ? "T128x128.L" : (cfg == tik::CFG_T256x64 ? "T256x64.L" : "T128x64.L")) +
                            std::to_string(index);
    if (part) {   // small batches: split K over more workgroups (latency path)
        t.ksplit = tik::splitk_for(t, cfg == tik::CFG_T256x64 ? 256 : 128, big ? 128 : 64,
                                   prec == tik::PREC_F32 ? 16 : 32, 64);
        t.partial = part;
    }
    ProfScope p(lab.c_str(), tcn_work(px_in, px_out, cin, cout, res), st);
    HIP_TRY(tik::launch_cgemm(t, cfg, st, prec));
    return TIK_OK;
}

// ---------------------------------------------------------------- one block, bf16x3 on fp32 activations
int Layer::spatial_x(const float* x, int ld, int N, int tin, float* z, hipStream_t st, int ncu, const RawInput* raw) const {
    const long long rin = (long long)N * tin * V;
    if (raw) {   // layer0.hip
        ProfScope p("G0f_raw.L0", gcn_work((double)rin, cin, cout, V, GCN_RAW0), st);
        HIP_TRY(tik::launch_gcn0_f32(raw->kp, (int)rin, V, cin, raw->bn_sc, raw->bn_sh, wg.p, cinp, bias2.p, amix.p, mix_sparse ? 1 : 0,
                                     cout, z, cout, raw->xb4, st));
    } else if (xgw_path()) {   // xgraph.hip
        tik::XGraphArgs g{};
        g.nframes = N * tin; g.x = x; g.ldx = ld; g.cin = cin; g.cout = cout; g.wp = xgw.p;
        g.bias2 = bias2.p; g.amix = amix.p; g.mix_sparse = mix_sparse ? 1 : 0; g.out = z; g.ldo = cout;
        g.nts = 1; g.trash = xtrash;
        const std::string lab = "XGW.L" + std::to_string(index);
        ProfScope p(lab.c_str(), gcn_work((double)rin, cin, cout, V), st);
        p.out(z, (size_t)rin * cout * 4);
        HIP_TRY(launch_xgraph_traced(g, ncu, st, lab.c_str()));
    } else {   // xgemm.hip
        tik::XArgs g{};
        g.M = (int)rin; g.Nc = cout; g.V = V; g.tout = tin;
        g.seg[0] = tik::XSeg{x, ld, cin, 1, 1, 0, tin, rin};
        g.nseg = 1; g.wp = xg.p;
        g.bias = bias2.p; g.amix = amix.p; g.mix_sparse = mix_sparse ? 1 : 0; g.out = z; g.ldo = cout; g.act = tik::ACT_RELU;
        g.nts = 1;
        const std::string lab = std::string(xg_bn == 128 ? "XG128.L" : "XG64.L") + std::to_string(index);
        ProfScope p(lab.c_str(), gcn_work((double)rin, cin, cout, V), st);
        p.out(z, (size_t)rin * cout * 4);
        HIP_TRY(launch_xgemm_traced(g, xg_bn, tik::EPI_GRAPH, st, lab.c_str()));
    }
    return TIK_OK;
}

int Layer::temporal_x(const float* x, int ld, int N, int tin, const float* z, float* out, hipStream_t st, int ncu,
                      const RawInput* raw, const FusedNext* fg) const {
    const int to = tout(tin, stride);
    const long long rin = (long long)N * tin * V, rout = (long long)N * to * V;
    const double px_in = (double)rin, px_out = (double)rout;
    if (xtws_path(raw != nullptr, ld, tin)) {   // xtws.hip
        tik::XTConvArgs c{};
        c.M = (int)rout; c.T = tin; c.z = z; c.ldz = cout; c.x = x; c.ldx = ld; c.wp = xtw.p; c.bias = biasT.p;
        c.out = out; c.ldo = cout; c.nts = 1; c.trash = xtrash;
        Work w = tcn_work(px_in, px_out, cin, cout, RES_IDEN);
        if (fg) {   // + block l+1's gcn: its algorithmic FLOPs, its z written (out is not re-read)
            const Layer& gn = *fg->layer;
            c.wg = gn.xgw.p; c.bias2 = gn.bias2.p; c.amix = gn.amix.p; c.mix_sparse = gn.mix_sparse ? 1 : 0;
            c.zout = fg->zn; c.ldzo = gn.cout;
            w = w + gcn_work(px_out, gn.cin, gn.cout, V, GCN_FUSED);
        }
        const std::string lab = (fg ? "XTWG.L" : "XTW.L") + std::to_string(index);
        ProfScope p(lab.c_str(), w, st);
        p.out(out, (size_t)rout * cout * 4);
        HIP_TRY(tik::launch_xtws(c, ncu, st));
        return TIK_OK;
    }
    // xgemm.hip
    tik::XArgs t{};
    t.M = (int)rout; t.Nc = cout; t.V = V; t.tout = to;
    t.seg[0] = tik::XSeg{z, cout, cout, TK, stride, 1, tin, rin};
    t.nseg = 1;
    if (raw) {
        t.rx = raw->xb4; t.rxc = cin; t.rw = wr0.p;
    } else if (res == RES_CONV) {
        t.seg[1] = tik::XSeg{x, ld, cin, 1, stride, 0, tin, rin};
        t.nseg = 2;
    } else if (res == RES_IDEN) {
        t.idn = tik::XSeg{x, ld, cin, 1, 1, 0, to, rin};
    }
    t.wp = xt.p;
    if (tik::xgemm_kmain(t) != xt_ks) return fail(TIK_E_INVALID, "layer %d: xgemm K steps %d != packed %d", index, tik::xgemm_kmain(t), xt_ks);
    t.bias = biasT.p; t.out = out; t.ldo = cout; t.act = tik::ACT_RELU;
    t.nts = 1;
    t.trash = xtrash;
    const bool pt = xpt_path();
    const std::string lab = std::string(xt_bn == 128 ? (pt ? "XP128.L" : "XT128.L") : (pt ? "XP64.L" : "XT64.L")) +
                            std::to_string(index);
    ProfScope p(lab.c_str(), tcn_work(px_in, px_out, cin, cout, raw ? RES_RAW0 : res), st);
    p.out(out, (size_t)rout * cout * 4);
    if (pt) HIP_TRY(tik::launch_xgemm_pt(t, xt_bn, ncu, st));
    else HIP_TRY(launch_xgemm_traced(t, xt_bn, tik::EPI_BIAS, st, lab.c_str()));
    return TIK_OK;
}

// ---------------------------------------------------------------- backbone
// Backbone on fp32 activations, cgemm.hip (both precisions; split-K for small batches).
static int backbone(tik_model* m, const float* x, int N, int T, float** feat_out, int* tout, hipStream_t st,
                    const Workspace& w) {
    const int V = m->V;
    {
        const double px = (double)N * T * V;
        ProfScope p("data_bn", Work{2.0 * px * m->C0, 4.0 * px * (m->C0 + 4)}, st);
        HIP_TRY(tik::launch_data_bn(x, N * T * V, V, m->C0, m->bn_sc.p, m->bn_sh.p, w.xb.p, st));
    }
    const float* cur = w.xb.p;
    int ld = 4, t = T, rc;
    float* bufs[2] = {w.a0.p, w.a1.p};
    int which = 0;
    for (const Layer& L : m->layers) {
        float* o = bufs[which];
        if ((rc = L.forward(cur, ld, N, t, w.z.p, o, st, m->prec, w.part.p))) return rc;
        cur = o; ld = L.cout; t = Layer::tout(t, L.stride); which ^= 1;
    }
    *feat_out = const_cast<float*>(cur);
    *tout = t;
    return TIK_OK;
}

// Blocks 0 and 1 as whole-block kernels (xblock.hip): block 0 from the raw
// keypoints writes its output as bf16x3 planes into the z workspace, block 1
// reads them and writes fp32 rows to `out`.
static int blocks01_x(tik_model* m, const float* x, int N, int T, float* out, hipStream_t st, const Workspace& w) {
    const Layer& L0 = m->layers[0];
    const Layer& L1 = m->layers[1];
    const double px = (double)N * T * m->V;
    unsigned short* p3 = reinterpret_cast<unsigned short*>(w.z.p);
    tik::XBlkArgs b{};
    b.nframes = N * T; b.T = T;
    b.xraw = x; b.c0 = m->C0; b.bn_sc = m->bn_sc.p; b.bn_sh = m->bn_sh.p; b.wg0 = L0.wg.p; b.ldwg0 = L0.cinp; b.rw = L0.wr0.p;
    b.wtp = L0.xbt.p; b.bias2 = L0.bias2.p; b.amix = L0.amix.p; b.mix_sparse = L0.mix_sparse ? 1 : 0; b.bias = L0.biasT.p;
    b.out_p3 = p3; b.trash = L0.xtrash;
    {   // in: the raw keypoints; out: 384 B of planes per pixel
        const double fl = gcn_work(px, L0.cin, 64, 17).flops + tcn_work(px, px, L0.cin, 64, RES_CONV).flops;
        ProfScope p("XB0.L0", Work{fl, px * (4.0 * m->C0 + 384.0)}, st);
        p.out(p3, (size_t)px * 384);
        HIP_TRY(launch_xblock_traced(b, true, m->ncu, st, "XB0.L0"));
    }
    tik::XBlkArgs c{};
    c.nframes = N * T; c.T = T; c.xp3 = p3;
    c.wgp = L1.xbg.p; c.wtp = L1.xbt.p; c.bias2 = L1.bias2.p; c.amix = L1.amix.p; c.mix_sparse = L1.mix_sparse ? 1 : 0;
    c.bias = L1.biasT.p; c.out_f = out; c.trash = L1.xtrash;
    {   // in: the planes; out: 256 B of fp32 per pixel
        const double fl = gcn_work(px, 64, 64, 17).flops + tcn_work(px, px, 64, 64, RES_IDEN).flops;
        ProfScope p("XB1.L1", Work{fl, px * (384.0 + 256.0)}, st);
        p.out(out, (size_t)px * 256);
        HIP_TRY(launch_xblock_traced(c, false, m->ncu, st, "XB1.L1"));
    }
    return TIK_OK;
}

// Backbone on fp32 activations with the bf16x3 kernels. Layer 0 runs from the
// raw keypoints (data_bn folded into its gcn kernel).
static int backbone_x(tik_model* m, const float* x, int N, int T, float** feat_out, int* tout, hipStream_t st,
                      const Workspace& w) {
    const float* cur = nullptr;
    int ld = 0, t = T, rc;
    float* bufs[2] = {w.a0.p, w.a1.p};
    int which = 0;
    const bool xblk = m->use_xblk();
    if (xblk) {
        if ((rc = blocks01_x(m, x, N, T, w.a1.p, st, w))) return rc;
        cur = w.a1.p; ld = 64;
    }
    // The z buffers alternate (w.z.p, w.z2.p): a fused launch (xtws FG) reads z(l) halo
    // rows of neighbouring tiles while it writes z(l+1) into the other one.
    // z_made: the current block's z, when the previous block's launch made it.
    float* zbuf[2] = {w.z.p, w.z2.p};
    float* z_made = nullptr;
    int zw = 0;
    const RawInput raw{x, m->bn_sc.p, m->bn_sh.p, w.xb.p};
    const int nl = (int)m->layers.size();
    for (int l = 0; l < nl; ++l) {
        const Layer& L = m->layers[l];
        if (xblk && L.index < 2) continue;
        float* o = bufs[which];
        const RawInput* r = L.index == 0 ? &raw : nullptr;
        float* z = z_made ? z_made : zbuf[zw];
        const FusedNext fg{l + 1 < nl ? &m->layers[l + 1] : nullptr, zbuf[z == zbuf[0] ? 1 : 0]};
        const bool fuse = fg.layer && w.z2.p && L.index > 0 && L.xtws_path(false, ld, t) && L.fuses_gcn_of(*fg.layer);
        if (!z_made && (rc = L.spatial_x(cur, ld, N, t, z, st, m->ncu, r))) return rc;
        if ((rc = L.temporal_x(cur, ld, N, t, z, o, st, m->ncu, r, fuse ? &fg : nullptr))) return rc;
        z_made = fuse ? fg.zn : nullptr;
        zw = z == zbuf[0] ? 0 : 1;
        cur = o; ld = L.cout; t = Layer::tout(t, L.stride); which ^= 1;
    }
    *feat_out = const_cast<float*>(cur);
    *tout = t;
    return TIK_OK;
}

// ---------------------------------------------------------------- head
// One Linear layer of the head on cgemm.hip with split-K (few rows: the K loop spread over
// workgroups instead of run serially by the handful of row tiles; ks > 0: that many K
// slices whatever the row count)
static int linear_splitk(tik_model* m, const char* label, const float* in, int K, const DevBuf& W, const SplitW3& s3,
                         const DevBuf& b, int Nc, int act, int rows, float* out, float* part, hipStream_t st, int ks = 0) {
    tik::CgemmArgs h{};
    h.M = rows; h.Nc = Nc; h.V = 1; h.tout = rows;
    h.seg[0] = mkseg(in, W.p, s3, K, K, 1, 1, 0, rows, K);
    h.nseg = 1; h.bias = b.p; h.out = out; h.ldo = Nc; h.act = act;
    h.ksplit = ks > 0 ? ks : tik::splitk_for(h, 64, 64, m->prec == tik::PREC_F32 ? 16 : 32, 64);
    h.partial = part;
    ProfScope pr(label, Work{2.0 * rows * K * Nc, 4.0 * ((double)rows * (K + Nc) + (double)K * Nc)}, st);
    HIP_TRY(tik::launch_cgemm(h, tik::CFG_H64x64, st, m->prec));
    return TIK_OK;
}
// pose_regressor.3 (hidden -> pose_dim, pose_trainer.py:92)
static int head3_splitk(tik_model* m, const float* hid, int rows, float* poses, float* part, hipStream_t st, int ks = 0) {
    return linear_splitk(m, "H64x64.head3", hid, m->hidden, m->w3, m->s33, m->b3, m->pose_dim, tik::ACT_NONE, rows, poses, part, st, ks);
}
// the whole head on fp32 features (K = 4352, LeakyReLU, then pose_regressor.3)
static int head_splitk(tik_model* m, const float* f, int rows, float* poses, float* hid, float* part, hipStream_t st) {
    if (const int rc = linear_splitk(m, "H64x64.head0", f, m->feat, m->w0, m->s30, m->b0, m->hidden, tik::ACT_LEAKY, rows, hid, part, st))
        return rc;
    return head3_splitk(m, hid, rows, poses, part, st);
}

// Head of the bf16x3 path: pose_regressor.0 (feat -> hidden, LeakyReLU,
// pose_trainer.py:89-91) on xgemm.hip, its K = feat loop split into a fixed
// number of slices (the frames are few: 4096 rows at B = 1024, 128 tiles) and
// the slices summed in a fixed order by the reduce kernel (+ bias, LeakyReLU);
// then pose_regressor.3 with split-K as head_splitk.
static int head_x(tik_model* m, const float* f, int rows, float* poses, const Workspace& w, hipStream_t st) {
    if (!m->xh0.p) return head_splitk(m, f, rows, poses, w.hid.p, w.part.p, st);
    tik::XArgs h{};
    h.M = rows; h.Nc = m->hidden; h.V = 1; h.tout = rows;
    h.seg[0] = tik::XSeg{f, m->feat, m->feat, 1, 1, 0, rows, rows};
    h.nseg = 1; h.wp = m->xh0.p;
    {   // K slices: the fixed count (4: 512 workgroups at 4096 rows), each non-empty
        const int ks = tik::xgemm_kmain(h), kper = (ks + m->XHEAD_KS - 1) / m->XHEAD_KS;
        h.ksplit = (ks + kper - 1) / kper;
    }
    if (h.ksplit > 1) {
        h.out = w.part.p; h.act = tik::ACT_NONE;
    } else {
        h.out = w.hid.p; h.bias = m->b0.p; h.act = tik::ACT_LEAKY;
    }
    h.ldo = m->hidden;
    {
        ProfScope pr("XH128.head0", Work{2.0 * rows * m->feat * m->hidden,
                                         4.0 * ((double)rows * (m->feat + (double)h.ksplit * m->hidden) + (double)m->feat * m->hidden)}, st);
        HIP_TRY(tik::launch_xgemm(h, 128, tik::EPI_BIAS, st));
    }
    if (h.ksplit > 1) {
        ProfScope pr("XR.head0", Work{(double)rows * m->hidden * h.ksplit, 4.0 * (double)rows * m->hidden * (h.ksplit + 1)}, st);
        HIP_TRY(tik::launch_xgemm_splitk_reduce(w.part.p, h.ksplit, rows, m->hidden, m->b0.p, tik::ACT_LEAKY, w.hid.p,
                                                m->hidden, st));
    }
    // pose_regressor.3: a fixed K split too (4 slices of 128), so no row's
    // arithmetic depends on the batch size
    return head3_splitk(m, w.hid.p, rows, poses, w.part.p, st, std::min(4, std::max(1, m->hidden / 128)));
}

// ---------------------------------------------------------------- batches
// Windows per xgemm call: every fp32 activation tensor the DMA reads stays
// below 2 GiB (32-bit buffer offsets), block 0's bf16x3-plane output of the
// whole-block path included.
static int x_chunk(const tik_model* m, int T) {
    long long worst = 1;
    int t = T;
    for (const Layer& L : m->layers) {
        worst = std::max(worst, (long long)t * m->V * L.cout * 4);   // z
        t = Layer::tout(t, L.stride);
        worst = std::max(worst, (long long)t * m->V * L.cout * 4);   // out
    }
    if (m->use_xblk()) worst = std::max(worst, (long long)T * m->V * (long long)(XB0_P3_FLOATS * 4));
    const long long lim = (1LL << 31) - (1LL << 20);
    const int c = (int)std::max(1LL, lim / worst);
    return m->x_chunk_max > 0 ? std::min(c, m->x_chunk_max) : c;
}

// the workspaces and aux streams of the parts 1 .. np-1 of a split batch
static int reserve_parts(tik_model* m, int np, int N, int T) {
    int rc;
    if (!m->ev_fork) HIP_TRY(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    for (int k = 1; k < np; ++k) {
        if ((rc = model_reserve_ws(m, m->ws[k], N, T))) return rc;
        if (!m->aux[k - 1]) {
            HIP_TRY(hipStreamCreateWithFlags(&m->aux[k - 1], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&m->ev_join[k - 1], hipEventDisableTiming));
        }
    }
    return TIK_OK;
}

// The backbone over a batch, then tail(features, first window, windows, T', stream, workspace)
// on each sub-batch. The bf16x3 path runs in sub-batches of x_chunk windows, the large ones
// (allow_split) as parts on several streams.
template <class Tail>
static int forward_batches(tik_model* m, const float* x, int N, int T, hipStream_t st, Workspace& ws, bool allow_split,
                           Tail tail) {
    int rc;
    if (!m->use_x()) {
        float* f;
        int to;
        if ((rc = model_reserve_ws(m, ws, N, T)) || (rc = backbone(m, x, N, T, &f, &to, st, ws))) return rc;
        return tail(f, 0, N, to, st, ws);
    }
    const int chunk = std::min(N, x_chunk(m, T));
    if ((rc = model_reserve_ws(m, ws, chunk, T))) return rc;
    // large batches: np parts on np streams (the caller's + handle-owned
    // ones, fork/join by events), so one part's HBM-bound graph launches
    // run beside another part's MFMA-bound temporal convs (not while
    // profiling: per-launch events would time overlapping kernels)
    const bool split = allow_split && m->split && !m->profiling && (long long)chunk * T >= 32768 && N >= 2;
    const int np = split ? std::min((int)tik_model::MAXSPLIT, chunk) : 1;
    if (split && (rc = reserve_parts(m, np, (chunk + np - 1) / np, T))) return rc;
    auto part = [&](int n0, int n, hipStream_t s, const Workspace& w) -> int {
        float* f;
        int to;
        if (const int r = backbone_x(m, x + (size_t)n0 * T * m->V * m->C0, n, T, &f, &to, s, w)) return r;
        return tail(f, n0, n, to, s, w);
    };
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int n = std::min(chunk, N - n0);
        if (!(split && n >= np && (long long)n * T >= 32768)) {
            if ((rc = part(n0, n, st, ws))) return rc;
            continue;
        }
        HIP_TRY(hipEventRecord(m->ev_fork, st));
        for (int k = 1; k < np; ++k) HIP_TRY(hipStreamWaitEvent(m->aux[k - 1], m->ev_fork, 0));
        for (int k = 0; k < np; ++k) {
            const int a0 = (int)((long long)n * k / np), a1 = (int)((long long)n * (k + 1) / np);
            if ((rc = part(n0 + a0, a1 - a0, k == 0 ? st : m->aux[k - 1], k == 0 ? ws : m->ws[k]))) return rc;
        }
        for (int k = 1; k < np; ++k) {
            HIP_TRY(hipEventRecord(m->ev_join[k - 1], m->aux[k - 1]));
            HIP_TRY(hipStreamWaitEvent(st, m->ev_join[k - 1], 0));
        }
    }
    return TIK_OK;
}

int model_forward_ws(tik_model* m, const float* x, int N, int T, float* poses, hipStream_t st, Workspace& ws,
                     bool allow_split) {
    return forward_batches(m, x, N, T, st, ws, allow_split,
                           [&](const float* f, int n0, int n, int to, hipStream_t s, const Workspace& w) -> int {
        float* ps = poses + (size_t)n0 * to * m->pose_dim;
        return m->use_x() ? head_x(m, f, n * to, ps, w, s) : head_splitk(m, f, n * to, ps, w.hid.p, w.part.p, s);
    });
}
}  // namespace tik_host

extern "C" {

int tik_backbone_forward(tik_model_t m, const float* x, int N, int T, float* feat, void* stream) {
    if (!m || !x || !feat || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "tik_backbone_forward: bad arguments");
    ProfGuard pg(m);
    return forward_batches(m, x, N, T, (hipStream_t)stream, m->ws[0], false,
                           [&](const float* f, int n0, int n, int to, hipStream_t s, const Workspace&) -> int {
        HIP_TRY(hipMemcpyAsync(feat + (size_t)n0 * to * m->feat, f, sizeof(float) * (size_t)n * to * m->feat,
                               hipMemcpyDeviceToDevice, s));
        return TIK_OK;
    });
}

int tik_ik_forward(tik_model_t m, const float* x, int N, int T, float* poses, void* stream) {
    if (!m || !x || !poses || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "tik_ik_forward: bad arguments");
    if (m->pose_dim <= 0) return fail(TIK_E_INVALID, "tik_ik_forward: backbone-only handle (no pose_regressor weights)");
    ProfGuard pg(m);
    return model_forward_ws(m, x, N, T, poses, (hipStream_t)stream, m->ws[0], true);
}

int tik_stgcn_block_fwd(tik_block_t b, const float* x, int N, int T, float* out, void* stream) {
    if (!b || !x || !out || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "tik_stgcn_block_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const Layer& L = b->layer;
    const size_t rows = (size_t)N * T * L.V;
    int rc;
    const float* xin = x;
    if (L.cin != L.cinp) {
        if ((rc = b->xp.reserve(rows * L.cinp))) return rc;
        HIP_TRY(tik::launch_pad_channels(x, (long long)rows, L.cin, L.cinp, b->xp.p, st));
        xin = b->xp.p;
    }
    if ((rc = b->z.reserve(rows * L.cout))) return rc;
    return L.forward(xin, L.cinp, N, T, b->z.p, out, st, b->prec);
}

}  // extern "C"
