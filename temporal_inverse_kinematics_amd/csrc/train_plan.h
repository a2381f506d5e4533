// train_plan.h — the host side of a trainer's state dict, with no HIP call in it:
// validation of the tensors tik_trainer_create is given, the flat parameter /
// buffer layout, the per-layer descriptors, and the sizes that follow from a
// batch shape (N windows of T frames).
//
//   P  flat fp32 parameters in the reference's tensor layouts (grad, Adam state alike)
//   B  flat fp32 buffers: BatchNorm running statistics and the adjacency A
//
// Entries are registered in a fixed order (tik_trainer_tensor(i) shows it):
// the four data_bn tensors, A, per layer the block's tensors (with the
// residual conv's six where the block has one), edge_importance.*, the head.
//
// Every tensor is checked by name for rank and for the exact number of values
// it holds before any shape[i] or v[i] of it is read (include/tik.h is a C ABI:
// the tensors come from outside the program): the kernels read `cout` values at
// a recorded offset, so a short tensor would have them read its neighbour.
// Everything here runs before the first device allocation (train_model.cpp),
// and stands alone in tests/test_train_plan_host.py.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <initializer_list>

#include "fold.h"

namespace tik_train {

using namespace tik_host;

constexpr int V = 17;
constexpr int HIDDEN = 512;

struct PlanEntry {       // one exported state-dict tensor
    std::string name;
    std::vector<int64_t> shape;
    long long off = 0, numel = 0;
    int kind = 0;        // 0 parameter (flat P / grad / Adam state), 1 buffer (flat B)
};

struct PlanLayer {
    int cin = 0, cinp = 0, cout = 0, stride = 1, res = RES_IDEN;
    // parameter offsets (flat P) and buffer offsets (flat B); -1: the block has no residual conv
    long long wg = -1, bg = -1, g1 = -1, b1 = -1, wt = -1, bt = -1, g2 = -1, b2 = -1, wr = -1, br = -1, g3 = -1,
              b3 = -1, E = -1;
    long long rm1 = -1, rv1 = -1, rm2 = -1, rv2 = -1, rm3 = -1, rv3 = -1;
};

struct TrainPlan {
    std::vector<PlanEntry> ents;
    std::vector<float> hp, hb;                                    // flat P and B on the host
    std::vector<PlanLayer> L;
    long long dg = -1, db = -1, rm0 = -1, rv0 = -1, A = -1;       // data_bn + adjacency
    long long w1 = -1, b1 = -1, w2 = -1, b2 = -1;                 // head
    int feat = 0, pose_dim = 0;
    int ldp = 0;                                                  // pose_dim rounded to 4
    int maxc = 4;                                                 // widest activation row (batch_fits_32bit)
    int kmax = 4 * V;                                             // widest BatchNorm (the k[3][C] scratch)
    std::vector<int> cmap0;                                       // data_bn: padded column 4v+c -> channel 3v+c, -1 padding
};

// One tensor to register: suffix under the group's prefix, kind, the exact
// number of values, and where its offset goes.
struct Want {
    const char* suffix;
    int kind;
    long long count;
    long long* off;
};

inline const HostTensor* need(const TensorMap& m, const std::string& name, int& rc) {
    const HostTensor* h = find(m, name);
    if (!h) rc = fail(TIK_E_MISSING, "tik_trainer_create: missing tensor '%s'", name.c_str());
    return h;
}

inline int take(const TensorMap& m, const std::string& pre, std::initializer_list<Want> wants, TrainPlan& p) {
    for (const Want& w : wants) {
        const std::string name = pre + w.suffix;
        int rc = TIK_OK;
        const HostTensor* h = need(m, name, rc);
        if (!h) return rc;
        if ((long long)h->v.size() != w.count)
            return fail(TIK_E_INVALID, "tik_trainer_create: '%s' holds %zu values%s, exactly %lld expected", name.c_str(),
                        h->v.size(), h->v.empty() ? " (null data?)" : "", w.count);
        std::vector<float>& dst = w.kind == 0 ? p.hp : p.hb;
        PlanEntry e;
        e.name = name;
        e.shape = h->shape;
        e.numel = w.count;
        e.kind = w.kind;
        e.off = *w.off = (long long)dst.size();
        dst.insert(dst.end(), h->v.begin(), h->v.end());
        p.ents.push_back(std::move(e));
    }
    return TIK_OK;
}

inline int plan_trainer(const TensorMap& m, TrainPlan& p) {
    int rc = TIK_OK;
    const HostTensor* strides = find(m, "tik.strides");
    if (!strides) return fail(TIK_E_MISSING, "tik_trainer_create: missing 'tik.strides'");
    if (strides->v.empty()) return fail(TIK_E_INVALID, "tik_trainer_create: 'tik.strides' is empty: one temporal stride per layer");
    for (const float s : strides->v)
        if (!(s >= 1.f && s < 2147483648.f) || s != std::floor(s))
            return fail(TIK_E_INVALID, "tik_trainer_create: 'tik.strides' entry %g is not a positive whole number", (double)s);
    const std::string bb = "backbone.";
    if ((rc = take(m, bb, {{"data_bn.weight", 0, 3 * V, &p.dg}, {"data_bn.bias", 0, 3 * V, &p.db},
                           {"data_bn.running_mean", 1, 3 * V, &p.rm0}, {"data_bn.running_var", 1, 3 * V, &p.rv0},
                           {"A", 1, V * V, &p.A}}, p)))
        return rc;
    const int nl = (int)strides->v.size();
    int cin = 3;
    for (int i = 0; i < nl; ++i) {
        const std::string pre = bb + "st_gcn_networks." + std::to_string(i) + ".";
        const HostTensor* wg = need(m, pre + "gcn.conv.weight", rc);
        if (!wg || (rc = expect(*wg, pre + "gcn.conv.weight", 2, 0))) return rc;
        PlanLayer l;
        l.cin = cin;
        l.cinp = round4(cin);
        l.stride = (int)strides->v[i];
        if (wg->shape[1] != cin || wg->shape[0] < 4 || wg->shape[0] % 4 || wg->shape[0] > 256)
            return fail(TIK_E_INVALID, "tik_trainer_create: layer %d: '%sgcn.conv.weight' (%lld,%lld) vs %d input channels"
                        " (output channels: a multiple of 4, at most 256)", i, pre.c_str(), (long long)wg->shape[0],
                        (long long)wg->shape[1], cin);
        const int co = l.cout = (int)wg->shape[0];
        l.res = find(m, pre + "residual.0.weight") ? RES_CONV : RES_IDEN;
        if (l.res == RES_IDEN && (cin != co || l.stride != 1))
            return fail(TIK_E_INVALID, "tik_trainer_create: layer %d: identity residual needs cin == cout, stride 1", i);
        if ((rc = take(m, pre, {{"gcn.conv.weight", 0, (long long)co * cin, &l.wg}, {"gcn.conv.bias", 0, co, &l.bg},
                                {"tcn.0.weight", 0, co, &l.g1}, {"tcn.0.bias", 0, co, &l.b1},
                                {"tcn.0.running_mean", 1, co, &l.rm1}, {"tcn.0.running_var", 1, co, &l.rv1},
                                {"tcn.2.weight", 0, 3LL * co * co, &l.wt}, {"tcn.2.bias", 0, co, &l.bt},
                                {"tcn.3.weight", 0, co, &l.g2}, {"tcn.3.bias", 0, co, &l.b2},
                                {"tcn.3.running_mean", 1, co, &l.rm2}, {"tcn.3.running_var", 1, co, &l.rv2}}, p)))
            return rc;
        if (l.res == RES_CONV &&
            (rc = take(m, pre, {{"residual.0.weight", 0, (long long)co * cin, &l.wr}, {"residual.0.bias", 0, co, &l.br},
                                {"residual.1.weight", 0, co, &l.g3}, {"residual.1.bias", 0, co, &l.b3},
                                {"residual.1.running_mean", 1, co, &l.rm3}, {"residual.1.running_var", 1, co, &l.rv3}}, p)))
            return rc;
        p.maxc = std::max(p.maxc, std::max(l.cinp, co));
        p.kmax = std::max(p.kmax, co);
        cin = co;
        p.L.push_back(l);
    }
    for (int i = 0; i < nl; ++i) {
        const std::string imp = "edge_importance." + std::to_string(i);
        if ((rc = take(m, bb, {{imp.c_str(), 0, V * V, &p.L[i].E}}, p))) return rc;
    }
    // the head: Linear(feat, 512) -> LeakyReLU -> Dropout -> Linear(512, pose_dim)
    const char *n1 = "pose_regressor.0.weight", *n2 = "pose_regressor.3.weight";
    const HostTensor* W1 = need(m, n1, rc);
    if (!W1 || (rc = expect(*W1, n1, 2, 0))) return rc;
    const HostTensor* W2 = need(m, n2, rc);
    if (!W2 || (rc = expect(*W2, n2, 2, 0))) return rc;
    p.feat = V * cin;
    if (W1->shape[0] != HIDDEN || W1->shape[1] != p.feat || W2->shape[1] != HIDDEN || W2->shape[0] < 1 ||
        W2->shape[0] > INT_MAX / HIDDEN)
        return fail(TIK_E_INVALID, "tik_trainer_create: head shapes '%s' (%lld,%lld), '%s' (%lld,%lld) vs feature %d, hidden %d",
                    n1, (long long)W1->shape[0], (long long)W1->shape[1], n2, (long long)W2->shape[0],
                    (long long)W2->shape[1], p.feat, HIDDEN);
    p.pose_dim = (int)W2->shape[0];
    p.ldp = round4(p.pose_dim);
    if ((rc = take(m, "pose_regressor.", {{"0.weight", 0, (long long)HIDDEN * p.feat, &p.w1}, {"0.bias", 0, HIDDEN, &p.b1},
                                          {"3.weight", 0, (long long)p.pose_dim * HIDDEN, &p.w2},
                                          {"3.bias", 0, p.pose_dim, &p.b2}}, p)))
        return rc;
    p.cmap0.resize(4 * V);
    for (int c = 0; c < 4 * V; ++c) p.cmap0[c] = (c % 4 < 3) ? (c / 4) * 3 + c % 4 : -1;
    return TIK_OK;
}

// ---- what follows from a batch shape: N windows of T frames
struct Frames {
    int tin = 0, tout = 0;
};

// The frame chain t -> (t-1)/stride + 1 through the temporal convs: layer i's
// input and output length into fr[i] (fr may be null), the head's length returned.
inline int frame_chain(const TrainPlan& p, int T, Frames* fr) {
    for (size_t i = 0; i < p.L.size(); ++i) {
        const int tout = (T - 1) / p.L[i].stride + 1;
        if (fr) fr[i] = Frames{T, tout};
        T = tout;
    }
    return T;
}

// every float4 launcher indexes rows x channels / 4 in 32 bits: the widest activation of the batch
inline bool batch_fits_32bit(const TrainPlan& p, int N, int T) {
    const long long lim = (1LL << 31) - 1;
    return (long long)N * T * V * p.maxc / 4 <= lim && (long long)N * T * V * 4 <= lim;
}

struct StepSizes {            // element counts of the step's workspace
    long long p0 = 0;         // input positions N*T*V (x4, x0: 4 floats each)
    long long rows_h = 0;     // head rows N*T' (Ph, Dh, dD, mask: HIDDEN floats each; Oh, dOh: ldp)
    long long big = 0;        // the widest activation (gA, gB, the t* scratch, up)
    long long colsz = 0;      // the largest explicit im2col
    long long partf_cap = 0, partd_cap = 0;   // split-row partial sums: fp32 (wgrad, split-K), double (colstats)
};

inline StepSizes step_sizes(const TrainPlan& p, const Frames* fr, int N, int T) {
    StepSizes s;
    for (size_t i = 0; i < p.L.size(); ++i) {
        const PlanLayer& l = p.L[i];
        const long long pin = (long long)N * fr[i].tin * V, pout = (long long)N * fr[i].tout * V;
        s.big = std::max(s.big, pin * std::max(l.cout, l.cinp));
        s.colsz = std::max(s.colsz, std::max(pout * 3LL * l.cout, pout * (long long)l.cinp));
    }
    s.rows_h = (long long)N * fr[p.L.size() - 1].tout;
    s.p0 = (long long)N * T * V;
    s.partf_cap = std::max<long long>(8LL << 20, 64LL * s.rows_h * HIDDEN);
    s.partd_cap = 2LL * 1024 * 1024;
    return s;
}

struct EvalSizes {            // element counts of the eval pass's workspace
    long long p0 = 0, rows = 0;
    long long zsz = 0;        // a block's graph-mix output
    long long asz = 0;        // the activation ping-pong
};

inline EvalSizes eval_sizes(const TrainPlan& p, const Frames* fr, int N, int T) {
    EvalSizes s;
    for (size_t i = 0; i < p.L.size(); ++i) {
        s.zsz = std::max(s.zsz, (long long)N * fr[i].tin * V * p.L[i].cout);
        s.asz = std::max(s.asz, (long long)N * fr[i].tout * V * p.L[i].cout);
    }
    s.rows = (long long)N * fr[p.L.size() - 1].tout;
    s.p0 = (long long)N * T * V;
    return s;
}

}  // namespace tik_train
