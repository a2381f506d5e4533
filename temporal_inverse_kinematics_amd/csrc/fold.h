// fold.h — the host side of a state dict, with no HIP call in it: the view of
// a tik_tensor array, its validation, and the fold algebra of the IK forward.
//
//   z   = ReLU( mix_A( x . wg^T ) + bias2[w][c] )                  gcn + tcn.0 BN
//   out = ReLU( sum_tap z[s t'+tap-1] . wt_tap^T + res + biasT )   tcn.2 + tcn.3 BN + residual
//
// BatchNorm (eval), the gcn bias times colsum(A) and the residual conv's BN
// are folded into wg / bias2 / wt / biasT / wr. Everything here runs before the
// first device allocation (model.cpp), and stands alone in tests/test_fold_host.py.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/tik.h"

namespace tik {
bool fits_coco_hop2(const float* A, int V);   // cgemm.h
}

namespace tik_host {

inline thread_local std::string g_err;   // tik_last_error()

inline int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

constexpr float BN_EPS = 1e-5f;
constexpr int TK = 3;   // temporal kernel (pose_trainer.py:85)

struct HostTensor {
    std::vector<float> v;         // empty when the tensor's data was null
    std::vector<int64_t> shape;
};

using TensorMap = std::map<std::string, HostTensor>;

// The tensors come from outside the program (include/tik.h is a C ABI):
// tik_tensor::shape has 4 entries, and an extent is never negative.
inline int to_map(const tik_tensor* t, int n, TensorMap& m) {
    for (int i = 0; i < n; ++i) {
        if (!t[i].name) continue;
        if (t[i].ndim < 0 || t[i].ndim > 4) return fail(TIK_E_INVALID, "'%s': ndim %d outside 0..4", t[i].name, t[i].ndim);
        HostTensor h;
        int64_t numel = 1;
        for (int d = 0; d < t[i].ndim; ++d) {
            if (t[i].shape[d] < 0) return fail(TIK_E_INVALID, "'%s': negative extent %lld", t[i].name, (long long)t[i].shape[d]);
            h.shape.push_back(t[i].shape[d]);
            numel *= t[i].shape[d];
        }
        if (t[i].data) h.v.assign(t[i].data, t[i].data + numel);
        m[t[i].name] = std::move(h);
    }
    return TIK_OK;
}

inline const HostTensor* find(const TensorMap& m, const std::string& k) {
    auto it = m.find(k);
    return it == m.end() ? nullptr : &it->second;
}

// a named tensor's rank and the values it really holds, before any shape[i] or v[i] is read
inline int expect(const HostTensor& t, const std::string& name, size_t min_rank, size_t min_values) {
    if (t.shape.size() < min_rank)
        return fail(TIK_E_INVALID, "'%s' has %zu dimensions, at least %zu expected", name.c_str(), t.shape.size(), min_rank);
    if (t.v.size() < min_values)
        return fail(TIK_E_INVALID, "'%s' holds %zu values, at least %zu expected", name.c_str(), t.v.size(), min_values);
    return TIK_OK;
}

// eval BatchNorm -> (scale, shift)
inline int bn_fold(const TensorMap& m, const std::string& pre, int C, std::vector<float>& sc, std::vector<float>& sh) {
    const HostTensor* g = find(m, pre + ".weight");
    const HostTensor* b = find(m, pre + ".bias");
    const HostTensor* mu = find(m, pre + ".running_mean");
    const HostTensor* var = find(m, pre + ".running_var");
    if (!g || !b || !mu || !var) return fail(TIK_E_MISSING, "missing BatchNorm tensors under '%s'", pre.c_str());
    if ((int)g->v.size() != C || (int)b->v.size() != C || (int)mu->v.size() != C || (int)var->v.size() != C)
        return fail(TIK_E_INVALID, "BatchNorm '%s' expects %d channels", pre.c_str(), C);
    sc.resize(C);
    sh.resize(C);
    for (int c = 0; c < C; ++c) {
        const double s = (double)g->v[c] / std::sqrt((double)var->v[c] + (double)BN_EPS);
        sc[c] = (float)s;
        sh[c] = (float)((double)b->v[c] - (double)mu->v[c] * s);
    }
    return TIK_OK;
}

enum ResKind { RES_ZERO = 0, RES_IDEN = 1, RES_CONV = 2 };

inline int round4(int c) { return (c + 3) & ~3; }

// One StGcnBlock with its BatchNorms folded into fp32 weights.
struct FoldedBlock {
    int cin = 0, cinp = 0, cout = 0, stride = 1, res = RES_IDEN, V = 17;
    bool mix_sparse = false;      // every nonzero of A_eff inside the COCO hop <= 2 pattern
    std::vector<float> wg;        // [cout][cinp]      gcn conv scaled by tcn.0 BN
    std::vector<float> bias2;     // [V][cout]         sc1*bg*colsum(A)[w] + sh1
    std::vector<float> amix;      // [V][V]            A_eff[v][w]
    std::vector<float> wt;        // [cout][3*cout]    tcn conv scaled by tcn.3 BN, k = tap*cout + ci
    std::vector<float> biasT;     // [cout]            tcn bias (+ residual bias) folded
    std::vector<float> wr;        // [cout][cinp]      residual conv scaled by residual.1 BN (RES_CONV)
    std::vector<float> wr0;       // [cout][cin]       the same unpadded, for a raw-input first layer (cin <= 4)
};

inline int fold_block(const TensorMap& m, const std::string& pre, int cin, int cout, int stride, int residual,
                      const std::vector<float>& A_eff, int V, FoldedBlock& f) {
    f.cin = cin; f.cout = cout; f.stride = stride; f.V = V;
    f.cinp = round4(cin);
    const int cinp = f.cinp;
    if (cout % 4 != 0) return fail(TIK_E_INVALID, "out_channels must be a multiple of 4 (got %d)", cout);
    f.res = !residual ? RES_ZERO : ((cin == cout && stride == 1) ? RES_IDEN : RES_CONV);
    const HostTensor* Wg = find(m, pre + "gcn.conv.weight");
    const HostTensor* bg = find(m, pre + "gcn.conv.bias");
    if (!Wg) return fail(TIK_E_MISSING, "missing '%sgcn.conv.weight'", pre.c_str());
    if ((int64_t)Wg->v.size() != (int64_t)cout * cin)
        return fail(TIK_E_INVALID, "'%sgcn.conv.weight' must be (%d,%d,1,1) (spatial kernel K=1 only)", pre.c_str(), cout, cin);
    std::vector<float> sc1, sh1, sc2, sh2;
    int rc;
    if ((rc = bn_fold(m, pre + "tcn.0", cout, sc1, sh1))) return rc;
    if ((rc = bn_fold(m, pre + "tcn.3", cout, sc2, sh2))) return rc;
    if (bg && (rc = expect(*bg, pre + "gcn.conv.bias", 0, cout))) return rc;
    std::vector<double> colsum(V, 0.0);
    for (int v = 0; v < V; ++v)
        for (int w = 0; w < V; ++w) colsum[w] += A_eff[v * V + w];
    f.wg.assign((size_t)cout * cinp, 0.f);
    f.bias2.resize((size_t)V * cout);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) f.wg[(size_t)co * cinp + ci] = sc1[co] * Wg->v[(size_t)co * cin + ci];
    for (int w = 0; w < V; ++w)
        for (int co = 0; co < cout; ++co) {
            const double b = bg ? bg->v[co] : 0.0;
            f.bias2[(size_t)w * cout + co] = (float)((double)sc1[co] * b * colsum[w] + sh1[co]);
        }
    const HostTensor* Wt = find(m, pre + "tcn.2.weight");
    const HostTensor* bt = find(m, pre + "tcn.2.bias");
    if (!Wt) return fail(TIK_E_MISSING, "missing '%stcn.2.weight'", pre.c_str());
    if ((int64_t)Wt->v.size() != (int64_t)cout * cout * TK)
        return fail(TIK_E_INVALID, "'%stcn.2.weight' must be (%d,%d,3,1)", pre.c_str(), cout, cout);
    if (bt && (rc = expect(*bt, pre + "tcn.2.bias", 0, cout))) return rc;
    f.wt.resize((size_t)cout * TK * cout);
    f.biasT.resize(cout);
    for (int co = 0; co < cout; ++co) {
        for (int tap = 0; tap < TK; ++tap)
            for (int ci = 0; ci < cout; ++ci)
                f.wt[(size_t)co * TK * cout + tap * cout + ci] = sc2[co] * Wt->v[((size_t)co * cout + ci) * TK + tap];
        f.biasT[co] = (float)((double)sc2[co] * (bt ? bt->v[co] : 0.0) + sh2[co]);
    }
    f.wr.clear();
    f.wr0.clear();
    if (f.res == RES_CONV) {
        const HostTensor* Wr = find(m, pre + "residual.0.weight");
        const HostTensor* br = find(m, pre + "residual.0.bias");
        if (!Wr) return fail(TIK_E_MISSING, "missing '%sresidual.0.weight'", pre.c_str());
        if ((int64_t)Wr->v.size() != (int64_t)cout * cin)
            return fail(TIK_E_INVALID, "'%sresidual.0.weight' must be (%d,%d,1,1)", pre.c_str(), cout, cin);
        std::vector<float> scr, shr;
        if ((rc = bn_fold(m, pre + "residual.1", cout, scr, shr))) return rc;
        if (br && (rc = expect(*br, pre + "residual.0.bias", 0, cout))) return rc;
        f.wr.assign((size_t)cout * cinp, 0.f);
        for (int co = 0; co < cout; ++co) {
            for (int ci = 0; ci < cin; ++ci) f.wr[(size_t)co * cinp + ci] = scr[co] * Wr->v[(size_t)co * cin + ci];
            f.biasT[co] += (float)((double)scr[co] * (br ? br->v[co] : 0.0) + shr[co]);
        }
        if (cin <= 4) {
            f.wr0.resize((size_t)cout * cin);
            for (int co = 0; co < cout; ++co)
                for (int ci = 0; ci < cin; ++ci) f.wr0[(size_t)co * cin + ci] = f.wr[(size_t)co * cinp + ci];
        }
    }
    f.amix.assign(A_eff.begin(), A_eff.end());
    f.mix_sparse = tik::fits_coco_hop2(f.amix.data(), V);
    return TIK_OK;
}

// data_bn over V*C0 channels; C0 (<= 4) is read off its size
inline int fold_data_bn(const TensorMap& m, int V, int& C0, std::vector<float>& sc, std::vector<float>& sh) {
    const HostTensor* g = find(m, "backbone.data_bn.weight");
    if (!g) return fail(TIK_E_MISSING, "missing 'backbone.data_bn.weight'");
    C0 = (int)g->v.size() / V;
    if (C0 * V != (int)g->v.size() || C0 > 4) return fail(TIK_E_INVALID, "data_bn size %zu not V*C (C<=4)", g->v.size());
    return bn_fold(m, "backbone.data_bn", V * C0, sc, sh);
}

// A PoseRegressor state dict on the host: graph, data_bn, the blocks and the
// head (hidden = 0: a backbone-only StgGcn18 state dict, st_gcn_aaai18.py:32-133).
struct FoldedModel {
    int V = 17, C0 = 3, feat = 0, hidden = 0, pose_dim = 0;
    std::vector<float> bn_sc, bn_sh;   // data_bn (V*C0)
    std::vector<FoldedBlock> blocks;
    const HostTensor *W0 = nullptr, *B0 = nullptr, *W3 = nullptr, *B3 = nullptr;   // head, in the caller's map
};

inline int fold_backbone(const TensorMap& m, FoldedModel& f) {
    const HostTensor* A = find(m, "backbone.A");
    if (!A) return fail(TIK_E_MISSING, "missing 'backbone.A'");
    if (A->shape.size() != 3 || A->shape[1] != A->shape[2])
        return fail(TIK_E_INVALID, "'backbone.A' must be (K,V,V)");
    if (A->shape[0] != 1) return fail(TIK_E_INVALID, "only the 'uniform' graph strategy (K=1) is supported by the fused path");
    if (A->shape[1] != 17) return fail(TIK_E_INVALID, "fused path is built for V=17 (coco), got %d", (int)A->shape[1]);
    const int V = f.V = 17;
    int rc;
    if ((rc = expect(*A, "backbone.A", 3, (size_t)V * V))) return rc;
    if ((rc = fold_data_bn(m, V, f.C0, f.bn_sc, f.bn_sh))) return rc;
    const HostTensor* strides = find(m, "tik.strides");
    int cin = f.C0;
    for (int l = 0;; ++l) {
        const std::string pre = "backbone.st_gcn_networks." + std::to_string(l) + ".";
        const HostTensor* Wg = find(m, pre + "gcn.conv.weight");
        if (!Wg) break;
        if ((rc = expect(*Wg, pre + "gcn.conv.weight", 2, 0))) return rc;
        const int cout = (int)Wg->shape[0];
        if ((int)Wg->shape[1] != cin) return fail(TIK_E_INVALID, "layer %d: in_channels %d != previous out %d", l, (int)Wg->shape[1], cin);
        // Temporal strides are architecture, not weights: the IK config of
        // pose_trainer.py:76-83 unless the caller passes a "tik.strides" tensor.
        static const int ik_strides[8] = {1, 1, 2, 1, 1, 2, 2, 2};
        int stride = l < 8 ? ik_strides[l] : 1;
        if (strides) {
            if (l >= (int)strides->v.size()) return fail(TIK_E_INVALID, "'tik.strides' has no entry for layer %d", l);
            stride = (int)strides->v[l];
        }
        const HostTensor* Wr = find(m, pre + "residual.0.weight");
        if ((Wr != nullptr) != (cin != cout || stride != 1))
            return fail(TIK_E_INVALID, "layer %d: residual conv presence does not match (cin=%d, cout=%d, stride=%d)", l, cin, cout, stride);
        const std::string iname = "backbone.edge_importance." + std::to_string(l);
        const HostTensor* imp = find(m, iname);
        if (imp && (rc = expect(*imp, iname, 0, (size_t)V * V))) return rc;
        std::vector<float> Ae(V * V);
        for (int i = 0; i < V * V; ++i) Ae[i] = A->v[i] * (imp ? imp->v[i] : 1.0f);
        f.blocks.emplace_back();
        if ((rc = fold_block(m, pre, cin, cout, stride, 1, Ae, V, f.blocks.back()))) return rc;
        cin = cout;
    }
    if (f.blocks.empty()) return fail(TIK_E_MISSING, "no 'backbone.st_gcn_networks.*' layers");
    f.feat = V * cin;
    return TIK_OK;
}

// the head's two Linear layers: all four tensors, or none (backbone-only)
inline int fold_head(const TensorMap& m, FoldedModel& f) {
    f.W0 = find(m, "pose_regressor.0.weight");
    f.B0 = find(m, "pose_regressor.0.bias");
    f.W3 = find(m, "pose_regressor.3.weight");
    f.B3 = find(m, "pose_regressor.3.bias");
    if (!f.W0 && !f.B0 && !f.W3 && !f.B3) return TIK_OK;
    if (!f.W0 || !f.B0 || !f.W3 || !f.B3) return fail(TIK_E_MISSING, "missing pose_regressor.{0,3}.{weight,bias}");
    int rc;
    if ((rc = expect(*f.W0, "pose_regressor.0.weight", 2, 0)) || (rc = expect(*f.W3, "pose_regressor.3.weight", 2, 0))) return rc;
    f.hidden = (int)f.W0->shape[0];
    f.pose_dim = (int)f.W3->shape[0];
    if ((int)f.W0->shape[1] != f.feat || (int)f.W3->shape[1] != f.hidden) return fail(TIK_E_INVALID, "head shapes do not match backbone features %d", f.feat);
    if (f.hidden % 4) return fail(TIK_E_INVALID, "hidden size must be a multiple of 4");
    if ((rc = expect(*f.W0, "pose_regressor.0.weight", 2, (size_t)f.hidden * f.feat)) || (rc = expect(*f.B0, "pose_regressor.0.bias", 0, f.hidden)) ||
        (rc = expect(*f.W3, "pose_regressor.3.weight", 2, (size_t)f.pose_dim * f.hidden)) || (rc = expect(*f.B3, "pose_regressor.3.bias", 0, f.pose_dim)))
        return rc;
    return TIK_OK;
}

}  // namespace tik_host
