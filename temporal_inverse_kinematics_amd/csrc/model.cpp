// model.cpp — building the IK handles: the state dict is validated and folded
// on the host (fold.h), then packed for each kernel family and uploaded; the
// handle-owned workspaces and what the online-IK stream needs from a model.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "model.h"
#include "stream.h"

using namespace tik_host;

namespace tik_host {

int Layer::pack(const FoldedBlock& f) {
    cin = f.cin; cinp = f.cinp; cout = f.cout; stride = f.stride; res = f.res; V = f.V; mix_sparse = f.mix_sparse;
    int rc;
    // cgemm.hip: fp32 rows and their bf16 planes (also read by layer0.hip, xblock.hip's block 0
    // and, copied back, by the online-IK stream)
    if ((rc = wg.upload(f.wg)) || (rc = bias2.upload(f.bias2)) || (rc = amix.upload(f.amix)) || (rc = wt.upload(f.wt)) ||
        (rc = biasT.upload(f.biasT)) || (rc = s3g.build(f.wg, cout, 1, cinp, cinp)) ||
        (rc = s3t.build(f.wt, cout, TK, cout, TK * cout)))
        return rc;
    if (res == RES_CONV && ((rc = wr.upload(f.wr)) || (rc = s3r.build(f.wr, cout, 1, cinp, cinp)))) return rc;
    // layer0.hip / xblock.hip: the unpadded residual conv of a raw-input first layer
    if ((rc = wr0.upload(f.wr0))) return rc;
    // xgemm.hip: bf16x3 tiles
    const int bn = cout >= 128 ? 128 : 64;
    if (cin % 32 == 0) {
        const tik::XPackSeg g{f.wg.data(), cinp, 1, cin};
        if ((rc = xg.upload(tik::xgemm_pack(&g, 1, cout, bn)))) return rc;
        xg_bn = bn;
    }
    if (cout % 32 == 0) {
        tik::XPackSeg t[2] = {{f.wt.data(), TK * cout, TK, cout}, {f.wr.data(), cinp, 1, cin}};
        const int ns = (res == RES_CONV && cin % 32 == 0) ? 2 : 1;
        if ((rc = xt.upload(tik::xgemm_pack(t, ns, cout, bn)))) return rc;
        xt_bn = bn; xt_ks = TK * cout / 32 + (ns == 2 ? cin / 32 : 0);
    }
    // xtws.hip
    if (cout == 128 && cin == 128 && stride == 1 && res == RES_IDEN)
        if ((rc = xtw.upload(tik::xblock_pack_weights(f.wt.data(), cout, TK * cout, TK, cout)))) return rc;
    // xgraph.hip
    if ((cout == 128 || cout == 256) && (cin == 64 || cin == 128 || cin == 256))
        if ((rc = xgw.upload(tik::xblock_pack_weights(f.wg.data(), cout, cinp, 1, cin)))) return rc;
    // xblock.hip
    if (cout == 64 && stride == 1) {
        if ((rc = xbt.upload(tik::xblock_pack_weights(f.wt.data(), cout, TK * cout, TK, cout)))) return rc;
        if (cin == 64 && (rc = xbg.upload(tik::xblock_pack_weights(f.wg.data(), cout, cinp, 1, cin)))) return rc;
    }
    return TIK_OK;
}

// Handle settings read from the environment (each selects a test-pinned
// alternative of the default path) and the device facts the launches need.
static void apply_env(tik_model* md) {
    if (const char* e = getenv("TIK_X_CHUNK")) md->x_chunk_max = atoi(e);
    if (const char* e = getenv("TIK_XBLK")) md->xblk = e[0] != '0';
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
        md->ncu = ncu;
    for (auto& L : md->layers) {
        if (const char* w = getenv("TIK_XGW")) L.xgwon = (atoi(w) >> L.index) & 1;
        if (const char* w = getenv("TIK_XTWS")) L.xtwson = (atoi(w) >> L.index) & 1;
        if (const char* w = getenv("TIK_XFG")) L.xfgon = (atoi(w) >> L.index) & 1;
        L.xtrash = reinterpret_cast<float*>(md->trash.p);
    }
    if (const char* e = getenv("TIK_SPLIT")) md->split = e[0] != '0';
}

int model_reserve_ws(tik_model* m, Workspace& w, int N, int T) {
    const size_t V = m->V;
    size_t zmax = 0, amax = 0;
    int t = T;
    for (const Layer& L : m->layers) {
        zmax = std::max(zmax, (size_t)N * t * V * L.cout);
        t = Layer::tout(t, L.stride);
        amax = std::max(amax, (size_t)N * t * V * L.cout);
    }
    if (m->use_xblk()) zmax = std::max(zmax, (size_t)N * T * V * XB0_P3_FLOATS);
    // the second z buffer: the next block's z made inside a fused xtws launch
    size_t z2max = 0;
    t = T;
    for (size_t l = 0; l + 1 < m->layers.size(); ++l) {
        const Layer& L = m->layers[l];
        t = Layer::tout(t, L.stride);
        if (L.index > 0 && L.stride == 1 && L.fuses_gcn_of(m->layers[l + 1])) z2max = std::max(z2max, (size_t)N * t * V * m->layers[l + 1].cout);
    }
    t = T;
    for (const Layer& L : m->layers) t = Layer::tout(t, L.stride);
    int rc;
    if (z2max && (rc = w.z2.reserve(z2max))) return rc;
    // split-K partials: ksplit * tiles <= 256 + 128 launches of <= 128x128 tiles
    // (cgemm), or up to 8 K slices of the xgemm head's hidden rows
    if ((rc = w.xb.reserve((size_t)N * T * V * 4)) || (rc = w.z.reserve(zmax)) ||
        (rc = w.a0.reserve(amax)) || (rc = w.a1.reserve(amax)) || (rc = w.hid.reserve((size_t)N * t * m->hidden)) ||
        (rc = w.part.reserve(std::max((size_t)384 * 128 * 128, (size_t)8 * N * t * m->hidden))))
        return rc;
    return TIK_OK;
}

void model_retain(tik_model* m) { m->refs.fetch_add(1); }
void model_release(tik_model* m) {
    if (m->refs.fetch_sub(1) == 1) delete m;
}

OnlineModelView model_online_view(const tik_model* m) {
    static_assert((int)tik::ONR_ZERO == RES_ZERO && (int)tik::ONR_IDEN == RES_IDEN && (int)tik::ONR_CONV == RES_CONV, "");
    OnlineModelView v;
    v.shape.V = m->V; v.shape.C0 = m->C0; v.shape.feat = m->feat; v.shape.hidden = m->hidden; v.shape.pose_dim = m->pose_dim;
    for (const Layer& L : m->layers) {
        v.shape.layers.push_back({L.cin, L.cinp, L.cout, L.stride, L.res});
        v.L.push_back({L.wg.p, L.bias2.p, L.amix.p, L.wt.p, L.wr.p, L.biasT.p});
    }
    v.bn_sc = m->bn_sc.p; v.bn_sh = m->bn_sh.p;
    v.w0 = m->w0.p; v.b0 = m->b0.p; v.w3 = m->w3.p; v.b3 = m->b3.p;
    v.ncu = m->ncu;
    return v;
}
}  // namespace tik_host

extern "C" {

int tik_model_create(const tik_tensor* tensors, int n_tensors, tik_model_t* out) try {
    if (!tensors || n_tensors <= 0 || !out) return fail(TIK_E_INVALID, "tik_model_create: null argument");
    *out = nullptr;
    // host: a refused state dict allocates nothing and never touches the GPU
    TensorMap m;
    FoldedModel f;
    int rc, prec;
    if ((rc = to_map(tensors, n_tensors, m)) || (rc = fold_backbone(m, f)) || (rc = precision_from_env(prec)) ||
        (rc = fold_head(m, f)))
        return rc;
    // device
    auto md = std::make_unique<tik_model>();
    md->V = f.V; md->C0 = f.C0; md->feat = f.feat; md->hidden = f.hidden; md->pose_dim = f.pose_dim; md->prec = prec;
    if ((rc = md->bn_sc.upload(f.bn_sc)) || (rc = md->bn_sh.upload(f.bn_sh))) return rc;
    md->layers.resize(f.blocks.size());
    for (size_t l = 0; l < f.blocks.size(); ++l) {
        md->layers[l].index = (int)l;
        if ((rc = md->layers[l].pack(f.blocks[l]))) return rc;
    }
    if (f.hidden) {   // else a backbone-only handle: tik_backbone_forward only; tik_ik_forward refuses it
        if ((rc = md->w0.upload(f.W0->v)) || (rc = md->b0.upload(f.B0->v)) || (rc = md->w3.upload(f.W3->v)) || (rc = md->b3.upload(f.B3->v)) ||
            (rc = md->s30.build(f.W0->v, md->hidden, 1, md->feat, md->feat)) ||
            (rc = md->s33.build(f.W3->v, md->pose_dim, 1, md->hidden, md->hidden)))
            return rc;
        if (md->feat % 32 == 0) {
            const tik::XPackSeg h{f.W0->v.data(), md->feat, 1, md->feat};
            if ((rc = md->xh0.upload(tik::xgemm_pack(&h, 1, md->hidden, 128)))) return rc;
        }
    }
    if ((rc = md->trash.upload(std::vector<unsigned short>(4096, 0)))) return rc;
    apply_env(md.get());
    *out = md.release();
    return TIK_OK;
} catch (const std::bad_alloc&) { return fail(TIK_E_NOMEM, "tik_model_create: out of host memory"); }   // no exception crosses the C ABI

int tik_model_destroy(tik_model_t m) {
    if (m) model_release(m);   // freed now, or when its last online-IK stream is destroyed
    return TIK_OK;
}

int tik_model_out_frames(tik_model_t m, int T) {
    if (!m || T <= 0) return fail(TIK_E_INVALID, "bad model/T");
    for (const Layer& L : m->layers) T = Layer::tout(T, L.stride);
    return T;
}

int tik_model_reserve(tik_model_t m, int N, int T) {
    if (!m || N <= 0 || T <= 0) return fail(TIK_E_INVALID, "tik_model_reserve: bad arguments");
    return model_reserve_ws(m, m->ws[0], N, T);
}

int tik_block_create(const tik_tensor* tensors, int n_tensors, int in_channels, int out_channels, int stride,
                     int residual, const float* A_eff_host, int V, tik_block_t* out) {
    if (!tensors || !A_eff_host || !out || in_channels <= 0 || out_channels <= 0 || stride <= 0 || V <= 0)
        return fail(TIK_E_INVALID, "tik_block_create: bad arguments");
    if (V != 17) return fail(TIK_E_INVALID, "fused block kernel is built for V=17 (coco layout), got V=%d", V);
    TensorMap m;
    FoldedBlock f;
    int rc, prec;
    if ((rc = to_map(tensors, n_tensors, m)) || (rc = precision_from_env(prec)) ||
        (rc = fold_block(m, "", in_channels, out_channels, stride, residual, std::vector<float>(A_eff_host, A_eff_host + V * V), V, f)))
        return rc;
    auto b = std::make_unique<tik_block>();
    b->prec = prec;
    if ((rc = b->layer.pack(f))) return rc;
    *out = b.release();
    return TIK_OK;
}

int tik_block_destroy(tik_block_t b) {
    delete b;
    return TIK_OK;
}

}  // extern "C"
