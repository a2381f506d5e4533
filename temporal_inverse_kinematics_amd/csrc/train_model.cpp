// train_model.cpp — building the trainer handle (include/tik.h, tik_trainer_*):
// the state dict is validated and laid out on the host (train_plan.h), so a
// refused one allocates nothing and never touches the GPU, then uploaded in one
// tail; the entry table, read / write of a tensor's value, gradient and Adam
// state, the step count and the debug hook.
//
// Parameters live in ONE flat fp32 buffer in the reference's tensor layouts
// (so Adam is one launch and a state-dict export is a copy); after every
// update the GEMM-side layouts are re-derived on the device (train_step.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>

#include "train_model.h"

using namespace tik_host;
using namespace tik_train;

namespace {

// (entry, what) -> the flat buffer that holds it: what = 0 value, 1 gradient of the last
// step, 2 Adam exp_avg, 3 Adam exp_avg_sq; a buffer (running statistics, A) has a value only
int entry_base(tik_trainer* t, const char* fn, int i, int what, const void* ptr, const PlanEntry*& e, float*& base) {
    if (!t || i < 0 || i >= (int)t->plan.ents.size() || !ptr || what < 0 || what > 3)
        return fail(TIK_E_INVALID, "%s: bad arguments", fn);
    e = &t->plan.ents[i];
    if (e->kind == 1 && what != 0)
        return fail(TIK_E_INVALID, "%s: '%s' is a buffer (it has a value only)", fn, e->name.c_str());
    DevBuf* const par[4] = {&t->P, &t->G, &t->M, &t->Vv};
    base = (e->kind == 1 ? t->B : *par[what]).p + e->off;
    return TIK_OK;
}

}  // namespace

extern "C" {

int tik_trainer_create(const tik_tensor* tensors, int n_tensors, float lr, tik_trainer_t* out) try {
    if (!tensors || n_tensors <= 0 || !out || !(lr > 0.f)) return fail(TIK_E_INVALID, "tik_trainer_create: bad arguments");
    *out = nullptr;
    // host
    TensorMap m;
    TrainPlan plan;
    int rc;
    if ((rc = to_map(tensors, n_tensors, m)) || (rc = plan_trainer(m, plan))) return rc;
    const int nl = (int)plan.L.size();
    int debug_layer = -1;
    if (const char* e = getenv("TIK_TRAIN_DEBUG_LAYER")) {
        char* end = nullptr;
        const long l = strtol(e, &end, 10);
        if (end == e || *end || l < 0 || l >= nl)
            return fail(TIK_E_INVALID, "tik_trainer_create: TIK_TRAIN_DEBUG_LAYER=%s: expected a layer index 0..%d", e, nl - 1);
        debug_layer = (int)l;
    }
    auto t = std::make_unique<tik_trainer>();
    t->plan = std::move(plan);
    TrainPlan& p = t->plan;
    t->lr = lr;
    t->debug = getenv("TIK_TRAIN_DEBUG") != nullptr;
    t->debug_layer = debug_layer;
    t->mix_sparse = tik::fits_coco_hop2(p.hb.data() + p.A, V);
    t->np = (long long)p.hp.size();
    t->fr.resize(nl);
    t->ev.fr.resize(nl);
    t->dbg_dx.resize(nl);
    t->L.resize(nl);
    for (int i = 0; i < nl; ++i) static_cast<PlanLayer&>(t->L[i]) = p.L[i];
    // device
    {
        const std::vector<float> zeros(p.hp.size(), 0.f);
        if ((rc = t->P.upload(p.hp)) || (rc = t->B.upload(p.hb)) || (rc = t->G.upload(zeros)) || (rc = t->M.upload(zeros)) ||
            (rc = t->Vv.upload(zeros)) || (rc = t->cmap0.upload(p.cmap0)))
            return rc;
    }
    std::vector<float>().swap(p.hp);
    std::vector<float>().swap(p.hb);
    for (TrainLayer& l : t->L) {
        const std::vector<float> zf((size_t)l.cout * l.cinp, 0.f);   // the padding columns of wgf / wrf stay zero
        if ((rc = l.wgf.upload(zf)) || (rc = l.wgb.reserve((size_t)l.cin * l.cout)) ||
            (rc = l.wtf.reserve(3ULL * l.cout * l.cout)) || (rc = l.wtb.reserve(3ULL * l.cout * l.cout)) ||
            (rc = l.aeff.reserve(V * V)) || (rc = l.st1.reserve(4 * l.cout)) || (rc = l.st2.reserve(4 * l.cout)) ||
            (rc = l.st3.reserve(4 * l.cout)))
            return rc;
        if (l.res == RES_CONV && ((rc = l.wrf.upload(zf)) || (rc = l.wrb.reserve((size_t)l.cin * l.cout)))) return rc;
        if ((rc = l.wg_e.reserve((size_t)l.cout * l.cinp)) || (rc = l.b2_e.reserve((size_t)V * l.cout)) ||
            (rc = l.wt_e.reserve(3ULL * l.cout * l.cout)) || (rc = l.bT_e.reserve(l.cout)) ||
            (l.res == RES_CONV && (rc = l.wr_e.reserve((size_t)l.cout * l.cinp))))
            return rc;
    }
    const std::vector<float> zw2((size_t)HIDDEN * p.ldp, 0.f);      // the padding columns of W2^T stay zero
    if ((rc = t->dbn_e.reserve(2 * 4 * V)) || (rc = t->w1b.reserve((size_t)p.feat * HIDDEN)) || (rc = t->w2b.upload(zw2)) ||
        (rc = t->st0.reserve(4 * 4 * V)) || (rc = t->k.reserve(3 * p.kmax)) || (rc = t->loss.reserve(1)) ||
        (rc = derive(t.get(), nullptr)))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    *out = t.release();
    return TIK_OK;
} catch (const std::bad_alloc&) {   // the flat host copies are the model's size; no exception crosses the C ABI
    return fail(TIK_E_NOMEM, "tik_trainer_create: out of host memory");
}

int tik_trainer_destroy(tik_trainer_t t) {
    if (t) {
        (void)hipDeviceSynchronize();
        delete t;   // the one delete of the training host code: create holds the handle in a unique_ptr
    }
    return TIK_OK;
}

int tik_trainer_count(tik_trainer_t t) {
    if (!t) return fail(TIK_E_INVALID, "tik_trainer_count: null handle");
    return (int)t->plan.ents.size();
}

int tik_trainer_tensor(tik_trainer_t t, int i, char* name, int name_len, int64_t* shape4, int* ndim, int* kind) {
    if (!t || i < 0 || i >= (int)t->plan.ents.size()) return fail(TIK_E_INVALID, "tik_trainer_tensor: bad index");
    const PlanEntry& e = t->plan.ents[i];
    if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s", e.name.c_str());
    if (ndim) *ndim = (int)e.shape.size();
    if (shape4)
        for (size_t d = 0; d < e.shape.size() && d < 4; ++d) shape4[d] = e.shape[d];
    if (kind) *kind = e.kind;
    return TIK_OK;
}

// what: 0 value, 1 gradient of the last step, 2 Adam exp_avg, 3 Adam exp_avg_sq (parameters only)
int tik_trainer_read(tik_trainer_t t, int i, int what, float* dst, void* stream) {
    const PlanEntry* e;
    float* base;
    if (const int rc = entry_base(t, "tik_trainer_read", i, what, dst, e, base)) return rc;
    HIP_TRY(hipMemcpyAsync(dst, base, e->numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TIK_OK;
}

int tik_trainer_write(tik_trainer_t t, int i, int what, const float* src, void* stream) {
    const PlanEntry* e;
    float* base;
    if (const int rc = entry_base(t, "tik_trainer_write", i, what, src, e, base)) return rc;
    HIP_TRY(hipMemcpyAsync(base, src, e->numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (what == 0) {   // the derived GEMM layouts and the eval set follow before their next use
        t->derive_stale = true;
        t->version += 1;
        // a new adjacency may leave the COCO hop<=2 pattern: the dense graph mix is right for any A
        if (e->kind == 1 && e->off == t->plan.A) t->mix_sparse = false;
    }
    return TIK_OK;
}

int tik_trainer_set_steps(tik_trainer_t t, long long steps) {
    if (!t) return fail(TIK_E_INVALID, "tik_trainer_set_steps: null handle");
    if (steps < 0) return fail(TIK_E_INVALID, "tik_trainer_set_steps: steps must be >= 0 (got %lld)", steps);
    t->steps = steps;
    return TIK_OK;
}

long long tik_trainer_steps(tik_trainer_t t) { return t ? t->steps : -1; }

int tik_trainer_out_frames(tik_trainer_t t, int T) {
    if (!t || T <= 0) return fail(TIK_E_INVALID, "tik_trainer_out_frames: bad arguments");
    return frame_chain(t->plan, T, nullptr);
}

// Debug / test hook on the last step's saved state: which = 0 block `layer`'s
// output, 2 its tcn conv output U, 3 its ReLU(BN(mix)) H, 4 the mix output Z,
// 5 the gcn conv output Y (channels-last rows), 6 the head's first Linear
// output, 7 the head's train-mode output Oh and 8 its gradient dOh (both as
// (N T', pose_dim) dense, whole rows only); 1 the block's input gradient and 10..14 its gS (identity-residual blocks),
// dU, dH (before the ReLU backward, which is folded into the BatchNorm pass), dZ, dY
// (recorded with TIK_TRAIN_DEBUG=1 / TIK_TRAIN_DEBUG_LAYER=l). Copies
// min(n, size) floats to the device pointer dst.
int tik_trainer_debug(tik_trainer_t t, int which, int layer, float* dst, long long n, void* stream) {
    if (!t || layer < 0 || layer >= (int)t->L.size() || !dst || n < 0) return fail(TIK_E_INVALID, "tik_trainer_debug: bad arguments");
    if (which == 7 || which == 8) {   // the head's train-mode output Oh / its gradient dOh, rows of ldp -> (R, pose_dim) dense
        const DevBuf& h = which == 7 ? t->Oh : t->dOh;
        if (!h.p || t->N <= 0) return fail(TIK_E_INVALID, "tik_trainer_debug: buffer not recorded");
        const size_t pd = (size_t)t->plan.pose_dim, R = (size_t)t->N * t->L.back().tout;
        const size_t rows = std::min<size_t>((size_t)n / pd, R);
        if (rows)
            HIP_TRY(hipMemcpy2DAsync(dst, pd * sizeof(float), h.p, (size_t)t->plan.ldp * sizeof(float), pd * sizeof(float), rows,
                                     hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return TIK_OK;
    }
    const TrainLayer& l = t->L[layer];
    const DevBuf* b = which == 0 ? &l.O : which == 1 ? &t->dbg_dx[layer]
                    : which == 2 ? &l.U : which == 3 ? &l.H : which == 4 ? &l.Z : which == 5 ? &l.Y
                    : which == 6 ? &t->Ph
                    : (which >= 10 && which < 15) ? &t->dbg_b[which - 10] : nullptr;
    if (!b || !b->p) return fail(TIK_E_INVALID, "tik_trainer_debug: buffer not recorded");
    const size_t m = std::min<size_t>((size_t)n, b->n);
    HIP_TRY(hipMemcpyAsync(dst, b->p, m * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return TIK_OK;
}

}  // extern "C"
