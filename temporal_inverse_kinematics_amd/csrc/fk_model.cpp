// fk_model.cpp — building the SMPL-X FK handle (include/tik.h, tik_fk_*): the
// constant set is validated and folded on the host (fk_fold.h), so a refused
// one allocates nothing and never touches the GPU, then uploaded in one tail;
// the handle's workspace, precision, getters and profiler.
// Replaces common/smpl_util.py:8-19 (load_smplx_models) and the constants of
// the third-party smplx.SMPLX it builds.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>

#include "cgemm.h"
#include "fk.h"
#include "fk_model.h"
#include "xgemm.h"

using namespace tik_host;

extern "C" {

int tik_fk_create(const tik_tensor* tensors, int n_tensors, int flags, tik_fk_t* out) try {
    if (!tensors || n_tensors <= 0 || !out) return fail(TIK_E_INVALID, "tik_fk_create: null argument");
    *out = nullptr;
    // host
    TensorMap m;
    FoldedSmplx f;
    int rc, prec;
    if ((rc = to_map(tensors, n_tensors, m)) || (rc = fold_smplx(m, flags, f)) || (rc = precision_from_env(prec))) return rc;
    const char* skin = getenv("TIK_FK_SKIN");   // sparse (default) | dense
    const char* chunk = getenv("TIK_FK_CHUNK");
    // device
    auto fk = std::make_unique<tik_fk>();
    fk->V = f.V; fk->F = f.F; fk->nb = f.nb; fk->ne = f.ne; fk->nlmk = f.nlmk; fk->ndyn = f.ndyn; fk->nextra = f.nextra;
    fk->njoints = f.njoints; fk->contour = f.contour; fk->nchain = f.nchain; fk->maxdepth = f.maxdepth; fk->ldv = f.ldv;
    fk->prec = prec;
    fk->dense = skin && !strcmp(skin, "dense");
    if (chunk) fk->chunk = std::max(1, atoi(chunk));
    if (f.nz && !fk->dense) fk->sp_nz = f.nz;
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
        fk->ncu = ncu;
    const tik::XPackSeg ps{f.PT.data(), KP, 1, KP}, ws{f.WT.data(), KJ, 1, KJ};
    if ((rc = fk->PT.upload(f.PT)) || (rc = fk->WT.upload(f.WT)) || (rc = fk->jt.upload(f.jt)) || (rc = fk->jd.upload(f.jd)) ||
        (rc = fk->pose_mean.upload(f.pose_mean)) || (rc = fk->lmk_bary.upload(f.lmk_bary)) || (rc = fk->parents.upload(f.parents)) ||
        (rc = fk->chain.upload(f.chain)) || (rc = fk->faces.upload(f.faces)) || (rc = fk->lmk_faces.upload(f.lmk_faces)) ||
        (rc = fk->extra.upload(f.extra)) || (rc = fk->depth.upload(f.depth)) ||
        (fk->sp_nz && (rc = fk->nzw.upload(f.nzw))) ||
        (rc = fk->xPT.upload(tik::xgemm_pack(&ps, 1, 3 * f.V, 128))) || (rc = fk->xWT.upload(tik::xgemm_pack(&ws, 1, f.V, 128))) ||
        (rc = fk->dyn_faces.upload(f.dyn_faces)) || (rc = fk->dyn_bary.upload(f.dyn_bary)) ||
        (rc = fk->pick_v.upload(f.pick_v)) || (rc = fk->pick_w.upload(f.pick_w)) || (rc = fk->dyn_v.upload(f.dyn_v)) ||
        (rc = fk->anc.upload(f.anc)))
        return rc;
    *out = fk.release();
    return TIK_OK;
} catch (const std::bad_alloc&) {   // the host copies are large (P^T: 3 V 512 floats); no exception crosses the C ABI
    return fail(TIK_E_NOMEM, "tik_fk_create: out of host memory");
}

int tik_fk_destroy(tik_fk_t handle) {
    if (handle) fk_release(handle);   // freed now, or when the last stream that refines with it is destroyed
    return TIK_OK;
}

int tik_fk_set_precision(tik_fk_t fk, int prec) {
    if (!fk || (prec != tik::PREC_F32 && prec != tik::PREC_BF16X3))
        return fail(TIK_E_INVALID, "tik_fk_set_precision: precision must be 0 (fp32) or 2 (bf16x3), got %d", prec);
    fk->prec = prec;
    return TIK_OK;
}

int tik_fk_num_joints(tik_fk_t fk) {
    if (!fk) return fail(TIK_E_INVALID, "null fk handle");
    return fk->njoints;
}

int tik_fk_num_verts(tik_fk_t fk) {
    if (!fk) return fail(TIK_E_INVALID, "null fk handle");
    return fk->V;
}

int tik_fk_reserve(tik_fk_t fk, int B) {
    if (!fk || B <= 0) return fail(TIK_E_INVALID, "tik_fk_reserve: bad arguments");
    if (B <= fk->cap) return TIK_OK;
    int rc;
    if ((rc = fk->feat.reserve((size_t)B * KP)) || (rc = fk->ablk.reserve((size_t)B * 16 * KJ)) ||
        (rc = fk->vposed.reserve((size_t)std::max(B, 2 * std::min(fk->chunk, B)) * fk->ldv)) || (rc = fk->dyn_bin.reserve((size_t)B)) ||
        (fk->sp_nz && (rc = fk->ajt.reserve((size_t)B * 55 * 12))) ||
        (rc = fk->zero_transl.upload(std::vector<float>((size_t)B * 3, 0.f))) ||
        (!fk->trash.p && (rc = fk->trash.upload(std::vector<unsigned short>(4096, 0)))))
        return rc;
    fk->cap = B;
    return TIK_OK;
}

long long tik_fk_workspace_bytes(tik_fk_t fk) {
    if (!fk) return fail(TIK_E_INVALID, "null fk handle");
    return (long long)(4 * (fk->feat.n + fk->ablk.n + fk->vposed.n + fk->verts_ws.n + fk->ajt.n + fk->zero_transl.n +
                            fk->dyn_bin.n + fk->jchain.n + fk->jacw.n + fk->shpw.n) + 2 * fk->trash.n);
}

int tik_fk_profile(tik_fk_t fk, int max_launches) {
    if (!fk || max_launches < 0) return fail(TIK_E_INVALID, "tik_fk_profile: bad arguments");
    fk->profiling = max_launches > 0;
    return max_launches > 0 ? fk->prof.enable(max_launches) : (fk->prof.clear(), TIK_OK);
}

int tik_fk_profile_count(tik_fk_t fk) {
    if (!fk) return fail(TIK_E_INVALID, "null FK handle");
    return (int)fk->prof.recs.size();
}

int tik_fk_profile_read(tik_fk_t fk, int i, char* label, int label_len, float* ms, double* flops, double* bytes) {
    if (!fk) return fail(TIK_E_INVALID, "tik_fk_profile_read: null FK handle");
    return fk->prof.read(i, label, label_len, ms, flops, bytes);
}

}  // extern "C"
