// fk_model.h — the SMPL-X FK handle, shared by fk_model.cpp (create: fold on
// the host, then one upload; reserve, profile, the getters) and fk_forward.cpp
// (the three launch paths).
#pragma once
#include <atomic>

#include "common.h"
#include "fk.h"
#include "fk_fold.h"

struct tik_fk {
    std::atomic<int> refs{1};   // the handle + every online-IK stream that refines with it (fk_retain / fk_release)
    int V = 0, F = 0, nb = 0, ne = 0, nlmk = 0, ndyn = 0, nextra = 0, njoints = 0;
    bool contour = false;
    tik_host::DevBuf PT;         // [3V][KP]    (fp32 path)
    tik_host::DevBuf WT;         // [V][KJ]     (fp32 path)
    tik_host::DevHBuf xPT;       // bf16x3 tiles of P^T for xgemm.hip (the blend-shape GEMM, unfused paths)
    bool dense = false;   // TIK_FK_SKIN=dense: the skinning GEMM even when the weights are sparse
    // bodies per blend + skin chunk (TIK_FK_CHUNK at creation; >= B: one blend + one skin, the
    // round-4 arrangement). Same box, alternating (profiles/r06_fk_ab_chunk.txt): 2048 4.02-4.04M
    // bodies/s, 1024 3.93-3.95M, one chunk (4096) 3.91-3.95M
    int chunk = 2048;
    hipStream_t aux = nullptr;           // the second stream of the chunk pipeline
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ~tik_fk() {
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (aux) (void)hipStreamDestroy(aux);
    }
    tik_host::DevHBuf xWT;       // bf16x3 tiles of W^T for xgemm.hip (the dense skinning GEMM, EPI_SKIN)
    int ncu = 256;
    int prec = 2;
    // sparse skinning (fused, or fk.hip fk_skin_sparse_kernel): per vertex the joints with
    // W > 2^-30 as {joint, weight} pairs, sp_nz per vertex (0: more than 16, the dense GEMM)
    tik_host::DevIBuf nzw;
    int sp_nz = 0;
    tik_host::DevBuf jt, jd, pose_mean, lmk_bary, dyn_bary;
    tik_host::DevIBuf parents, chain, faces, lmk_faces, dyn_faces, extra, depth;
    int nchain = 0, maxdepth = 0;
    int ldv = 0;       // v_posed row stride (3V rounded up to 4 floats: vector stores)
    // workspace
    tik_host::DevBuf feat, ablk, vposed, verts_ws, ajt;
    tik_host::DevHBuf trash;
    tik_host::DevBuf zero_transl;   // (B,3) zeros: the skinning kernel always reads a translation
    tik_host::DevIBuf dyn_bin;
    int cap = 0;
    // tik_fk_joints (fk_joints.hip): per joint >= 55 its (vertex, barycentric weight) picks, the
    // contour's by bin; workspace: the chain's (B,55,3) joints (feat, ajt, dyn_bin are shared)
    tik_host::DevIBuf pick_v, dyn_v;
    tik_host::DevBuf pick_w, jchain;
    // tik_fk_joints_jacobian (fk_jacobian.hip): bit j of anc[k] = joint j is k or an ancestor of k;
    // workspace: dR and omega of every dof (FKJAC_WS floats per body)
    tik_host::DevArray<unsigned long long> anc;
    tik_host::DevBuf jacw;
    // tik_fk_joints_shape_jacobian (fk_shape.hip): workspace: d(chain joints) / d(beta) of every beta
    // (FKS_PER_BETA nb floats per body)
    tik_host::DevBuf shpw;
    tik_host::Profiler prof;     // per-launch HIP events (tik_fk_profile; bench.py's FK roofline)
    bool profiling = false;
};

namespace tik_host {

inline void fk_retain(tik_fk* fk) { fk->refs.fetch_add(1); }   // a refining stream keeps its body model alive
inline void fk_release(tik_fk* fk) {
    if (fk->refs.fetch_sub(1) == 1) delete fk;
}

// The arguments the mesh-free kernels share (fk_joints.hip, fk_jacobian.hip, fk_shape.hip, lm_refine.hip), from the
// handle (after its workspace is reserved; sel is set by the caller).
inline void fill_sel_args(const tik_fk* fk, int B, int n_sel, tik::FkSelArgs& k) {
    k.B = B; k.n_sel = n_sel; k.nextra = fk->nextra; k.nz = fk->dense ? 0 : fk->sp_nz;
    k.ajt = fk->ajt.p; k.PT = fk->PT.p; k.WT = fk->WT.p; k.nzw = reinterpret_cast<const int2*>(fk->nzw.p);
    k.pick_v = fk->pick_v.p; k.pick_w = fk->pick_w.p;
}

}  // namespace tik_host
