// fk_forward.cpp — the launch paths of the SMPL-X FK check (include/tik.h:
// tik_fk_forward, tik_fk_joints, tik_fk_joints_jacobian, tik_fk_joints_shape_jacobian).
// Replaces common/smpl_util.py:22-82 (run_smpl_inference) and the third-party
// smplx.SMPLX.forward it calls (lbs + landmarks).
//
// Per call (B bodies):
//   fk_chain            R_j, J, A_j, pose feature (B,512), first 55 joints (wave per body)
//   fk_blend            v_posed(B,3V) = [vec(R-I) | beta | expr | 1] . [posedirs; shapedirs; exprdirs; v_template]
//   fk_skin             T_v(b) = sum_j W[v][j] A_j(b); verts = T_v[:3,:3] v_posed + T_v[:,3] (+ transl)
//   fk_landmarks        21 vertex joints + 51 face landmarks + 17 dynamic contour landmarks
// bf16x3 (default): the blend shapes on xgemm.hip, the skinning on the sparse
// weights (fk.hip, at most 16 live joints per vertex, fp32 FMAs). Batches of
// more than one chunk (2048 bodies) run blend + skin per chunk, the chunks
// alternating between the caller's stream and a handle-owned one, so one
// chunk's HBM-bound skinning runs beside the next chunk's MFMA-bound blend
// shapes (a 2048-body v_posed is 257 MB, about the Infinity Cache); each
// chunk's landmarks follow its skinning in its stream.
// TIK_FK_SKIN=dense: the skinning as a GEMM on the persistent xgemm kernel
// (EPI_SKIN; also the path for weights with more than 16 live joints per
// vertex). fp32: both GEMMs on cgemm.hip.
// (Tried and not kept: the sparse skinning fused into the blend GEMM's
// epilogue, v_posed never in HBM: bitwise equal but 1.31 vs 0.91 ms, the
// per-tile A_j gather is latency-bound; profiles/r05_fk1_*. Also the blends in
// order on one stream with each chunk's skinning on the other: 1.01 vs 0.97 ms
// per 4096 bodies, a lone 2048-body blend takes 0.37 ms and two concurrent
// ones 0.56; profiles/r06_ab_fk_pipe.txt.)
// tik_fk_joints / tik_fk_joints_jacobian / tik_fk_joints_shape_jacobian: the chain
// into a (B,55,3) workspace, then fk_joints.hip / fk_jacobian.hip / fk_shape.hip on
// the vertices the selection is made of.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cgemm.h"
#include "fk.h"
#include "fk_model.h"
#include "xgemm.h"

using namespace tik_host;
static_assert(KP == tik::FK_KP, "the kernels' feature row is the folded one");

namespace {

struct FkInputs {
    const float *pose, *betas, *expr, *transl;
    int B;
};

// What differs between the chain launches of the three paths: where the first 55 joints go and
// the row length there, and which of the feature rows and the two A_j layouts are written.
struct ChainOut {
    float* joints;
    int njoints;
    float *feat, *ablk, *ajt;
    int arows;   // rows of A_j per body in ablk
};

tik::FkChainArgs chain_args(const tik_fk* fk, const FkInputs& in, const ChainOut& o) {
    tik::FkChainArgs c{};
    c.B = in.B; c.nb = fk->nb; c.ne = fk->ne; c.kp = KP; c.kj = KJ; c.njoints = o.njoints; c.nchain = fk->nchain;
    c.pose = in.pose; c.betas = in.betas; c.expr = in.expr; c.transl = in.transl; c.pose_mean = fk->pose_mean.p;
    c.parents = fk->parents.p; c.chain = fk->chain.p; c.jt = fk->jt.p; c.jd = fk->jd.p;
    c.feat = o.feat; c.ablk = o.ablk; c.arows = o.arows; c.ajt = o.ajt;
    c.joints = o.joints; c.dyn_bin = fk->contour ? fk->dyn_bin.p : nullptr;
    c.depth = fk->depth.p; c.maxdepth = fk->maxdepth;
    return c;
}

// bytes of a fk_chain launch: pose (55 x 3) and shape (20) in, `written` floats per body out
constexpr int CHAIN_MESH = KP + 16 * KJ;    // the mesh path: feat and A_j
constexpr int CHAIN_JOINTS = NJ * 3;        // the (B,55,3) workspace ...
constexpr int CHAIN_WS = KP + 12 * NJ;      // ... + feat and ajt, when a selected joint is made of vertices
double chain_bytes(int B, int written) { return 4.0 * (double)B * (NJ * 3 + 20 + written); }

// The chain of the mesh-free paths: its joints into the (B,55,3) workspace; the feature rows and
// A_j only when `ws` (a vertex will be evaluated).
int launch_chain_joints(tik_fk* fk, const FkInputs& in, bool ws, hipStream_t st) {
    const tik::FkChainArgs c =
        chain_args(fk, in, ChainOut{fk->jchain.p, NJ, ws ? fk->feat.p : nullptr, nullptr, ws ? fk->ajt.p : nullptr, 12});
    ProfRange pr(fk->profiling ? &fk->prof : nullptr, "fk_chain", 0.0, chain_bytes(in.B, CHAIN_JOINTS + (ws ? CHAIN_WS : 0)), st);
    HIP_TRY(tik::launch_fk_chain(c, st));
    return TIK_OK;
}

// workspace of the mesh-free paths: chain joints 165 floats + the bin per body, feat 512 + A_j 660
// when `ws`; never the mesh path's v_posed / vertex / ablk buffers or its second stream
int reserve_joints_ws(tik_fk* fk, int B, bool ws) {
    int rc;
    if ((rc = fk->jchain.reserve((size_t)B * NJ * 3)) || (fk->contour && (rc = fk->dyn_bin.reserve((size_t)B))) ||
        (ws && ((rc = fk->feat.reserve((size_t)B * KP)) || (rc = fk->ajt.reserve((size_t)B * NJ * 12)))))
        return rc;
    return TIK_OK;
}

// A joint selection (sel, or 0 .. n - 1 when null) into the kernels' 16-bit table: every index
// is range-checked before it is narrowed. -> its number of vertex evaluations in npick.
int resolve_selection(const tik_fk* fk, const char* who, const int* sel, int n, bool refuse_contour, unsigned short* out, int& npick) {
    const int nstatic = NJ + fk->nextra + fk->nlmk;
    npick = 0;
    for (int s = 0; s < n; ++s) {
        const int j = sel ? sel[s] : s;
        if (j < 0 || j >= fk->njoints) return fail(TIK_E_INVALID, "%s: joint index %d out of range [0, %d)", who, j, fk->njoints);
        if (refuse_contour && j >= nstatic)
            return fail(TIK_E_INVALID, "%s: joint %d is a contour landmark: its vertices are picked by a "
                        "pose-dependent bin (piecewise constant), so it has no Jacobian here", who, j);
        if (sel) out[s] = (unsigned short)j;
        npick += j < NJ ? 0 : j < NJ + fk->nextra ? 1 : 3;
    }
    return TIK_OK;
}

// The two Jacobian entry points between their checks and their own kernels: the joints first, on tik_fk_joints itself
// (its bits, its "fk_chain" / "fk_joints" launches); the workspace, its 1337 floats per body + the entry point's own
// (include/tik.h); the chain with feat and A_j forced on unless tik_fk_joints ran it so (npick > 0); then k's base.
int jacobian_inputs(tik_fk* fk, const FkInputs& in, const int* sel, int n_sel, int npick, float* joints, DevBuf& own,
                    size_t own_floats, tik::FkSelArgs& k, hipStream_t st) {
    int rc;
    if (joints && (rc = tik_fk_joints(fk, in.pose, in.betas, in.expr, in.transl, in.B, sel, n_sel, joints, st))) return rc;
    if ((rc = reserve_joints_ws(fk, in.B, true)) || (rc = own.reserve(in.B * own_floats))) return rc;
    if ((!joints || npick == 0) && (rc = launch_chain_joints(fk, in, true, st))) return rc;
    fill_sel_args(fk, in.B, n_sel, k);
    return TIK_OK;
}

}  // namespace

extern "C" {

int tik_fk_forward(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                   const float* transl, int B, float* joints, float* verts, void* stream) {
    if (!fk || !full_pose || !joints || B <= 0) return fail(TIK_E_INVALID, "tik_fk_forward: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = tik_fk_reserve(fk, B))) return rc;
    float* vout = verts;
    if (!vout) {
        if ((rc = fk->verts_ws.reserve((size_t)B * 3 * fk->V))) return rc;
        vout = fk->verts_ws.p;
    }
    const bool bf = fk->prec == tik::PREC_BF16X3;
    const bool sparse = bf && fk->sp_nz > 0;
    // rows of A_j per body in ablk: the bf16x3 skinning GEMM skips the [0 0 0 1] row
    const int ar = bf ? 12 : 16;
    const tik::FkChainArgs c = chain_args(fk, FkInputs{full_pose, betas, expression, transl, B},
                                          ChainOut{joints, fk->njoints, fk->feat.p, sparse ? nullptr : fk->ablk.p,
                                                   sparse ? fk->ajt.p : nullptr, ar});
    Profiler* pf = fk->profiling ? &fk->prof : nullptr;
    const double Vd = fk->V;
    const int V3 = 3 * fk->V;
    const float* tr = transl ? transl : fk->zero_transl.p;
    {
        ProfRange pr(pf, "fk_chain", 0.0, chain_bytes(B, CHAIN_MESH), st);
        HIP_TRY(tik::launch_fk_chain(c, st));
    }
    // v_posed = feat . P for n bodies. Algorithmic: K = 507 live blend-shape columns (486 pose +
    // 20 shape + template); bytes: feat rows in, v_posed out, P^T once
    auto blend_range = [&](int n, hipStream_t s) {
        return ProfRange(pf, "fk_blend", 2.0 * n * V3 * 507, 4.0 * ((double)n * KP + (double)n * V3 + (double)V3 * 507), s);
    };

    // v_posed = feat . P on xgemm.hip (bf16x3, fp32 feat rows by LDS-DMA), bodies b0 .. b0 + n
    auto blend = [&](int b0, int n, float* vp, hipStream_t s) -> int {
        tik::XArgs g{};
        g.M = n; g.Nc = V3; g.V = 1; g.tout = n;
        g.seg[0] = tik::XSeg{fk->feat.p + (size_t)b0 * KP, KP, KP, 1, 1, 0, n, n};
        g.nseg = 1; g.wp = fk->xPT.p;
        g.out = vp; g.ldo = fk->ldv; g.act = tik::ACT_NONE;
        // P^T (V3 x 512 bf16x3, ~97 MB) is the large operand: group the row tiles so each XCD
        // streams it about once (its contiguous run of workgroups covers gm row tiles x all columns)
        { const int gx = (n + 127) / 128; g.gm = (gx + 7) / 8; }
        ProfRange pr = blend_range(n, s);
        HIP_TRY(tik::launch_xgemm(g, 128, tik::EPI_BIAS, s));
        return TIK_OK;
    };
    // skinning + vertex transform on the sparse weights (fk.hip): fp32 FMAs over each vertex's joints
    auto skin = [&](int b0, int n, const float* vp, hipStream_t s) -> int {
        tik::FkSkinSpArgs k{};
        k.B = n; k.V = fk->V; k.nz = fk->sp_nz; k.ajt = fk->ajt.p + (size_t)b0 * 12; k.ajt_ld = B;
        k.nzw = reinterpret_cast<const int2*>(fk->nzw.p);
        k.vposed = vp; k.ldv = fk->ldv; k.transl = tr + (size_t)b0 * 3; k.verts = vout + (size_t)b0 * V3;
        k.ncu = fk->ncu;
        // algorithmic: nz joints x 12 entries + the 3x4 vertex transform per (body, vertex);
        // bytes: A_j in, v_posed in, vertices out, the pairs once
        ProfRange pr(pf, "fk_skin", 2.0 * n * Vd * (12.0 * fk->sp_nz + 9.0),
                     4.0 * ((double)n * 12 * NJ + 2.0 * n * V3 + 2.0 * Vd * fk->sp_nz), s);
        HIP_TRY(tik::launch_fk_skin_sparse(k, s));
        return TIK_OK;
    };

    // the 21 vertex joints and 89 landmarks of bodies b0 .. b0 + n (after their vertices)
    auto lmk = [&](int b0, int n, hipStream_t s) -> int {
        tik::FkLmkArgs l{};
        l.B = n; l.V = fk->V; l.njoints = fk->njoints; l.nextra = fk->nextra; l.nlmk = fk->nlmk; l.ndyn = fk->ndyn;
        l.verts = vout + (size_t)b0 * V3; l.transl = transl ? transl + (size_t)b0 * 3 : nullptr;
        l.extra = fk->extra.p; l.faces = fk->faces.p; l.lmk_faces = fk->lmk_faces.p;
        l.lmk_bary = fk->lmk_bary.p; l.dyn_faces = fk->dyn_faces.p; l.dyn_bary = fk->dyn_bary.p;
        l.dyn_bin = fk->dyn_bin.p + b0; l.joints = joints + (size_t)b0 * fk->njoints * 3;
        ProfRange pr(pf, "fk_landmarks", 0.0, 4.0 * (double)n * (3.0 * 144 + 3.0 * 3 * 3 * 89), s);
        HIP_TRY(tik::launch_fk_landmarks(l, s));
        return TIK_OK;
    };

    if (sparse) {
        const int CH = fk->chunk, nch = (B + CH - 1) / CH;
        if (nch > 1 && !fk->aux) {
            HIP_TRY(hipStreamCreateWithFlags(&fk->aux, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&fk->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&fk->ev_join, hipEventDisableTiming));
        }
        if (nch > 1) {
            HIP_TRY(hipEventRecord(fk->ev_fork, st));
            HIP_TRY(hipStreamWaitEvent(fk->aux, fk->ev_fork, 0));
        }
        for (int k = 0; k < nch; ++k) {
            const int b0 = k * CH, n = std::min(CH, B - b0);
            hipStream_t s = (k & 1) ? fk->aux : st;
            // two v_posed chunk buffers, one per stream (reused in stream order)
            float* vp = fk->vposed.p + (size_t)(nch > 1 ? (k & 1) * CH : 0) * fk->ldv;
            // each chunk's landmarks in its stream, beside the other stream's skinning
            if ((rc = blend(b0, n, vp, s)) || (rc = skin(b0, n, vp, s)) || (rc = lmk(b0, n, s))) return rc;
        }
        if (nch > 1) {
            HIP_TRY(hipEventRecord(fk->ev_join, fk->aux));
            HIP_TRY(hipStreamWaitEvent(st, fk->ev_join, 0));
        }
    } else if (bf) {
        if ((rc = blend(0, B, fk->vposed.p, st))) return rc;
        // skinning + vertex transform as a GEMM on the persistent xgemm kernel (EPI_SKIN): the DMA
        // pipeline runs across tiles (K = 64 is 2 steps per tile); rows = body * 12 + transform entry
        tik::XArgs s{};
        s.M = B * ar; s.Nc = fk->V; s.V = 1; s.tout = B * ar;
        s.seg[0] = tik::XSeg{fk->ablk.p, KJ, KJ, 1, 1, 0, B * ar, (long long)B * ar};
        s.nseg = 1; s.wp = fk->xWT.p; s.skin_rows = ar;
        s.resid = fk->vposed.p; s.ldr = fk->ldv; s.out = vout; s.ldo = V3; s.act = tik::ACT_NONE;
        s.bias = tr;
        s.trash = reinterpret_cast<float*>(fk->trash.p);
        // algorithmic: 12 transform entries x 55 joints per (body, vertex) + the
        // 3x4 vertex transform; bytes: A_j rows and v_posed in, vertices out, W once
        ProfRange pr(pf, "fk_skin", 2.0 * B * Vd * 12 * NJ + 18.0 * B * Vd,
                     4.0 * ((double)B * 12 * NJ + 2.0 * B * V3 + Vd * NJ), st);
        HIP_TRY(tik::launch_xgemm_pt(s, 128, fk->ncu, st, tik::EPI_SKIN));
    } else {
        {
            tik::CgemmArgs g{};   // v_posed = feat . P (exact fp32 MFMA)
            g.M = B; g.Nc = V3; g.V = 1; g.tout = B;
            g.seg[0] = tik::Seg{fk->feat.p, fk->PT.p, KP, KP, 1, 1, 0, B, KP};
            g.nseg = 1; g.out = fk->vposed.p; g.ldo = fk->ldv; g.act = tik::ACT_NONE;
            ProfRange pr = blend_range(B, st);
            HIP_TRY(tik::launch_cgemm(g, tik::CFG_T128x128, st, tik::PREC_F32));
        }
        tik::CgemmArgs s{};   // skinning + vertex transform (exact fp32 MFMA)
        s.M = B * 16; s.Nc = fk->V; s.V = 1; s.tout = B * 16;
        s.seg[0] = tik::Seg{fk->ablk.p, fk->WT.p, KJ, KJ, 1, 1, 0, B * 16, KJ};
        s.nseg = 1; s.resid = fk->vposed.p; s.ldr = fk->ldv; s.out = vout; s.ldo = V3; s.bias = transl;
        ProfRange pr(pf, "fk_skin", 2.0 * B * Vd * 16 * NJ + 18.0 * B * Vd,
                     4.0 * ((double)B * 16 * NJ + 2.0 * B * V3 + Vd * NJ), st);
        HIP_TRY(tik::launch_cgemm(s, tik::CFG_S128x128, st, tik::PREC_F32));
    }

    if (!sparse) return lmk(0, B, st);
    return TIK_OK;
}

int tik_fk_joints(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                  const float* transl, int B, const int* sel_host, int n_sel, float* out, void* stream) {
    if (!fk || !full_pose || !out || B <= 0) return fail(TIK_E_INVALID, "tik_fk_joints: bad arguments");
    if (sel_host && (n_sel < 1 || n_sel > tik::FKJ_MAX_SEL))
        return fail(TIK_E_INVALID, "tik_fk_joints: n_sel must be 1..%d, got %d", tik::FKJ_MAX_SEL, n_sel);
    if (fk->njoints > 65535) return fail(TIK_E_INVALID, "tik_fk_joints: too many joints");
    hipStream_t st = (hipStream_t)stream;
    tik::FkJointsArgs k{};   // the selection travels in the kernel arguments: nothing is uploaded per call
    k.sel_all = sel_host ? 0 : 1;
    const int n_out = sel_host ? n_sel : fk->njoints;
    int rc, npick;           // vertex evaluations of this selection
    if ((rc = resolve_selection(fk, "tik_fk_joints", sel_host, n_out, false, k.sel, npick)) ||
        (rc = reserve_joints_ws(fk, B, npick > 0)) ||
        (rc = launch_chain_joints(fk, FkInputs{full_pose, betas, expression, transl, B}, npick > 0, st)))
        return rc;
    fill_sel_args(fk, B, n_out, k);
    k.nlmk = fk->nlmk; k.ndyn = fk->ndyn; k.feat = fk->feat.p; k.jchain = fk->jchain.p; k.transl = transl;
    k.dyn_v = fk->dyn_v.p; k.dyn_w = fk->dyn_bary.p; k.dyn_bin = fk->dyn_bin.p; k.out = out;
    // algorithmic, per vertex evaluation: 3 dot products of 507 + the skinning sum + the 3x4 transform;
    // bytes: feat and A_j in, the picked P^T rows once, the joints out
    const double terms = k.nz ? k.nz : NJ;
    ProfRange pr(fk->profiling ? &fk->prof : nullptr, "fk_joints", 2.0 * B * npick * (3.0 * 507 + 12.0 * terms + 9.0),
                 4.0 * ((double)B * (npick ? KP + 12 * NJ : 0) + 3.0 * 507 * npick + 3.0 * B * NJ + 3.0 * B * n_out), st);
    HIP_TRY(tik::launch_fk_joints(k, st));
    return TIK_OK;
}

int tik_fk_joints_jacobian(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                           const float* transl, int B, const int* sel_host, int n_sel, const int* dof_host, int n_dof,
                           float* jac, float* joints, void* stream) {
    if (!fk || !full_pose || !sel_host || !jac || B <= 0) return fail(TIK_E_INVALID, "tik_fk_joints_jacobian: bad arguments");
    if (n_sel < 1 || n_sel > tik::FKJ_MAX_SEL)
        return fail(TIK_E_INVALID, "tik_fk_joints_jacobian: n_sel must be 1..%d, got %d", tik::FKJ_MAX_SEL, n_sel);
    if (dof_host && (n_dof < 1 || n_dof > NJ))
        return fail(TIK_E_INVALID, "tik_fk_joints_jacobian: n_dof must be 1..%d, got %d", NJ, n_dof);
    hipStream_t st = (hipStream_t)stream;
    tik::FkJacArgs k{};   // selection and dof list travel in the kernel arguments: nothing is uploaded per call
    int rc, npick;
    if ((rc = resolve_selection(fk, "tik_fk_joints_jacobian", sel_host, n_sel, true, k.sel, npick))) return rc;
    k.n_dof = dof_host ? n_dof : 22;
    unsigned long long seen = 0;
    for (int d = 0; d < k.n_dof; ++d) {
        const int j = dof_host ? dof_host[d] : d;
        if (j < 0 || j >= NJ) return fail(TIK_E_INVALID, "tik_fk_joints_jacobian: dof joint %d out of range [0, %d)", j, NJ);
        if ((seen >> j) & 1ull) return fail(TIK_E_INVALID, "tik_fk_joints_jacobian: dof joint %d repeated", j);
        seen |= 1ull << j;
        k.dof[d] = (unsigned char)j;
    }
    if ((rc = jacobian_inputs(fk, FkInputs{full_pose, betas, expression, transl, B}, sel_host, n_sel, npick, joints, fk->jacw,
                              tik::FKJAC_WS, k, st))) return rc;
    k.pose = full_pose; k.pose_mean = fk->pose_mean.p; k.parents = fk->parents.p; k.anc = fk->anc.p;
    k.feat = fk->feat.p; k.jchain = fk->jchain.p; k.transl = transl; k.jw = fk->jacw.p; k.jac = jac;
    // algorithmic, per (vertex evaluation, dof): the masked skinning sum, three cross products, the
    // 27-term pose-blend derivative and its 3x3 transform; per vertex evaluation the 3 dot products of
    // 507; bytes: the Jacobian out, feat / A_j / chain joints in, the dof workspace written and read
    const double terms = k.nz ? k.nz : NJ, nd = k.n_dof;
    ProfRange pr(fk->profiling ? &fk->prof : nullptr, "fk_jacobian",
                 2.0 * B * (npick * (3.0 * 507 + 12.0 * terms + nd * (4.0 * terms + 27 + 81 + 27)) + 9.0 * n_sel * nd + 150.0 * nd),
                 4.0 * B * (9.0 * n_sel * nd + KP + 12 * NJ + 3 * NJ + 2.0 * tik::FKJAC_PER_DOF * nd), st);
    HIP_TRY(tik::launch_fk_jacobian(k, st));
    return TIK_OK;
}

int tik_fk_joints_shape_jacobian(tik_fk_t fk, const float* full_pose, const float* betas, const float* expression,
                                 const float* transl, int B, const int* sel_host, int n_sel, float* jac, float* joints,
                                 void* stream) {
    if (!fk || !full_pose || !sel_host || !jac || B <= 0) return fail(TIK_E_INVALID, "tik_fk_joints_shape_jacobian: bad arguments");
    if (n_sel < 1 || n_sel > tik::FKJ_MAX_SEL)
        return fail(TIK_E_INVALID, "tik_fk_joints_shape_jacobian: n_sel must be 1..%d, got %d", tik::FKJ_MAX_SEL, n_sel);
    if (fk->nb < 1 || fk->nb > tik::FKS_MAX_NB)
        return fail(TIK_E_INVALID, "tik_fk_joints_shape_jacobian: the model has %d betas, need 1..%d", fk->nb, tik::FKS_MAX_NB);
    hipStream_t st = (hipStream_t)stream;
    tik::FkShapeArgs k{};   // the selection travels in the kernel arguments: nothing is uploaded per call
    int rc, npick;
    if ((rc = resolve_selection(fk, "tik_fk_joints_shape_jacobian", sel_host, n_sel, true, k.sel, npick))) return rc;
    if ((rc = jacobian_inputs(fk, FkInputs{full_pose, betas, expression, transl, B}, sel_host, n_sel, npick, joints, fk->shpw,
                              (size_t)tik::FKS_PER_BETA * fk->nb, k, st))) return rc;
    k.nb = fk->nb; k.ns = fk->nb + fk->ne; k.parents = fk->parents.p; k.jd = fk->jd.p; k.sw = fk->shpw.p; k.jac = jac;
    // algorithmic, per (body, beta): the chain's 54 rotated differences; per (vertex evaluation,
    // skinning entry, beta): a 3x3 product, the add of dP and the weighted sum; bytes: the Jacobian
    // out, A_j in, the beta workspace written and read
    const double terms = k.nz ? k.nz : NJ, nbd = k.nb;
    ProfRange pr(fk->profiling ? &fk->prof : nullptr, "fk_shape_jacobian",
                 2.0 * B * nbd * (54.0 * 12 + npick * terms * 15.0),
                 4.0 * B * (3.0 * n_sel * nbd + 12 * NJ + 2.0 * tik::FKS_PER_BETA * nbd), st);
    HIP_TRY(tik::launch_fk_shape_jacobian(k, st));
    return TIK_OK;
}

}  // extern "C"
