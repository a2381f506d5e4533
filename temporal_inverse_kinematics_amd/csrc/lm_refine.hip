// lm_refine.hip — the Levenberg-Marquardt refinement of a frame in ONE launch (tik_fk_refine, and the last
// launch of an online stream's recorded step): one workgroup of LM_T = 256 threads per frame, everything about
// the frame in LDS and registers from the first Rodrigues to the last accept. Only the pose, and optionally the
// cost row and the first linearisation, go back to HBM.
//
//   r(th)    = rel(FK keypoints(th)) - rel(kps)                       rel(x) = x - mean of columns 11 / 12
//   cost(th) = 1/2 sum_k w_k |r_k|^2 + 1/2 mu |th - th0|^2 + 1/2 s |th - thp|^2   (last term only with thp, s > 0)
//   (J^T W J + (mu + s + lambda) I) delta = -(J^T W r + mu (th - th0) + s (th - thp))
//
// With sigma > 0 (tik_fk_refine_robust) the data term is Geman-McClure on s_k = |r_k|^2:
//   rho(s)   = sigma^2 s / (sigma^2 + s)             cost(th) = 1/2 sum_k w_k rho(s_k) + the two quadratic terms
//   omega_k  = w_k rho'(s_k) = w_k (sigma^2 / (sigma^2 + s_k))^2     from the current state's residual
//   (J^T Omega J + (mu + s + lambda) I) delta = -(J^T Omega r + mu (th - th0) + s (th - thp))
// J^T Omega r is the exact gradient of the robust term; the matrix is the Gauss-Newton (IRLS) one: the
// second-derivative term of rho (2 w_k rho''(s_k) J_k^T r_k r_k^T J_k, negative for every s > 0) is dropped on
// purpose, which keeps the matrix positive definite. Accept and reject are judged on the true robust cost. The
// base weights (Lds::rw) and the IRLS weights (Lds::ow, recomputed from the current state's r every iteration:
// the same bits while steps are rejected) both live in LDS; sigma = 0 takes the branches of the plain square,
// uniform over the workgroup, and gives its bits. LDS: 48220 B with 4 skinning entries per vertex, 58636 B with
// the dense table (of them 208 B for Lds::ow).
//
// th: the 66 pose values of joints 0..21; the other 33 joints stay at pose_mean. The policy is refine._lm_loop's
// with a frame as the unit: th + delta is kept where its cost fell (lambda / 3), else th stays (3 lambda); a NaN
// cost or a failed pivot is no fall; exactly `iters` iterations.
//
// The frame's set-up, fk_eval and linearize live in lm_refine_dev.h (shared with fk_kploss.hip).
// FK of a pose (fk_eval; the arithmetic of fk_chain_kernel and fk_joints.hip, other sum orders):
//   1  thread j < 55: R_j = rodrigues_smplx(th_j + pose_mean_j), the pose feature vec(R_j - I)        barrier
//   2  the chain by tree depth, thread j: G_j = G_parent [R_j | J_j - J_parent]           barrier per level
//   3  thread j: A_j, the posed joint P_j; the waves: the 512-wide blend dot products of the vertex
//      keypoints (lane = 8 k, then a butterfly sum over the wave)                                     barrier
//   4  thread (vertex, row): T = sum_n w_n A_k(n) over the skinning entries in table order, x = T (vp, 1)  barrier
//   5  the 17 keypoints, then r                                                                2 barriers
// An FK state (A, P, feature, vp, x, keypoints, r) exists twice: the current pose's and the candidate's; an
// accepted candidate's state becomes the current one (an index flips), nothing is evaluated twice.
// Linearisation of the current state (linearize), skipped while steps are being rejected:
//   a  thread j < 22: dR_j / dth (3 axes) and the world angular velocities; threads 64..: T.R per vertex  barrier
//   b  (column, dof) pairs, 17 x 22 over 256 threads: the 3x3 blocks, chain joints by the ancestor mask,
//      vertices by the masked skinning sum and the pose-blend derivative (fk_jacobian.hip's formulas)  barrier
//   c  rel on the rows of J (thread = (component, unknown))                                           barrier
// Then lm_dev.h on the LDS copy of J: lm_accumulate_body, lm_damp, lm_factor_solve (2 barriers per column and
// per solve step: about 280 of an iteration's about 330 barriers).
// Every sum has a fixed order (FMA chains, fixed butterflies), no atomics, no waiting between workgroups, and
// a workgroup sees only its own frame: a frame's bits do not depend on B or on its place in the batch.
#include "fk_model.h"
#include "lm_refine_dev.h"

namespace tik {
namespace lmr {

// cost of state S at pose th: wave 0, three fixed butterflies; every thread gets the value
__device__ __forceinline__ float cost_of(const LmRefineArgs& a, const Lds& s, const float* S, const float* th, bool tie, float sig2) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        float q0 = 0.f, qp = 0.f;
        for (int i = tid; i < N; i += 64) {
            const float d = th[i] - s.th0[i];
            q0 = fmaf(d, d, q0);
            if (tie) {
                const float e = th[i] - s.thp[i];
                qp = fmaf(e, e, qp);
            }
        }
        const float p = sig2 > 0.f ? weighted_rho(s, S, sig2) : weighted_sq(s, S);   // uniform over the workgroup
        q0 = wave_sum(q0); qp = wave_sum(qp);
        if (tid == 0) s.c[0] = 0.5f * p + 0.5f * a.mu * q0 + (tie ? 0.5f * a.smooth * qp : 0.f);
    }
    __syncthreads();
    const float c = s.c[0];
    __syncthreads();   // s.c is rewritten by the next call
    return c;
}

}  // namespace lmr

__global__ __launch_bounds__(LM_T) void lm_refine_kernel(LmRefineArgs a) {
    using namespace lmr;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int K = skin_count(a);
    const Lds s(smem, K);
    const LmLds L(s.lm, N);

    // where this frame comes from: the batch's rows, or (a stream's step) the ring slot of frame c = count - 1 - h
    const float *poses = a.poses + b * N, *prior = a.prior ? a.prior + b * N : nullptr, *prev = a.prev ? a.prev + b * N : nullptr;
    const float* kps = a.kps ? a.kps + b * M : nullptr;
    const float* conf = nullptr;
    int count = 0;
    if (a.st.count) {
        count = *a.st.count;
        const int c = count - 1 - a.st.h;
        // this push's confidences from pinned host memory (as the dataflow kernel reads the frame) into the slot of
        // frame count - 1, the keypoint ring's index rule; the load is complete before the host is told (the waits below)
        if (tid < NC) a.st.cring[(size_t)((count - 1) % a.st.W) * NC + tid] = a.st.conf_host[tid];
        if (c < 0) {   // the stream is still filling: the pose passes through, have-previous stays clear
            if (tid < N) __hip_atomic_store(a.st.pose_host + tid, poses[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store(a.st.done_host, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        kps = a.st.ring + (size_t)(c % a.st.W) * M;
        conf = a.st.cring + (size_t)(c % a.st.W) * NC;
        prev = (c > 0 && *a.st.have) ? a.st.prev : nullptr;
        __syncthreads();   // h = 0: the slot read is the one just written, by other threads
    }
    const bool tie = prev && a.smooth > 0.f;
    // sigma = 0 (sig2 = 0): the plain weighted square, its arithmetic and its bits; the branches on it are uniform
    const float sig2 = a.sigma * a.sigma;
    const bool robust = sig2 > 0.f;

    int dj, par;
    frame_setup(a, s, poses, prior, prev, tie, kps, conf, (a.flags & TIK_REFINE_SKIP_NONFINITE) != 0, b, K, 2, dj, par);

    int cur = 0;
    fk_eval(a, s, s.state(0), s.th, dj, par, K);
    float cost = cost_of(a, s, s.state(0), s.th, tie, sig2);
    float lam = a.lam0;
    float* hist = a.out_cost ? a.out_cost + b * (a.iters + 1) : nullptr;
    if (hist && tid == 0) hist[0] = cost;
    bool lin = false;
    if (a.dbg_jac || a.dbg_r || a.dbg_w) {   // the first linearisation, rows root-relative
        linearize(a, s, s.state(0), s.th, par, K);
        lin = true;
        if (a.dbg_jac)
            for (int e = tid; e < M * N; e += LM_T) a.dbg_jac[b * M * N + e] = s.J[e];
        if (a.dbg_r && tid < M) a.dbg_r[b * M + tid] = s.state(0)[ST_R + tid];
        if (a.dbg_w && tid < NC) a.dbg_w[b * NC + tid] = robust ? robust_weight(s, s.state(0), tid, sig2) : s.rw[3 * tid];
    }
    const float damp0 = tie ? a.mu + a.smooth : a.mu;
    for (int it = 0; it < a.iters; ++it) {
        const float* S = s.state(cur);
        if (!lin) linearize(a, s, S, s.th, par, K);   // J of a pose that was kept is still in LDS
        lin = true;
        if (tid < N) {
            s.d0[tid] = s.th[tid] - s.th0[tid];
            s.dp[tid] = tie ? s.th[tid] - s.thp[tid] : 0.f;
        }
        // the IRLS weights of the current state's residual: they change only with the state, and recomputing
        // them from the same r gives the same bits, so a rejected step needs no bookkeeping (J in LDS stays valid)
        if (robust && tid < M) s.ow[tid] = robust_weight(s, S, tid / 3, sig2);
        lm_clear(L, N);
        __syncthreads();
        lm_accumulate_body(L, s.J, S + ST_R, robust ? s.ow : s.rw, M, N);
        float g = lm_damp(L, N, damp0 + lam, a.mu, s.d0);
        if (tie && tid < N) g = fmaf(a.smooth, s.dp[tid], g);
        __syncthreads();
        const bool ok = lm_factor_solve(L, N, -g);   // the same verdict in every thread
        bool fell = false;
        float cc = cost;
        if (ok) {
            if (tid < N) s.cand[tid] = s.th[tid] + L.sG[tid];
            __syncthreads();
            fk_eval(a, s, s.state(cur ^ 1), s.cand, dj, par, K);
            cc = cost_of(a, s, s.state(cur ^ 1), s.cand, tie, sig2);
            fell = cc < cost;   // false for a NaN cost
        }
        if (fell) {
            if (tid < N) s.th[tid] = s.cand[tid];
            cur ^= 1;
            cost = cc;
            lam = lam / 3.f;
            lin = false;
        } else {
            lam = lam * 3.f;
        }
        __syncthreads();
        if (hist && tid == 0) hist[it + 1] = cost;
    }

    if (a.out_poses && tid < N) a.out_poses[b * N + tid] = s.th[tid];
    if (a.st.count) {
        // the pose to pinned host memory with ordinary vector stores at system scope, complete in every wave before
        // the host is told (the dataflow kernel's head task does the same); prev and have stay on the device
        if (tid < N) {
            a.st.prev[tid] = s.th[tid];
            __hip_atomic_store(a.st.pose_host + tid, s.th[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (tid == 0) *a.st.have = 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(a.st.done_host, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- host
int lm_refine_model_args(const tik_fk* fk, const char* who, const int* sel17, int iters, float mu, float smooth, float lam0,
                         LmRefineArgs& a) {
    using namespace tik_host;
    if (!fk) return fail(TIK_E_INVALID, "%s: null FK handle", who);
    if (iters < 0) return fail(TIK_E_INVALID, "%s: iters must be >= 0, got %d", who, iters);
    if (!(mu > 0.f)) return fail(TIK_E_INVALID, "%s: mu must be > 0, got %g", who, (double)mu);
    if (!(smooth >= 0.f)) return fail(TIK_E_INVALID, "%s: smooth must be >= 0, got %g", who, (double)smooth);
    if (!(lam0 > 0.f)) return fail(TIK_E_INVALID, "%s: lam0 must be > 0, got %g", who, (double)lam0);
    if (fk->nb < 0 || fk->nb > 32 || lmr::SD0 + fk->nb + fk->ne + 1 > lmr::KP)
        return fail(TIK_E_INVALID, "%s: the model has %d betas and %d expression values, need at most 32 betas in a %d-wide row",
                    who, fk->nb, fk->ne, lmr::KP);
    a = LmRefineArgs{};
    tik_host::fill_sel_args(fk, 0, LMR_COLS, a);
    if (!fkd::nz_ok(a)) return fail(TIK_E_INVALID, "%s: the handle's skinning table has %d entries per vertex", who, a.nz);
    a.nv = 0;
    for (int s = 0; s < LMR_COLS; ++s) {
        const int j = sel17 ? sel17[s] : LMR_COCO_SMPLX[s];
        if (j < 0 || j >= fk->njoints) return fail(TIK_E_INVALID, "%s: joint index %d out of range [0, %d)", who, j, fk->njoints);
        if (j >= 55 + fk->nextra)
            return fail(TIK_E_INVALID, "%s: joint %d is a landmark of three vertices (or a contour landmark); the kernel takes "
                        "chain joints and single-vertex joints (below %d)", who, j, 55 + fk->nextra);
        a.sel[s] = (unsigned short)j;
        a.slot[s] = -1;
        if (j >= 55) {
            a.slot[s] = (signed char)a.nv++;
        }
    }
    a.nb = fk->nb; a.ns = fk->nb + fk->ne; a.maxdepth = fk->maxdepth; a.iters = iters;
    a.mu = mu; a.smooth = smooth; a.lam0 = lam0;
    a.pose_mean = fk->pose_mean.p; a.jt = fk->jt.p; a.jd = fk->jd.p; a.parents = fk->parents.p; a.depth = fk->depth.p; a.anc = fk->anc.p;
    return TIK_OK;
}

int lm_refine_check_sigma(const char* who, float sigma) {
    if (!(sigma >= 0.f) || !(sigma <= 3.0e18f))   // NaN fails both; sigma^2 must stay finite in fp32
        return tik_host::fail(TIK_E_INVALID, "%s: robust_sigma must be >= 0 and finite (0 = off), got %g", who, (double)sigma);
    return TIK_OK;
}

int lm_refine_launch(const LmRefineArgs& a, void* stream) {
    return lm_launch(lm_refine_kernel, a.B, lmr::lds_floats(a.nz > 0 ? a.nz : 55), stream, a);
}

}  // namespace tik

using namespace tik_host;

// both entry points (`who`): every refusal before any device work
static int fk_refine(const char* who, tik_fk_t fk, const float* poses, const float* prior, const float* prev, const float* kps,
                     const float* betas, int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, int iters, float mu,
                     float smooth, float lam0, int B, float* out_poses, float* out_cost, float* dbg_jac, float* dbg_r, float robust_sigma,
                     int flags, float* dbg_w, void* stream) {
    if (!fk || !poses || !kps || !out_poses) return fail(TIK_E_INVALID, "%s: null pointer", who);
    if (B <= 0) return fail(TIK_E_INVALID, "%s: B must be positive, got %d", who, B);
    if (betas && betas_ld != 0 && betas_ld < fk->nb)
        return fail(TIK_E_INVALID, "%s: betas_ld must be 0 (one row for all frames) or >= %d, got %d", who, fk->nb, betas_ld);
    if (joint_w && joint_w_ld != 0 && joint_w_ld != tik::LMR_COLS)
        return fail(TIK_E_INVALID, "%s: joint_w_ld must be 0 (shared) or 17 (per frame), got %d", who, joint_w_ld);
    if (int rc = tik::lm_refine_check_sigma(who, robust_sigma)) return rc;
    if (flags & ~TIK_REFINE_SKIP_NONFINITE) return fail(TIK_E_INVALID, "%s: unknown bit in flags 0x%x", who, (unsigned)flags);
    tik::LmRefineArgs a;
    if (int rc = tik::lm_refine_model_args(fk, who, sel17, iters, mu, smooth, lam0, a)) return rc;
    a.B = B;
    a.poses = poses; a.prior = prior; a.prev = prev; a.kps = kps;
    a.betas = betas; a.betas_ld = betas_ld; a.joint_w = joint_w; a.joint_w_ld = joint_w_ld;
    a.out_poses = out_poses; a.out_cost = out_cost; a.dbg_jac = dbg_jac; a.dbg_r = dbg_r;
    a.sigma = robust_sigma; a.flags = flags; a.dbg_w = dbg_w;
    return tik::lm_refine_launch(a, stream);
}

extern "C" int tik_fk_refine(tik_fk_t fk, const float* poses, const float* prior, const float* prev, const float* kps,
                             const float* betas, int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17, int iters,
                             float mu, float smooth, float lam0, int B, float* out_poses, float* out_cost, float* dbg_jac, float* dbg_r,
                             void* stream) {
    return fk_refine("tik_fk_refine", fk, poses, prior, prev, kps, betas, betas_ld, joint_w, joint_w_ld, sel17, iters, mu, smooth, lam0,
                     B, out_poses, out_cost, dbg_jac, dbg_r, 0.f, 0, nullptr, stream);
}

extern "C" int tik_fk_refine_robust(tik_fk_t fk, const float* poses, const float* prior, const float* prev, const float* kps,
                                    const float* betas, int betas_ld, const float* joint_w, int joint_w_ld, const int* sel17,
                                    int iters, float mu, float smooth, float lam0, int B, float* out_poses, float* out_cost,
                                    float* dbg_jac, float* dbg_r, float robust_sigma, int flags, float* dbg_w, void* stream) {
    return fk_refine("tik_fk_refine_robust", fk, poses, prior, prev, kps, betas, betas_ld, joint_w, joint_w_ld, sel17, iters, mu, smooth,
                     lam0, B, out_poses, out_cost, dbg_jac, dbg_r, robust_sigma, flags, dbg_w, stream);
}
