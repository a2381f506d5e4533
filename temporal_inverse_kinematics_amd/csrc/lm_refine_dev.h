// lm_refine_dev.h — the device pieces that the one-workgroup-per-frame kernels share: lm_refine_kernel (lm_refine.hip, the
// whole Levenberg-Marquardt refinement) and fk_kploss_kernel (fk_kploss.hip, the keypoint loss and its pose gradient).
// Both keep everything about a frame in LDS: the carving of that LDS (Lds), the frame's set-up (frame_setup), the FK of a
// pose with its residual (fk_eval) and the analytic Jacobian of the residual (linearize). All inlined, on LmRefineArgs
// (lm_refine.h); lm_refine.hip's header comment states the phases and the order of every sum.
#pragma once
#include <type_traits>

#include "fk_dev.h"
#include "lm_dev.h"
#include "lm_refine.h"

namespace tik {
namespace lmr {
using namespace fkd;

constexpr int N = LMR_N, M = LMR_M, NC = LMR_COLS, ND = LMR_DOF, NJ = 55;
constexpr int r4(int x) { return (x + 3) & ~3; }
// an FK state, float offsets (every one a multiple of 4: the feature row is read 16 B at a time)
constexpr int ST_A = 0, ST_P = ST_A + NJ * 12, ST_F = ST_P + r4(NJ * 3), ST_VP = ST_F + KP, ST_X = ST_VP + r4(M), ST_XJ = ST_X + r4(M),
              ST_R = ST_XJ + r4(M), ST_FLOATS = ST_R + r4(M);
static_assert(ST_F % 4 == 0 && ST_FLOATS % 4 == 0, "16-byte slabs");

// The workgroup's LDS, carved from one dynamic array; K = skinning entries per vertex (nz, or 55); NS = FK states
// (lm_refine: the current pose's and the candidate's; the keypoint loss: one, and no lm_dev.h slabs behind J).
struct Lds {
    float *st0;                            // the NS FK states, ST_FLOATS apart
    __device__ float* state(int i) const { return st0 + i * ST_FLOATS; }
    float *G, *Jr;                         // G_j (55,12), the rest joints (55,3): chain scratch
    float *TR, *dR, *om;                   // linearisation: T.R per vertex (17,9), dR (22,3,9), omega (22,3,3)
    float *tgt, *rw, *ow;                  // rel(kps) (51), the row weights (51), the robust (IRLS) row weights (51)
    float *th, *th0, *thp, *cand, *d0, *dp;   // poses (66 each): current, prior, previous, candidate, th - th0, th - thp
    float *beta, *c;                       // betas (32), [0] a cost
    int *pv, *ancm;                        // vertex ids (17), the 22 low bits of anc (55)
    int *csel, *cslot;                     // per column: its joint, its vertex slot or -1 (the kernel arguments' tables)
    int *ek, *em;                          // per (vertex slot, entry): joint, its ancestor bits
    float *ew;                             //                          weight
    float *J;                              // (51,66)
    float *lm;                             // lm_dev.h's slabs (lm_refine only)
    __device__ Lds(float* p, int K, int NS = 2) {
        auto take = [&p](int n) { float* q = p; p += r4(n); return q; };
        st0 = take(NS * ST_FLOATS);
        G = take(NJ * 12); Jr = take(NJ * 3);
        TR = take(NC * 9); dR = take(ND * 27); om = take(ND * 9);
        tgt = take(M); rw = take(M); ow = take(M);
        th = take(N); th0 = take(N); thp = take(N); cand = take(N); d0 = take(N); dp = take(N);
        beta = take(32); c = take(4);
        pv = reinterpret_cast<int*>(take(NC)); ancm = reinterpret_cast<int*>(take(NJ));
        csel = reinterpret_cast<int*>(take(NC)); cslot = reinterpret_cast<int*>(take(NC));
        ek = reinterpret_cast<int*>(take(NC * K)); em = reinterpret_cast<int*>(take(NC * K));
        ew = take(NC * K);
        J = take(M * N);
        lm = p;
    }
};
// floats of LDS without lm_dev.h's slabs
__host__ __device__ constexpr size_t lds_frame_floats(int K, int NS) {
    return (size_t)NS * ST_FLOATS + r4(NJ * 12) + r4(NJ * 3) + r4(NC * 9) + r4(ND * 27) + r4(ND * 9) + 3 * r4(M) + 6 * r4(N) + 32 + 4 +
           3 * r4(NC) + r4(NJ) + 3 * (size_t)r4(NC * K) + r4(M * N);
}
__host__ __device__ constexpr size_t lds_floats(int K) { return lds_frame_floats(K, 2) + lm_lds_floats(N); }
static_assert(lds_floats(55) * 4 <= 64 * 1024, "the dense table form must fit the default LDS limit");

// the lane's value summed over the wave by a fixed butterfly: the same bits in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// neither NaN nor Inf, from the bits (no floating-point compile option can fold the test away)
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// The frame's constants into LDS, by the whole workgroup: poses, prior, prev (66 each; the last two or null) and kps
// (17,3) are the frame's own rows; f is its row of betas and joint_w; tie: thp = prev. Also thread j's tree depth
// and parent (-1 past the joints), and the feature tail of the NS states. Ends on a barrier.
// conf (17, or null): a stream's confidences of this frame; keypoint k then weighs conf[k] * joint_w[k], and nothing
// does where conf[11] or conf[12] is 0. skip (TIK_REFINE_SKIP_NONFINITE; refine._frame_weights' rule): a keypoint
// with a non-finite component weighs 0 and its target is taken as 0, and without both of columns 11 and 12 every
// weight of the frame is 0. With conf null and skip false: the arithmetic without them.
__device__ __forceinline__ void frame_setup(const LmRefineArgs& a, const Lds& s, const float* poses, const float* prior, const float* prev,
                                            bool tie, const float* kps, const float* conf, bool skip, size_t f, int K, int NS, int& dj,
                                            int& par) {
    const int tid = threadIdx.x;
    if (tid < N) {
        const float t = poses[tid];
        s.th[tid] = t;
        s.th0[tid] = prior ? prior[tid] : t;
        s.thp[tid] = tie ? prev[tid] : 0.f;
    }
    if (tid < M) {
        const int c = tid % 3, k = tid / 3;
        float x = kps[tid], ha = kps[33 + c], hb = kps[36 + c];
        float w = a.joint_w ? a.joint_w[f * a.joint_w_ld + k] : 1.f;
        if (conf) w = (conf[11] == 0.f || conf[12] == 0.f) ? 0.f : conf[k] * w;
        if (skip) {
            const bool seen = finite_bits(kps[3 * k]) && finite_bits(kps[3 * k + 1]) && finite_bits(kps[3 * k + 2]);
            const bool sa = finite_bits(kps[33]) && finite_bits(kps[34]) && finite_bits(kps[35]);
            const bool sb = finite_bits(kps[36]) && finite_bits(kps[37]) && finite_bits(kps[38]);
            x = seen ? x : 0.f; ha = sa ? ha : 0.f; hb = sb ? hb : 0.f;
            w = (seen && sa && sb) ? w : 0.f;
        }
        s.tgt[tid] = x - 0.5f * (ha + hb);
        s.rw[tid] = w;
    }
    if (tid < 32) s.beta[tid] = (a.betas && tid < a.nb) ? a.betas[f * a.betas_ld + tid] : 0.f;
    if (tid == 64) {   // the selection out of the kernel arguments by constant indices (scalar loads, no private copy)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int j = a.sel[c], sl = a.slot[c];
            s.csel[c] = j;
            s.cslot[c] = sl;
            if (sl >= 0) s.pv[sl] = a.pick_v[(j - 55) * 3];
        }
    }
    if (tid >= 128 && tid < 128 + NJ) s.ancm[tid - 128] = (int)(a.anc[tid - 128] & 0x3fffffull);
    dj = -1; par = -1;
    if (tid < NJ) {
        dj = a.depth[tid];
        par = a.parents[tid];
    }
    __syncthreads();
    for (int idx = tid; idx < a.nv * K; idx += LM_T) {   // fk_dev.h's entry walk, both table forms
        const int i = idx / K, n = idx - i * K;
        const SkinEntry e = skin_entry<false>(a, s.pv[i], n);
        s.ek[idx] = e.k;
        s.ew[idx] = e.w;
        s.em[idx] = s.ancm[e.k];
    }
    if (tid < NJ * 3) {   // the rest joints J = jt + jd . betas
        float v = a.jt[tid];
        const float* d = a.jd + (size_t)tid * a.ns;
        for (int l = 0; l < a.nb; ++l) v = fmaf(d[l], s.beta[l], v);
        s.Jr[tid] = v;
    }
    for (int k = SD0 + tid; k < KP; k += LM_T) {   // the feature tail [betas | expression (zero) | 1 | 0 ..] of every state
        const int l = k - SD0;
        const float f0 = l < a.nb ? s.beta[l] : (l == a.ns ? 1.f : 0.f);
        for (int i = 0; i < NS; ++i) s.state(i)[ST_F + k] = f0;
    }
    __syncthreads();
}

// FK of pose th (66, LDS) into state S. dj, par: thread j's tree depth and parent (-1 past the joints).
__device__ __forceinline__ void fk_eval(const LmRefineArgs& a, const Lds& s, float* S, const float* th, int dj, int par, int K) {
    const int tid = threadIdx.x;
    float* F = S + ST_F;
    float R[9];
    if (tid < NJ) {
        const int j = tid;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (j < ND ? th[3 * j + c] : 0.f) + a.pose_mean[3 * j + c];
        rodrigues_smplx(v[0], v[1], v[2], R);
        if (j > 0)
#pragma unroll
            for (int k = 0; k < 9; ++k) F[9 * (j - 1) + k] = R[k] - ((k % 4) == 0 ? 1.f : 0.f);
    }
    // the chain, one tree level at a time (fk_chain_kernel's recursion, G_parent from the level before)
    for (int d = 0; d <= a.maxdepth; ++d) {
        if (dj == d) {
            const int j = tid;
            float g[12];
            if (par < 0) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    g[4 * r] = R[3 * r]; g[4 * r + 1] = R[3 * r + 1]; g[4 * r + 2] = R[3 * r + 2]; g[4 * r + 3] = s.Jr[3 * j + r];
                }
            } else {
                const float* P = s.G + 12 * par;
                const float t0 = s.Jr[3 * j] - s.Jr[3 * par], t1 = s.Jr[3 * j + 1] - s.Jr[3 * par + 1], t2 = s.Jr[3 * j + 2] - s.Jr[3 * par + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[4 * r + c] = fmaf(P[4 * r + 2], R[6 + c], fmaf(P[4 * r + 1], R[3 + c], P[4 * r] * R[c]));
                    g[4 * r + 3] = fmaf(P[4 * r], t0, fmaf(P[4 * r + 1], t1, fmaf(P[4 * r + 2], t2, P[4 * r + 3])));
                }
            }
#pragma unroll
            for (int e = 0; e < 12; ++e) s.G[12 * j + e] = g[e];
        }
        __syncthreads();   // level d, and at d = 0 the feature rows, are in LDS
    }
    // A_j = [G_j.R | G_j.t - G_j.R J_j] and the posed joint
    if (tid < NJ) {
        const int j = tid;
        const float* g = s.G + 12 * j;
        const float J0 = s.Jr[3 * j], J1 = s.Jr[3 * j + 1], J2 = s.Jr[3 * j + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            S[ST_A + 12 * j + 4 * r] = g[4 * r]; S[ST_A + 12 * j + 4 * r + 1] = g[4 * r + 1]; S[ST_A + 12 * j + 4 * r + 2] = g[4 * r + 2];
            S[ST_A + 12 * j + 4 * r + 3] = g[4 * r + 3] - fmaf(g[4 * r + 2], J2, fmaf(g[4 * r + 1], J1, g[4 * r] * J0));
            S[ST_P + 3 * j + r] = g[4 * r + 3];
        }
    }
    // posed blend position of every vertex keypoint: vp[c] = feat . P^T row 3 v + c; lane = 8 consecutive k
    {
        const int lane = tid & 63, wv = tid >> 6;
        const f32x4 f0 = *reinterpret_cast<const f32x4*>(F + 8 * lane), f1 = *reinterpret_cast<const f32x4*>(F + 8 * lane + 4);
        for (int d = wv; d < 3 * a.nv; d += LM_T / 64) {
            const int i = d / 3, c = d - 3 * i;
            const float* pr = a.PT + ((size_t)s.pv[i] * 3 + c) * KP + 8 * lane;
            const f32x4 p0 = *reinterpret_cast<const f32x4*>(pr), p1 = *reinterpret_cast<const f32x4*>(pr + 4);
            float acc = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(f0[e], p0[e], acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(f1[e], p1[e], acc);
            acc = wave_sum(acc);
            if (lane == 0) S[ST_VP + d] = acc;
        }
    }
    __syncthreads();
    // skinning: thread (vertex slot i, row q): T row = sum_n w_n A_k(n) row, entries in table order; x = T (vp, 1)
    if (tid < 3 * a.nv) {
        const int i = tid / 3, q = tid - 3 * i;
        float T[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < K; ++n) {
            const float w = s.ew[i * K + n];
            const float* r = S + ST_A + 12 * s.ek[i * K + n] + 4 * q;
#pragma unroll
            for (int e = 0; e < 4; ++e) T[e] = fmaf(w, r[e], T[e]);
        }
        S[ST_X + tid] = row_affine(f32x4{T[0], T[1], T[2], T[3]}, S + ST_VP + 3 * i);
    }
    __syncthreads();
    if (tid < M) {
        const int sc = tid / 3, c = tid - 3 * sc;
        const int sl = s.cslot[sc];
        S[ST_XJ + tid] = sl < 0 ? S[ST_P + 3 * s.csel[sc] + c] : S[ST_X + 3 * sl + c];
    }
    __syncthreads();
    if (tid < M) {
        const int c = tid % 3;
        S[ST_R + tid] = (S[ST_XJ + tid] - 0.5f * (S[ST_XJ + 33 + c] + S[ST_XJ + 36 + c])) - s.tgt[tid];
    }
    __syncthreads();
}

// J (51,66) of state S at pose th, rows root-relative, into s.J
__device__ __forceinline__ void linearize(const LmRefineArgs& a, const Lds& s, const float* S, const float* th, int par, int K) {
    const int tid = threadIdx.x;
    if (tid < ND) {   // the derivative of rodrigues_smplx as written and omega = axial(G_parent.R dR G_j.R^T), as fk_jac_pre_kernel
        const int j = tid;
        RodDeriv rd;
        rodrigues_deriv_setup(th[3 * j] + a.pose_mean[3 * j], th[3 * j + 1] + a.pose_mean[3 * j + 1], th[3 * j + 2] + a.pose_mean[3 * j + 2], rd);
        float Gp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, Gj[9];
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Gj[3 * q + c] = S[ST_A + 12 * j + 4 * q + c];
                if (par >= 0) Gp[3 * q + c] = S[ST_A + 12 * par + 4 * q + c];
            }
        auto axis = [&](auto AX) __attribute__((always_inline)) {
            constexpr int ax = decltype(AX)::value;
            float dR[9], om[3];
            rodrigues_deriv_axis<ax>(rd, dR);
            rodrigues_omega(Gp, dR, Gj, om);
#pragma unroll
            for (int m = 0; m < 9; ++m) s.dR[(3 * j + ax) * 9 + m] = dR[m];
#pragma unroll
            for (int c = 0; c < 3; ++c) s.om[(3 * j + ax) * 3 + c] = om[c];
        };
        axis(std::integral_constant<int, 0>{});
        axis(std::integral_constant<int, 1>{});
        axis(std::integral_constant<int, 2>{});
    } else if (tid >= 64 && tid - 64 < 9 * a.nv) {   // T.R = sum_n w_n A_k(n).R of every vertex keypoint
        const int i = (tid - 64) / 9, e = (tid - 64) - 9 * i, q = e / 3, c = e - 3 * q;
        float t = 0.f;
        for (int n = 0; n < K; ++n) t = fmaf(s.ew[i * K + n], S[ST_A + 12 * s.ek[i * K + n] + 4 * q + c], t);
        s.TR[9 * i + e] = t;
    }
    __syncthreads();
    for (int idx = tid; idx < NC * ND; idx += LM_T) {
        const int sc = idx / ND, j = idx - sc * ND;
        const int sl = s.cslot[sc];
        const float* Pj = S + ST_P + 3 * j;
        const float* om = s.om + 9 * j;
        float o[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = 0.f;
        if (sl < 0) {   // a chain joint turns about every strict ancestor's posed joint
            const int jn = s.csel[sc];
            if (((s.ancm[jn] >> j) & 1) && j != jn) {
                const float D[3] = {S[ST_P + 3 * jn] - Pj[0], S[ST_P + 3 * jn + 1] - Pj[1], S[ST_P + 3 * jn + 2] - Pj[2]};
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const float w0 = om[3 * ax], w1 = om[3 * ax + 1], w2 = om[3 * ax + 2];
                    o[ax] = w1 * D[2] - w2 * D[1];
                    o[3 + ax] = w2 * D[0] - w0 * D[2];
                    o[6 + ax] = w0 * D[1] - w1 * D[0];
                }
            }
        } else {        // a vertex: omega x (S - sw P_j) + T.R u, the sums over the entries below dof j
            const float* vp = S + ST_VP + 3 * sl;
            float Sm[3] = {0.f, 0.f, 0.f}, sw = 0.f;
            for (int n = 0; n < K; ++n) {
                if ((s.em[sl * K + n] >> j) & 1) {
                    const float w = s.ew[sl * K + n];
                    const float* A = S + ST_A + 12 * s.ek[sl * K + n];
#pragma unroll
                    for (int c = 0; c < 3; ++c) Sm[c] = fmaf(w, row_affine(f32x4{A[4 * c], A[4 * c + 1], A[4 * c + 2], A[4 * c + 3]}, vp), Sm[c]);
                    sw += w;
                }
            }
            float D[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) D[c] = fmaf(-sw, Pj[c], Sm[c]);
            const float* pd = a.PT + (size_t)s.pv[sl] * 3 * KP + 9 * (j > 0 ? j - 1 : 0);   // read for j >= 1 only
            const float* TR = s.TR + 9 * sl;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float w0 = om[3 * ax], w1 = om[3 * ax + 1], w2 = om[3 * ax + 2];
                float t[3] = {w1 * D[2] - w2 * D[1], w2 * D[0] - w0 * D[2], w0 * D[1] - w1 * D[0]};
                if (j >= 1) {
                    const float* dR = s.dR + (3 * j + ax) * 9;
                    float u3[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int m = 0; m < 9; ++m)
#pragma unroll
                        for (int c = 0; c < 3; ++c) u3[c] = fmaf(dR[m], pd[c * KP + m], u3[c]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[c] += row_linear(TR[3 * c], TR[3 * c + 1], TR[3 * c + 2], u3[0], u3[1], u3[2]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * c + ax] = t[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) s.J[(3 * sc + c) * N + 3 * j + ax] = o[3 * c + ax];
    }
    __syncthreads();
    if (tid < 3 * N) {   // rel on the rows: thread = (component c, unknown q), every column of its own (c, q)
        const int c = tid / N, q = tid - c * N;
        const float m = 0.5f * (s.J[(33 + c) * N + q] + s.J[(36 + c) * N + q]);
        for (int sc = 0; sc < NC; ++sc) s.J[(3 * sc + c) * N + q] -= m;
    }
    __syncthreads();
}

// sum_k w_k |r_k|^2 of state S, for wave 0 (tid < 64): lane k's term, a fixed butterfly, the same bits in every lane
__device__ __forceinline__ float weighted_sq(const Lds& s, const float* S) {
    const int tid = threadIdx.x;
    float p = 0.f;
    if (tid < NC) {
        const float* r = S + ST_R + 3 * tid;
        p = s.rw[3 * tid] * fmaf(r[2], r[2], fmaf(r[1], r[1], r[0] * r[0]));
    }
    return wave_sum(p);
}

// Geman-McClure on s = |r_k|^2 with sig2 = sigma^2: rho(s) = sig2 s / (sig2 + s), rho'(s) = (sig2 / (sig2 + s))^2
__device__ __forceinline__ float sq_norm3(const float* r) { return fmaf(r[2], r[2], fmaf(r[1], r[1], r[0] * r[0])); }
// w_k rho'(s_k) of keypoint k of state S: the IRLS weight of its three rows
__device__ __forceinline__ float robust_weight(const Lds& s, const float* S, int k, float sig2) {
    const float t = sig2 / (sig2 + sq_norm3(S + ST_R + 3 * k));
    return s.rw[3 * k] * (t * t);
}
// sum_k w_k rho(|r_k|^2) of state S, as weighted_sq
__device__ __forceinline__ float weighted_rho(const Lds& s, const float* S, float sig2) {
    const int tid = threadIdx.x;
    float p = 0.f;
    if (tid < NC) {
        const float q = sq_norm3(S + ST_R + 3 * tid);
        p = s.rw[3 * tid] * (sig2 * q / (sig2 + q));
    }
    return wave_sum(p);
}

}  // namespace lmr
}  // namespace tik
