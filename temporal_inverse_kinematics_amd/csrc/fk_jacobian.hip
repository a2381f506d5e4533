// fk_jacobian.hip — d(selected SMPL-X joints) / d(pose) without the mesh (tik_fk_joints_jacobian).
//
// fk_chain_kernel (fk.hip, unchanged) leaves the pose feature (B,512), the
// transforms A_j (55,B,12) and the 55 chain joints. With R_j = rodrigues_smplx
// (theta_j + pose_mean_j), G_j = G_parent [R_j | J_j - J_parent] and
// A_j = [G_j.R | G_j.t - G_j.R J_j], a change of theta_{j,a} turns everything
// below joint j about the posed joint P_j with the world-frame angular velocity
//   omega_{j,a} = axial(G_parent.R (dR_j/dtheta_a) G_j.R^T)
// (A_j.R is G_j.R, so both factors are already in the workspace), and moves
// the posed blend shapes by dR_j/dtheta_a . posedirs:
//   chain joint k:  omega x (P_k - P_j)                       j a strict ancestor of k, else exactly 0
//   vertex v:       omega x (S - sw P_j) + T.R u              S  = sum_k [j anc-or-self k] w_k A_k(vp)
//                                                             sw = sum_k [j anc-or-self k] w_k
//                                                             T.R = sum_k w_k A_k.R
//                                                             u_c = sum_m dR[m] posedirs[9 (j-1) + m][3 v + c]   (j >= 1)
//   landmark:       the barycentric sum of its three vertices
//
// fk_jac_pre_kernel, lane = body, one workgroup row per dof joint: dR_a (27
// values) and omega_a (9 values) into the dof-major workspace jw, so that the
// main kernel's lane = body reads are coalesced. dR is the derivative of
// rodrigues_smplx as written: R = I + A K(v) + B K(v)^2 with A = sin t / t,
// B = (1 - cos t) / t^2, t = |v + 1e-8|; A, B, A'/t and B'/t by their series
// below t = 0.5 (the fp32 closed forms cancel there, and inference passes exact
// zeros for the hands, jaw and eyes).
//
// fk_jacobian_kernel, lane = body (a tile of FKJ_TB = 64 bodies per workgroup),
// wave = one output column (selected joint). A vertex's per-joint positions
// A_k(vp) pass through a wave-private LDS slab [k][3][lane] (no barrier: a wave
// reads only what it wrote); the ancestor test is a wave-uniform bit of the
// 55-entry mask table. Every sum has a fixed order (k ascending over the blend
// feature, the skinning entries in table order, the dofs in list order) and
// a lane works for its own body only, so a body's rows are the same bits for
// any B, any place in the batch and any selection around the column. A body's
// row is written in runs of 3 floats, contiguous over 3 n_dof. No atomics, no
// waiting between workgroups, plain vector stores. fk_dev.h (shared with fk_joints.hip and fk_shape.hip) holds
// the column of a wave, the decode of a static joint's vertices, the rows of A_k and the two row products; the
// blend dot product stays here (one 512-k chain, not fk_joints_kernel's eight chunks: other bits).
#include <type_traits>

#include "fk_dev.h"

namespace tik {
using namespace fkd;   // TB bodies per tile, KP the feature row length
constexpr int PD = FKJAC_PER_DOF;

__global__ __launch_bounds__(64) void fk_jac_pre_kernel(FkJacArgs a) {
    int b, d;
    if (!pre_body(a, b, d)) return;   // no barrier below
    const int j = a.dof[d];
    const float* pz = a.pose + ((size_t)b * 55 + j) * 3;
    RodDeriv rd;   // fk_dev.h: the coefficients and K(v), K(v)^2, once for the three axes
    rodrigues_deriv_setup(pz[0] + a.pose_mean[j * 3], pz[1] + a.pose_mean[j * 3 + 1], pz[2] + a.pose_mean[j * 3 + 2], rd);
    float Gp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, Gj[9];
    auto rot = [&](int k, float* G) __attribute__((always_inline)) {   // the 3x3 part of A_k
        const f32x4* r = ak_rows(a, k, b);
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[3 * q + c] = r[q][c];
    };
    const int p = a.parents[j];
    rot(j, Gj);
    if (p >= 0) rot(p, Gp);
    float* o = a.jw + (size_t)d * PD * a.B + b;
    auto axis = [&](auto AX) __attribute__((always_inline)) {
        constexpr int ax = decltype(AX)::value;
        float dR[9], om[3];
        rodrigues_deriv_axis<ax>(rd, dR);
#pragma unroll
        for (int m = 0; m < 9; ++m) o[(size_t)(9 * ax + m) * a.B] = dR[m];
        rodrigues_omega(Gp, dR, Gj, om);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)(27 + 3 * ax + c) * a.B] = om[c];
    };
    axis(std::integral_constant<int, 0>{});
    axis(std::integral_constant<int, 1>{});
    axis(std::integral_constant<int, 2>{});
}

// MAXK: skinning entries per vertex at most (16: the pairs; 55: the dense WT rows); JW: columns (waves) per workgroup
template <int MAXK, int JW>
__global__ __launch_bounds__(64 * JW) void fk_jacobian_kernel(FkJacArgs a) {
    __shared__ float sX[JW][MAXK * 3 * 64];
    Column col;
    if (!column(a, JW, col)) return;   // no barrier in this kernel
    const int lane = col.lane, b = col.b, s = col.s, jn = col.jn;
    const size_t B = a.B;
    const int nd3 = 3 * a.n_dof;
    float* row = a.jac + ((size_t)b * 3 * a.n_sel + 3 * s) * nd3;   // rows 3 s .. 3 s + 2 of this body
    const float* jc = a.jchain + (size_t)b * 55 * 3;
    float tr[3] = {0.f, 0.f, 0.f};
    if (a.transl)
        for (int c = 0; c < 3; ++c) tr[c] = a.transl[(size_t)b * 3 + c];

    if (jn < 55) {   // a chain joint
        const unsigned long long am = a.anc[jn];
        const float Pk[3] = {jc[3 * jn], jc[3 * jn + 1], jc[3 * jn + 2]};
        for (int d = 0; d < a.n_dof; ++d) {
            const int j = a.dof[d];
            float o[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = 0.f;
            if (((am >> j) & 1ull) && j != jn) {
                const float D[3] = {Pk[0] - jc[3 * j], Pk[1] - jc[3 * j + 1], Pk[2] - jc[3 * j + 2]};
                const float* w = a.jw + ((size_t)d * PD + 27) * B + b;
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const float w0 = w[(size_t)(3 * ax) * B], w1 = w[(size_t)(3 * ax + 1) * B], w2 = w[(size_t)(3 * ax + 2) * B];
                    o[ax] = w1 * D[2] - w2 * D[1];
                    o[3 + ax] = w2 * D[0] - w0 * D[2];
                    o[6 + ax] = w0 * D[1] - w1 * D[0];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) row[(size_t)c * nd3 + 3 * d + ax] = o[3 * c + ax];
        }
        return;
    }

    // a vertex joint (one vertex) or a static landmark (three)
    const int npick = pick_count(a, jn), K = skin_count(a);
    float* X = sX[col.wv];
    for (int i = 0; i < npick; ++i) {
        const Pick pk = pick(a, jn, i);
        const int v = pk.v;
        // posed blend position vp = feat . P^T rows 3 v .. 3 v + 2, k ascending
        float vp[3] = {0.f, 0.f, 0.f};
        {
            const float* f = a.feat + (size_t)b * KP;
            const float* pr = a.PT + (size_t)v * 3 * KP;
            for (int k4 = 0; k4 < KP; k4 += 4) {
                const f32x4 f4 = *reinterpret_cast<const f32x4*>(f + k4);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x4 p4 = *reinterpret_cast<const f32x4*>(pr + c * KP + k4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) vp[c] = fmaf(f4[e], p4[e], vp[c]);
                }
            }
        }
        // fk_dev.h's skin_entry<false> and ak_rows, spelled out: through the helpers the compiler contracts the cross
        // products below another way (other bits)
        auto entry = [&](int n) __attribute__((always_inline)) -> SkinEntry {
            if (a.nz > 0) {
                const int2 e = a.nzw[(size_t)v * a.nz + n];
                return {e.x, __builtin_bit_cast(float, e.y)};
            }
            return {n, a.WT[(size_t)v * 64 + n]};
        };
        // x_n = A_k(vp) into the slab, T.R = sum_n w_n A_k.R
        float TR[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) TR[e] = 0.f;
        for (int n = 0; n < K; ++n) {
            const SkinEntry e = entry(n);
            const f32x4* r = reinterpret_cast<const f32x4*>(a.ajt + ((size_t)e.k * B + b) * 12);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const f32x4 t = r[q];
                X[(n * 3 + q) * 64 + lane] = row_affine(t, vp);
#pragma unroll
                for (int c = 0; c < 3; ++c) TR[3 * q + c] = fmaf(e.w, t[c], TR[3 * q + c]);
            }
        }
        for (int d = 0; d < a.n_dof; ++d) {
            const int j = a.dof[d];
            float S[3] = {0.f, 0.f, 0.f}, sw = 0.f;
            for (int n = 0; n < K; ++n) {
                const SkinEntry e = entry(n);
                if ((a.anc[e.k] >> j) & 1ull) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) S[c] = fmaf(e.w, X[(n * 3 + c) * 64 + lane], S[c]);
                    sw += e.w;
                }
            }
            // the posed joint without the translation, as A_k(vp) is
            float D[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) D[c] = fmaf(-sw, jc[3 * j + c] - tr[c], S[c]);
            const float* w = a.jw + (size_t)d * PD * B + b;
            const float* pd = a.PT + (size_t)v * 3 * KP + 9 * (j > 0 ? j - 1 : 0);   // read for j >= 1 only
            float o[9];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float w0 = w[(size_t)(27 + 3 * ax) * B], w1 = w[(size_t)(28 + 3 * ax) * B], w2 = w[(size_t)(29 + 3 * ax) * B];
                float t[3] = {w1 * D[2] - w2 * D[1], w2 * D[0] - w0 * D[2], w0 * D[1] - w1 * D[0]};
                if (j >= 1) {
                    float u3[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int m = 0; m < 9; ++m) {
                        const float dr = w[(size_t)(9 * ax + m) * B];
#pragma unroll
                        for (int c = 0; c < 3; ++c) u3[c] = fmaf(dr, pd[c * KP + m], u3[c]);
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        t[c] += row_linear(TR[3 * c], TR[3 * c + 1], TR[3 * c + 2], u3[0], u3[1], u3[2]);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * c + ax] = pk.bw * t[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    float* q = row + (size_t)c * nd3 + 3 * d + ax;
                    *q = i == 0 ? o[3 * c + ax] : *q + o[3 * c + ax];   // a landmark: its own earlier store
                }
        }
    }
}

hipError_t launch_fk_jacobian(const FkJacArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.n_sel <= 0 || a.n_sel > FKJ_MAX_SEL || a.n_dof <= 0 || a.n_dof > 55 || !a.jac || !a.jw || !a.anc || !nz_ok(a))
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    const unsigned tiles = (a.B + TB - 1) / TB;
    hipLaunchKernelGGL(fk_jac_pre_kernel, dim3(tiles, a.n_dof), dim3(64), 0, st, a);
    if (a.nz > 0) {
        constexpr int JW = 4;
        hipLaunchKernelGGL((fk_jacobian_kernel<16, JW>), dim3(tiles, (a.n_sel + JW - 1) / JW), dim3(64 * JW), 0, st, a);
    } else {
        hipLaunchKernelGGL((fk_jacobian_kernel<55, 1>), dim3(tiles, a.n_sel), dim3(64), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace tik
