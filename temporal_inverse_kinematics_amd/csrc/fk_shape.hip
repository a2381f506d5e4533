// fk_shape.hip — d(selected SMPL-X joints) / d(betas) without the mesh (tik_fk_joints_shape_jacobian).
//
// For a fixed pose the joints are affine in the betas: the rest joints are J_k = jt_k + jd_k beta,
// the shaped vertex is v_template + shapedirs beta + (pose blend shapes), and the skinning
// transforms' rotations do not see the shape. With R_k the world rotation of chain joint k (the 3x3
// part of A_k, which fk_chain_kernel (fk.hip, unchanged) leaves in ajt), jd[k][:, i] the regressed
// shape direction of joint k and sd_v[:, i] = shapedirs[v, :, i] (column 486 + i of P^T):
//   chain joint 0:  dP_0,i = jd[0][:, i]
//   chain joint k:  dP_k,i = dP_parent,i + R_parent (jd[k][:, i] - jd[parent][:, i])
//   vertex v:       dx_v,i = sum_n w_n (R_k (sd_v[:, i] - jd[k][:, i]) + dP_k,i)     (k, w_n) the vertex's skinning entries
//   landmark:       the barycentric sum of its three vertices
// The pose blend shapes, the translation, the betas and the expression do not enter: the result
// is a function of the pose alone, the same bits whatever those inputs are.
//
// fk_shape_pre_kernel, lane = body, one workgroup row per beta: dP of the 55 chain joints in
// ascending order (parents[k] < k, so a lane reads back what it stored itself) into the beta-major
// workspace sw, so that the main kernel's lane = body reads are coalesced.
// fk_shape_jacobian_kernel, lane = body (a tile of FKJ_TB = 64 bodies per workgroup), wave = one
// output column (selected joint), 3 nb accumulators per lane, no LDS and no barrier. The skinning
// entries run in table order (the nzw pairs, or the 55 dense WT rows under TIK_FK_SKIN=dense), a
// landmark's three vertices in order with the barycentric weight folded into the skinning weight
// (x 1 for a vertex joint), every term an fp32 FMA chain in that one order; a lane works for its
// own body only, so a body's rows are the same bits for any B, any place in the batch and any
// selection around the column. A body's rows 3 s .. 3 s + 2 are one run of 3 nb floats. No atomics,
// no waiting between workgroups, plain vector stores.
#include "fk.h"
#include "dev_common.h"

namespace tik {

namespace fkshape {
constexpr int TB = FKJ_TB;        // bodies per tile
constexpr int KP = 512;           // feature row length
constexpr int SD0 = 486;          // first shape column of a P^T row
constexpr int MAXNB = FKS_MAX_NB;
constexpr int PB = FKS_PER_BETA;
constexpr int JW = 4;             // columns (waves) per workgroup
}  // namespace fkshape

__global__ __launch_bounds__(64) void fk_shape_pre_kernel(FkShapeArgs a) {
    using namespace fkshape;
    const int b = blockIdx.x * TB + threadIdx.x;
    if (b >= a.B) return;   // no barrier below
    const int i = blockIdx.y;
    const size_t B = a.B;
    float* o = a.sw + (size_t)i * PB * B + b;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * B] = a.jd[(size_t)c * a.ns + i];
    for (int k = 1; k < 55; ++k) {
        const int p = a.parents[k];
        const float* jk = a.jd + (size_t)k * 3 * a.ns + i;
        const float* jp = a.jd + (size_t)p * 3 * a.ns + i;
        const float d[3] = {jk[0] - jp[0], jk[a.ns] - jp[a.ns], jk[2 * a.ns] - jp[2 * a.ns]};
        const f32x4* r = reinterpret_cast<const f32x4*>(a.ajt + ((size_t)p * B + b) * 12);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 t = r[c];
            const float rd = fmaf(t[2], d[2], fmaf(t[1], d[1], t[0] * d[0]));
            o[(size_t)(3 * k + c) * B] = o[(size_t)(3 * p + c) * B] + rd;
        }
    }
}

__global__ __launch_bounds__(64 * fkshape::JW) void fk_shape_jacobian_kernel(FkShapeArgs a) {
    using namespace fkshape;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x * TB + lane;
    const int s = blockIdx.y * JW + wv;
    if (s >= a.n_sel || b >= a.B) return;   // no barrier in this kernel
    const int jn = a.sel[s];
    const size_t B = a.B;
    const int nb = a.nb;
    float* row = a.jac + ((size_t)b * 3 * a.n_sel + 3 * s) * nb;   // rows 3 s .. 3 s + 2 of this body

    if (jn < 55) {   // a chain joint: its dP
        for (int i = 0; i < nb; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) row[(size_t)c * nb + i] = a.sw[((size_t)i * PB + 3 * jn + c) * B + b];
        return;
    }

    // a vertex joint (one vertex) or a static landmark (three)
    const int jj = jn - 55;
    const int npick = jj < a.nextra ? 1 : 3;
    const int K = a.nz > 0 ? a.nz : 55;   // skinning entries per vertex: the pairs, or the dense WT row
    float acc[3 * MAXNB];
#pragma unroll
    for (int e = 0; e < 3 * MAXNB; ++e) acc[e] = 0.f;
    for (int q = 0; q < npick; ++q) {
        const int v = __builtin_amdgcn_readfirstlane(a.pick_v[jj * 3 + q]);
        const float bw = a.pick_w[jj * 3 + q];
        const float* sd = a.PT + (size_t)v * 3 * KP + SD0;
        for (int n = 0; n < K; ++n) {
            int k;
            float w;
            if (a.nz > 0) {
                const int2 e = a.nzw[(size_t)v * a.nz + n];
                k = __builtin_amdgcn_readfirstlane(e.x);   // v is wave-uniform, so is its table row
                w = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(e.y));
            } else {
                k = n;
                w = a.WT[(size_t)v * 64 + n];
            }
            w *= bw;   // a vertex joint: x 1
            const f32x4* r = reinterpret_cast<const f32x4*>(a.ajt + ((size_t)k * B + b) * 12);
            const f32x4 r0 = r[0], r1 = r[1], r2 = r[2];
            const float* jd = a.jd + (size_t)k * 3 * a.ns;
            const float* dp = a.sw + (size_t)3 * k * B + b;
#pragma unroll
            for (int i = 0; i < MAXNB; ++i) {
                if (i < nb) {
                    const float d0 = sd[i] - jd[i], d1 = sd[KP + i] - jd[a.ns + i], d2 = sd[2 * KP + i] - jd[2 * a.ns + i];
                    const float* p = dp + (size_t)i * PB * B;
                    const float u0 = fmaf(r0[2], d2, fmaf(r0[1], d1, r0[0] * d0)) + p[0];
                    const float u1 = fmaf(r1[2], d2, fmaf(r1[1], d1, r1[0] * d0)) + p[B];
                    const float u2 = fmaf(r2[2], d2, fmaf(r2[1], d1, r2[0] * d0)) + p[2 * B];
                    acc[3 * i] = fmaf(w, u0, acc[3 * i]);
                    acc[3 * i + 1] = fmaf(w, u1, acc[3 * i + 1]);
                    acc[3 * i + 2] = fmaf(w, u2, acc[3 * i + 2]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXNB; ++i) {
        if (i < nb) {
#pragma unroll
            for (int c = 0; c < 3; ++c) row[(size_t)c * nb + i] = acc[3 * i + c];
        }
    }
}

hipError_t launch_fk_shape_jacobian(const FkShapeArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.n_sel <= 0 || a.n_sel > FKJ_MAX_SEL || a.nb <= 0 || a.nb > FKS_MAX_NB || a.ns < a.nb || !a.jac || !a.sw ||
        !a.ajt || !a.jd || !a.parents || (a.nz != 0 && a.nz != 4 && a.nz != 8 && a.nz != 16) || (a.nz && !a.nzw))
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    const unsigned tiles = (a.B + fkshape::TB - 1) / fkshape::TB;
    hipLaunchKernelGGL(fk_shape_pre_kernel, dim3(tiles, a.nb), dim3(64), 0, st, a);
    constexpr int JW = fkshape::JW;
    hipLaunchKernelGGL(fk_shape_jacobian_kernel, dim3(tiles, (a.n_sel + JW - 1) / JW), dim3(64 * JW), 0, st, a);
    return hipGetLastError();
}

}  // namespace tik
