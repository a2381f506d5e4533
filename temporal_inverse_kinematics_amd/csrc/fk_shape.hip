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
// no waiting between workgroups, plain vector stores. fk_dev.h (shared with fk_joints.hip, fk_jacobian.hip): the
// column of a wave, the skinning entries (here made scalar), a static joint's vertices, the rows of A_k, row_linear.
#include "fk_dev.h"

namespace tik {
using namespace fkd;   // TB bodies per tile, KP the feature row length, SD0 the first shape column
constexpr int MAXNB = FKS_MAX_NB;
constexpr int PB = FKS_PER_BETA;
constexpr int JW = 4;   // columns (waves) per workgroup

__global__ __launch_bounds__(64) void fk_shape_pre_kernel(FkShapeArgs a) {
    int b, i;
    if (!pre_body(a, b, i)) return;   // no barrier below
    const size_t B = a.B;
    float* o = a.sw + (size_t)i * PB * B + b;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * B] = a.jd[(size_t)c * a.ns + i];
    for (int k = 1; k < 55; ++k) {
        const int p = a.parents[k];
        const float* jk = a.jd + (size_t)k * 3 * a.ns + i;
        const float* jp = a.jd + (size_t)p * 3 * a.ns + i;
        const float d[3] = {jk[0] - jp[0], jk[a.ns] - jp[a.ns], jk[2 * a.ns] - jp[2 * a.ns]};
        const f32x4* r = ak_rows(a, p, b);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f32x4 t = r[c];
            o[(size_t)(3 * k + c) * B] = o[(size_t)(3 * p + c) * B] + row_linear(t[0], t[1], t[2], d[0], d[1], d[2]);
        }
    }
}

__global__ __launch_bounds__(64 * JW) void fk_shape_jacobian_kernel(FkShapeArgs a) {
    Column col;
    if (!column(a, JW, col)) return;   // no barrier in this kernel
    const int b = col.b, s = col.s, jn = col.jn;
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
    const int npick = pick_count(a, jn), K = skin_count(a);
    float acc[3 * MAXNB];
#pragma unroll
    for (int e = 0; e < 3 * MAXNB; ++e) acc[e] = 0.f;
    for (int q = 0; q < npick; ++q) {
        const Pick pk = pick(a, jn, q);
        const float* sd = a.PT + (size_t)pk.v * 3 * KP + SD0;
        for (int n = 0; n < K; ++n) {
            const SkinEntry e = skin_entry<true>(a, pk.v, n);   // the vertex is wave-uniform, so is its table row
            const float w = e.w * pk.bw;   // a vertex joint: x 1
            const f32x4* r = ak_rows(a, e.k, b);
            const f32x4 r0 = r[0], r1 = r[1], r2 = r[2];
            const float* jd = a.jd + (size_t)e.k * 3 * a.ns;
            const float* dp = a.sw + (size_t)3 * e.k * B + b;
#pragma unroll
            for (int i = 0; i < MAXNB; ++i) {
                if (i < nb) {
                    const float d0 = sd[i] - jd[i], d1 = sd[KP + i] - jd[a.ns + i], d2 = sd[2 * KP + i] - jd[2 * a.ns + i];
                    const float* p = dp + (size_t)i * PB * B;
                    const float u0 = row_linear(r0[0], r0[1], r0[2], d0, d1, d2) + p[0];
                    const float u1 = row_linear(r1[0], r1[1], r1[2], d0, d1, d2) + p[B];
                    const float u2 = row_linear(r2[0], r2[1], r2[2], d0, d1, d2) + p[2 * B];
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
        !a.ajt || !a.jd || !a.parents || !nz_ok(a))
        return hipErrorInvalidValue;
    (void)hipGetLastError();
    const unsigned tiles = (a.B + TB - 1) / TB;
    hipLaunchKernelGGL(fk_shape_pre_kernel, dim3(tiles, a.nb), dim3(64), 0, st, a);
    hipLaunchKernelGGL(fk_shape_jacobian_kernel, dim3(tiles, (a.n_sel + JW - 1) / JW), dim3(64 * JW), 0, st, a);
    return hipGetLastError();
}

}  // namespace tik
