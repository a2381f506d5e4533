// fk_dev.h — the device pieces shared by the mesh-free FK kernels (fk_joints.hip, fk_jacobian.hip,
// fk_shape.hip, lm_refine.hip), on the selection base FkSelArgs (fk.h). All inlined; none holds a sum of its own, so the order
// of every sum stays where the kernels' header comments state it. Also rodrigues_smplx (fk.hip's chain and lm_refine.hip)
// and its derivative (fk_jac_pre_kernel and lm_refine.hip): one spelling of each, the same instructions as before the move.
// Not here, on purpose: the blend dot product v_posed = feat . P^T. fk_joints_kernel adds eight 64-k partial sums
// (what lets its two mappings agree), fk_jacobian_kernel runs one 512-k chain: different bits, both pinned by tests.
#pragma once
#include "dev_common.h"
#include "fk.h"

namespace tik {
namespace fkd {

constexpr int TB = FKJ_TB, KP = FK_KP, SD0 = FK_SD0;   // fk.h: tile, feature row length, first shape column
// the launchers' test of nz: the number of nzw pairs per vertex, or 0 for the dense WT rows
inline bool nz_ok(const FkSelArgs& a) { return (a.nz == 0 || a.nz == 4 || a.nz == 8 || a.nz == 16) && (!a.nz || a.nzw); }

// The skinning entries of vertex v in table order: the nz pairs of fk_skin_sparse_kernel (W > 2^-30, padding
// {0, 0.f} included), or the 55 weights of the dense WT row. UNIFORM: v is wave-uniform, so is its table row,
// and the pair is made scalar (fk_shape.hip: k then indexes jd by scalar loads); else the pair is as loaded.
struct SkinEntry { int k; float w; };   // joint, W[v][k]
__device__ __forceinline__ int skin_count(const FkSelArgs& a) { return a.nz > 0 ? a.nz : 55; }
template <bool UNIFORM>
__device__ __forceinline__ SkinEntry skin_entry(const FkSelArgs& a, int v, int n) {
    if (a.nz <= 0) return {n, a.WT[(size_t)v * 64 + n]};
    const int2 e = a.nzw[(size_t)v * a.nz + n];
    if (UNIFORM) return {__builtin_amdgcn_readfirstlane(e.x), __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(e.y))};
    return {e.x, __builtin_bit_cast(float, e.y)};
}

// A static joint jn >= 55 is one vertex (a vertex joint) or three (a landmark); vertex i (the same for every lane,
// made scalar) and its barycentric weight (a vertex joint: 1, 0, 0).
struct Pick { int v; float bw; };
__device__ __forceinline__ int pick_count(const FkSelArgs& a, int jn) { return jn - 55 < a.nextra ? 1 : 3; }
__device__ __forceinline__ Pick pick(const FkSelArgs& a, int jn, int i) {
    return {__builtin_amdgcn_readfirstlane(a.pick_v[(jn - 55) * 3 + i]), a.pick_w[(jn - 55) * 3 + i]};
}

// the three rows of A_k (3x4) of body b
__device__ __forceinline__ const f32x4* ak_rows(const FkSelArgs& a, int k, int b) {
    return reinterpret_cast<const f32x4*>(a.ajt + ((size_t)k * a.B + b) * 12);
}

// The row products. Two nestings, both pinned bit for bit: do not merge or reorder them.
// affine, row . (p, 1): the translation innermost; linear, row . d: the first term a plain product, innermost
__device__ __forceinline__ float row_affine(const f32x4 t, const float* p) {
    return fmaf(t[0], p[0], fmaf(t[1], p[1], fmaf(t[2], p[2], t[3])));
}
__device__ __forceinline__ float row_linear(float t0, float t1, float t2, float d0, float d1, float d2) {
    return fmaf(t2, d2, fmaf(t1, d1, t0 * d0));
}

// smplx lbs.batch_rodrigues: angle = ||v + 1e-8||, rot_dir = v / angle, R = I + sin K + (1 - cos) K K
// (fk_chain_kernel and lm_refine_kernel)
__device__ __forceinline__ void rodrigues_smplx(float x, float y, float z, float R[9]) {
    const float ax = x + 1e-8f, ay = y + 1e-8f, az = z + 1e-8f;
    const float ang = sqrtf(ax * ax + ay * ay + az * az);
    const float inv = 1.0f / ang;
    const float dx = x * inv, dy = y * inv, dz = z * inv;
    float s, c;
    sincosf(ang, &s, &c);
    const float oc = 1.0f - c;
    const float d2 = dx * dx + dy * dy + dz * dz;
    // K = [0,-dz,dy; dz,0,-dx; -dy,dx,0];  (K K)_ij = d_i d_j - delta_ij |d|^2
    R[0] = 1.f + oc * (dx * dx - d2);  R[1] = -s * dz + oc * dx * dy;      R[2] = s * dy + oc * dx * dz;
    R[3] = s * dz + oc * dx * dy;      R[4] = 1.f + oc * (dy * dy - d2);  R[5] = -s * dx + oc * dy * dz;
    R[6] = -s * dy + oc * dx * dz;     R[7] = s * dx + oc * dy * dz;      R[8] = 1.f + oc * (dz * dz - d2);
}

// The derivative of rodrigues_smplx as written, R = I + A K(v) + B K(v)^2 with A = sin t / t, B = (1 - cos t) / t^2,
// t = |v + 1e-8|: the coefficients A, B, A'/t, B'/t (by their series below t = 0.5, where the fp32 closed forms
// cancel), K(v) and K(v)^2 = v v^T - |v|^2 I, once per joint; then dR / dv_ax per axis
// (fk_jac_pre_kernel and lm_refine_kernel).
struct RodDeriv { float u[3], v[3], cA, cB, cAp, cBp, K[9], K2[9]; };
__device__ __forceinline__ void rodrigues_deriv_setup(float x, float y, float z, RodDeriv& d) {
    d.v[0] = x; d.v[1] = y; d.v[2] = z;
    d.u[0] = x + 1e-8f; d.u[1] = y + 1e-8f; d.u[2] = z + 1e-8f;
    const float t2 = d.u[0] * d.u[0] + d.u[1] * d.u[1] + d.u[2] * d.u[2];
    if (t2 < 0.25f) {
        d.cA = fmaf(t2, fmaf(t2, fmaf(t2, -1.f / 5040.f, 1.f / 120.f), -1.f / 6.f), 1.f);
        d.cB = fmaf(t2, fmaf(t2, fmaf(t2, -1.f / 40320.f, 1.f / 720.f), -1.f / 24.f), 0.5f);
        d.cAp = fmaf(t2, fmaf(t2, fmaf(t2, 1.f / 45360.f, -1.f / 840.f), 1.f / 30.f), -1.f / 3.f);
        d.cBp = fmaf(t2, fmaf(t2, fmaf(t2, 1.f / 453600.f, -1.f / 6720.f), 1.f / 180.f), -1.f / 12.f);
    } else {
        const float t = sqrtf(t2);
        float s, c;
        sincosf(t, &s, &c);
        d.cA = s / t;
        d.cB = (1.f - c) / t2;
        d.cAp = (t * c - s) / (t * t2);
        d.cBp = (t * s - 2.f * (1.f - c)) / (t2 * t2);
    }
    const float vv = x * x + y * y + z * z;
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d.K[3 * r + c] = K[3 * r + c];
            d.K2[3 * r + c] = d.v[r] * d.v[c] - (r == c ? vv : 0.f);
        }
}
// dR = A K(e) + A'/t u_a K(v) + B (e v^T + v e^T - 2 v_a I) + B'/t u_a K(v)^2; AX is a compile-time axis
template <int AX>
__device__ __forceinline__ void rodrigues_deriv_axis(const RodDeriv& d, float dR[9]) {
    const float ka = d.cAp * d.u[AX], kb = d.cBp * d.u[AX];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // K(e_ax)[r][c]: +1 at (ax+2, ax+1), -1 at (ax+1, ax+2) (indices mod 3)
            const float ke = (r == (AX + 2) % 3 && c == (AX + 1) % 3) ? 1.f : (r == (AX + 1) % 3 && c == (AX + 2) % 3) ? -1.f : 0.f;
            const float sy = (r == AX ? d.v[c] : 0.f) + (c == AX ? d.v[r] : 0.f) - (r == c ? 2.f * d.v[AX] : 0.f);
            dR[3 * r + c] = fmaf(kb, d.K2[3 * r + c], fmaf(d.cB, sy, fmaf(ka, d.K[3 * r + c], d.cA * ke)));
        }
}
// omega = axial(Gp dR Gj^T): the world-frame angular velocity of a unit change of that axis; Gp, Gj row-major 3x3
__device__ __forceinline__ void rodrigues_omega(const float* Gp, const float* dR, const float* Gj, float om[3]) {
    float M[9], W[9];   // M = Gp dR, W = M Gj^T
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            M[3 * r + c] = row_linear(Gp[3 * r], Gp[3 * r + 1], Gp[3 * r + 2], dR[c], dR[3 + c], dR[6 + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            W[3 * r + c] = row_linear(M[3 * r], M[3 * r + 1], M[3 * r + 2], Gj[3 * c], Gj[3 * c + 1], Gj[3 * c + 2]);
    om[0] = 0.5f * (W[7] - W[5]);
    om[1] = 0.5f * (W[2] - W[6]);
    om[2] = 0.5f * (W[3] - W[1]);
}

// The lane's body b and the wave's column s (joint jn) of a Jacobian kernel with jw waves per workgroup.
// -> false where there is no such column or body (the caller returns: those kernels have no barrier)
struct Column { int lane, wv, b, s, jn; };
__device__ __forceinline__ bool column(const FkSelArgs& a, int jw, Column& c) {
    c.lane = threadIdx.x & 63;
    c.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    c.b = blockIdx.x * TB + c.lane;
    c.s = blockIdx.y * jw + c.wv;
    if (c.s >= a.n_sel || c.b >= a.B) return false;
    c.jn = a.sel[c.s];
    return true;
}
// the same of a pre kernel (64 threads, one grid row per dof / beta). -> false past the batch
__device__ __forceinline__ bool pre_body(const FkSelArgs& a, int& b, int& row) {
    b = blockIdx.x * TB + threadIdx.x;
    row = blockIdx.y;
    return b < a.B;
}

}  // namespace fkd
}  // namespace tik
