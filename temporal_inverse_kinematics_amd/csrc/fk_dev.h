// fk_dev.h — the device pieces shared by the three mesh-free FK kernels (fk_joints.hip, fk_jacobian.hip,
// fk_shape.hip), on the selection base FkSelArgs (fk.h). All inlined; none holds a sum of its own, so the order
// of every sum stays where the kernels' header comments state it.
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
