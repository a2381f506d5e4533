// fk_joints.hip — the joints of the SMPL-X FK without the mesh (tik_fk_joints).
//
// fk_chain_kernel (fk.hip, unchanged) leaves the pose feature (B,512), the
// transforms A_j (55,B,12), the contour bin and the 55 chain joints. Every
// other joint is 1 or 3 vertices of the body; fk_joints_kernel evaluates just
// those (blend shapes, skinning, barycentric sum) in fp32 FMAs.
//
// Mapping: lane = body (a workgroup owns a tile of FKJ_TB = 64 bodies), wave
// = one output column (FKJ_JW = 8 columns per workgroup, taken with a stride
// of the grid's column count so that the contour columns, the slow ones, land
// in different workgroups). The tile's feature rows pass through LDS in
// chunks of 64 k, transposed (k-major, so lane b reads its own body's value
// with a conflict-free ds_read_b32), double buffered, one barrier per chunk.
// A static joint's vertices are the same for every lane: its P^T rows are
// wave-uniform and are read once per tile by scalar loads (an FMA takes the
// SGPR operand directly). A contour joint's vertices depend on the body's
// bin: each lane reads its own rows, 16 B at a time along k; lanes of one bin
// share their cache lines.
//
// Arithmetic order of a dot product: the 8 chunks of 64 k are summed each
// from zero, k ascending, and the 8 partial sums are added in chunk order.
// That is what lets a small launch (few body tiles x few columns, e.g. B = 1)
// use the other mapping, split: a workgroup per column, wave = chunk, the
// feature values straight from global memory, the partials combined through
// LDS by wave 0 in the same order. Both mappings and both regimes give the
// same bits, so a result does not depend on B, on the body's place in the
// batch, or on what else is selected. No atomics, no waiting between
// workgroups. fk_dev.h (shared with fk_jacobian.hip, fk_shape.hip): the walk over a vertex's skinning entries, a
// static joint's vertices, the rows of A_k, the affine row product; not the dot product above (see there).
#include "fk_dev.h"

namespace tik {
using namespace fkd;         // TB bodies per tile, KP the feature row length
constexpr int JW = 8;        // output columns (waves) per workgroup
constexpr int KC = 64;       // k per staged chunk
constexpr int LDF = TB + 1;  // LDS row stride of the transposed chunk (the staging writes spread over banks)
constexpr int NLD = KC * TB / 4 / (64 * JW);   // f32x4 staging loads per thread per chunk
static_assert(NLD * 4 * 64 * JW == KC * TB, "chunk must divide over the workgroup");

// part[3 i + c] = sum over the chunk's k of feat[b][k] * PT[3 v_i + c][k], from zero, k ascending.
// DIRECT: sf is the lane's own feature row in global memory; else the transposed chunk in LDS.
template <int NP, bool DIRECT>
__device__ __forceinline__ void fkj_blend_chunk(float (&part)[9], const float* sf, const float* const (&row)[3], int lane) {
#pragma unroll
    for (int e = 0; e < 9; ++e) part[e] = 0.f;
#pragma unroll 2
    for (int k4 = 0; k4 < KC; k4 += 4) {
        f32x4 p[NP][3];
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[i][c] = *reinterpret_cast<const f32x4*>(row[i] + c * KP + k4);
        f32x4 f4;
        if (DIRECT) f4 = *reinterpret_cast<const f32x4*>(sf + k4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = DIRECT ? f4[e] : sf[(k4 + e) * LDF + lane];
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) part[3 * i + c] = fmaf(f, p[i][c][e], part[3 * i + c]);
        }
    }
}

// one chunk of this wave's column: kind 1 vertex joint, 2 landmark (uniform rows), 3 contour (per-lane rows)
template <bool DIRECT>
__device__ __forceinline__ void fkj_chunk(float (&part)[9], int kind, const float* sf, const float* const (&urow)[3],
                                          const float* const (&lrow)[3], int kc, int lane) {
    if (kind == 3) {
        const float* const rk[3] = {lrow[0] + kc * KC, lrow[1] + kc * KC, lrow[2] + kc * KC};
        fkj_blend_chunk<3, DIRECT>(part, sf, rk, lane);
    } else {
        const float* const rk[3] = {urow[0] + kc * KC, urow[1] + kc * KC, urow[2] + kc * KC};
        if (kind == 1) fkj_blend_chunk<1, DIRECT>(part, sf, rk, lane);
        else fkj_blend_chunk<3, DIRECT>(part, sf, rk, lane);
    }
}

// x = T[:3,:3] vp + T[:,3] with T = sum_j W[v][j] A_j(b), the skinning entries in table order (joints ascending)
__device__ __forceinline__ void fkj_skin(const FkJointsArgs& a, int v, int b, const float* vp, float* x) {
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
    const int K = skin_count(a);
    for (int n = 0; n < K; ++n) {
        const SkinEntry s = skin_entry<false>(a, v, n);   // v is the lane's own for a contour joint
        const f32x4* r = ak_rows(a, s.k, b);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 t = r[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) T[4 * q + e] = fmaf(s.w, t[e], T[4 * q + e]);
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) x[g] = row_affine(f32x4{T[4 * g], T[4 * g + 1], T[4 * g + 2], T[4 * g + 3]}, vp);
}

__global__ __launch_bounds__(64 * JW) void fk_joints_kernel(FkJointsArgs a) {
    __shared__ __attribute__((aligned(16))) float sF[2][KC * LDF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * TB, b = b0 + lane;
    const bool live = b < a.B;
    const int bc = live ? b : a.B - 1;
    // this wave's output column: split, the workgroup's one; else every gridDim.y-th, from blockIdx.y
    const int nby = gridDim.y;
    const int s = a.split ? (int)blockIdx.y : wv * nby + (int)blockIdx.y;
    auto joint_of = [&](int col) { return col < a.n_sel ? (a.sel_all ? col : (int)a.sel[col]) : -1; };
    const int j = joint_of(s);
    bool need = j >= 55;   // any column of this workgroup past the chain joints
    if (!a.split)
        for (int w = 0; w < JW; ++w) need |= joint_of(w * nby + (int)blockIdx.y) >= 55;

    // this wave's column: 0 none / chain joint, 1 vertex joint, 2 landmark, 3 contour landmark
    const int jj = j - 55;
    const int kind = jj < 0 ? 0 : jj < a.nextra ? 1 : jj < a.nextra + a.nlmk ? 2 : 3;
    int vu[3] = {0, 0, 0}, vl[3] = {0, 0, 0};   // vertex ids: wave-uniform (static joints) / per lane (contour)
    float w[3] = {0.f, 0.f, 0.f};
    if (kind == 1 || kind == 2) {
        for (int i = 0; i < 3; ++i) {
            const Pick p = pick(a, j, i);
            vu[i] = p.v;
            w[i] = p.bw;
        }
    } else if (kind == 3) {
        const int bin = min(max(a.dyn_bin[bc], 0), 78);
        const int o = (bin * a.ndyn + (jj - a.nextra - a.nlmk)) * 3;
        for (int i = 0; i < 3; ++i) {
            vl[i] = a.dyn_v[o + i];
            w[i] = a.dyn_w[o + i];
        }
    }
    const float* urow[3];   // P^T rows 3 v .. 3 v + 2 of each vertex
    const float* lrow[3];
    for (int i = 0; i < 3; ++i) {
        urow[i] = a.PT + (size_t)vu[i] * 3 * KP;
        lrow[i] = a.PT + (size_t)vl[i] * 3 * KP;
    }

    float acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.f;
    if (need && a.split) {
        // wave = chunk: its partial sums to LDS, wave 0 adds them in chunk order
        float part[9];
        fkj_chunk<true>(part, kind, a.feat + (size_t)bc * KP + wv * KC, urow, lrow, wv, lane);
        float* sP = &sF[0][0];   // [chunk][9][lane]
#pragma unroll
        for (int e = 0; e < 9; ++e) sP[(wv * 9 + e) * 64 + lane] = part[e];
        __syncthreads();
        if (wv != 0) return;
        for (int kc = 0; kc < KP / KC; ++kc)
#pragma unroll
            for (int e = 0; e < 9; ++e) acc[e] += sP[(kc * 9 + e) * 64 + lane];
    } else if (need) {
        f32x4 st[NLD];
        auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < NLD; ++r) {
                const int q = tid + 64 * JW * r, body = q >> 4, k4 = q & 15;
                st[r] = b0 + body < a.B ? *reinterpret_cast<const f32x4*>(a.feat + (size_t)(b0 + body) * KP + kc * KC + 4 * k4)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        auto put = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < NLD; ++r) {
                const int q = tid + 64 * JW * r, body = q >> 4, k4 = q & 15;
#pragma unroll
                for (int e = 0; e < 4; ++e) sF[buf][(4 * k4 + e) * LDF + body] = st[r][e];
            }
        };
        load(0);
        put(0);
        __syncthreads();
        for (int kc = 0; kc < KP / KC; ++kc) {
            if (kc + 1 < KP / KC) load(kc + 1);
            if (kind != 0) {
                float part[9];
                fkj_chunk<false>(part, kind, sF[kc & 1], urow, lrow, kc, lane);
#pragma unroll
                for (int e = 0; e < 9; ++e) acc[e] += part[e];
            }
            if (kc + 1 < KP / KC) put((kc + 1) & 1);
            __syncthreads();
        }
    } else if (a.split && wv != 0) {
        return;   // a chain column: wave 0 copies it
    }
    if (j < 0 || !live) return;   // no barrier below
    float o[3];
    if (kind == 0) {
        const float* c = a.jchain + ((size_t)b * 55 + j) * 3;
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
    } else {
        o[0] = o[1] = o[2] = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (i > 0 && kind == 1) break;   // a vertex joint is one evaluation
            float x[3];
            fkj_skin(a, kind == 3 ? vl[i] : vu[i], b, acc + 3 * i, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = fmaf(w[i], x[c], o[c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] += a.transl ? a.transl[(size_t)b * 3 + c] : 0.f;
    }
    float* d = a.out + ((size_t)b * a.n_sel + s) * 3;
    d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
}

hipError_t launch_fk_joints(const FkJointsArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.n_sel <= 0) return hipSuccess;
    if (!a.jchain || !a.out || (!a.sel_all && a.n_sel > FKJ_MAX_SEL) || !nz_ok(a)) return hipErrorInvalidValue;
    (void)hipGetLastError();
    // few workgroups (a small batch or a short selection): a workgroup per column, its waves over k
    FkJointsArgs k = a;
    const unsigned tiles = (a.B + TB - 1) / TB, nby = (a.n_sel + JW - 1) / JW;
    k.split = tiles * nby <= 64 ? 1 : 0;
    static_assert(8 * 9 * 64 <= 2 * KC * LDF, "the split partials reuse the chunk buffers");
    hipLaunchKernelGGL(fk_joints_kernel, dim3(tiles, k.split ? a.n_sel : nby), dim3(64 * JW), 0, st, k);
    return hipGetLastError();
}

}  // namespace tik
