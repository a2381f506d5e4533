// xgemm_dev.h — device pieces shared by the bf16x3 GEMM kernels (xgemm.hip,
// xgraph.hip, xblock.hip, xtws.hip):
//   xsplit8 / xsplit8_part / xsplit4   fp32 -> three bf16 planes (8 or 4 channels)
//   xmma, xmma6                        one product; the six of a K step, weights as A
//   xmix_row                           one output joint of the graph mix + bias2 + ReLU
//   xst4                               epilogue store (nontemporal or plain)
//   tik_llvm_raw_buffer_load_v4f32     16-B buffer load into registers (zeros out of range)
//   xtile_run, XPhaseClock             a persistent workgroup's run of tiles; -DTIK_XTRACE stamps
//   xa_swz, xa_dma_unit, xskin_row, XCfg   xgemm.hip's A image, EPI_SKIN rows, tile and LDS ring
#pragma once
#include <hip/hip_runtime.h>

#include "cgemm.h"
#include "dev_common.h"
#include "xgemm.h"

namespace tik {

typedef __bf16 xbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 xbf16x4 __attribute__((ext_vector_type(4)));

// element e of the three planes: b0 = bf16(x), b1 = bf16(x - b0), b2 = bf16(x - b0 - b1)
template <class P>
__device__ __forceinline__ void xsplit1(const float x, P& p0, P& p1, P& p2, int e) {
    const __bf16 b0 = (__bf16)x;
    const float r1 = x - (float)b0;
    const __bf16 b1 = (__bf16)r1;
    p0[e] = b0;
    p1[e] = b1;
    p2[e] = (__bf16)(r1 - (float)b1);
}

__device__ __forceinline__ void xsplit8(const f32x4 lo, const f32x4 hi, xbf16x8& p0, xbf16x8& p1, xbf16x8& p2) {
#pragma unroll
    for (int e = 0; e < 8; ++e) xsplit1(e < 4 ? lo[e] : hi[e - 4], p0, p1, p2, e);
}

// part q (0..3) of xsplit8: elements 2q, 2q + 1 (the same arithmetic), so a
// fragment's split can be spread over four MFMA groups
__device__ __forceinline__ void xsplit8_part(const f32x4 lo, const f32x4 hi, xbf16x8& p0, xbf16x8& p1, xbf16x8& p2, int q) {
#pragma unroll
    for (int e = 2 * q; e < 2 * q + 2; ++e) xsplit1(e < 4 ? lo[e] : hi[e - 4], p0, p1, p2, e);
}

// 4 channels (one 16-B fp32 unit -> 8 B per plane): the cooperative splits into an LDS planes image
__device__ __forceinline__ void xsplit4(const f32x4 x, xbf16x4& p0, xbf16x4& p1, xbf16x4& p2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) xsplit1(x[e], p0, p1, p2, e);
}

// epilogue stores of output tiles: nontemporal for the backbone's layer
// outputs (XArgs::nts; same-box A/B +0.9 % IK frames/s), plain for split-K
// partials and the FK GEMMs (re-read at once; NT measured slower there)
__device__ __forceinline__ void xst4(float* p, const f32x4 v, bool nt) {
    if (nt) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else *reinterpret_cast<f32x4*>(p) = v;
}

__device__ __forceinline__ int xa_swz(int r) { return (r >> 1) & 7; }

// A DMA: the lane that fills unit lane & 7 of image row rr fetches the logical
// unit pl = (lane & 7) ^ swz(rr) (g = pl & 3, h = pl >> 2); its byte offset in
// the row's 128-B K block
__device__ __forceinline__ int xa_dma_unit(int rr, int lane) {
    const int pl = (lane & 7) ^ xa_swz(rr);
    return 32 * (pl & 3) + 16 * (pl >> 2);
}

// one bf16 MFMA of the bf16x3 product. TR: C^T = W . X^T, so lane l ends with
// row (l & 15), channels 4 (l >> 4) .. +3; else lane l holds column (l & 15), rows 4 (l >> 4) .. +3
template <bool TR>
__device__ __forceinline__ void xmma(const xbf16x8& x, const xbf16x8& w, f32x4& c) {
    c = TR ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, c, 0, 0, 0)
           : __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, w, c, 0, 0, 0);
}

// the six products of one K step, transposed (weights are the A operand), in
// the one order every bf16x3 kernel keeps (bitwise equality rests on it):
// (w0,x2) (w1,x1) (w2,x0) (w0,x1) (w1,x0) (w0,x0). xgemm.hip's two kernels
// spell it out: TR is a parameter there and their planes are not [3] arrays
__device__ __forceinline__ void xmma6(const xbf16x8 (&w)[3], const xbf16x8 (&x)[3], f32x4& c) {
    xmma<true>(x[2], w[0], c);
    xmma<true>(x[1], w[1], c);
    xmma<true>(x[0], w[2], c);
    xmma<true>(x[1], w[0], c);
    xmma<true>(x[0], w[1], c);
    xmma<true>(x[0], w[0], c);
}

// graph mix of output joint w (compile-time, as is the v loop: the sparse
// COCO pattern unrolls) on 4 channels: z = bias2[w] (bias_row), then
// z += A[v][w] y[v] for v ascending, ReLU. Only the y[v] that the pattern
// names are read. amv: A_eff across the wave (xam)
template <bool SPARSE>
__device__ __forceinline__ f32x4 xmix_row(const f32x4 (&y)[17], const float (&amv)[5], const float* bias_row, int w) {
    f32x4 z = *reinterpret_cast<const f32x4*>(bias_row);
#pragma unroll
    for (int v = 0; v < 17; ++v)
        if (!SPARSE || ((coco_hop2_mask3(w) >> v) & 1u)) z += xam(amv, v * 17 + w) * y[v];
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = z[e] > 0.f ? z[e] : 0.f;
    return z;
}

// 16 B per lane from rsrc + voffset into registers (offsets at or past
// num_records read zeros); aux: cache policy, an immediate (0, or 2 = nontemporal)
__device__ f32x4 tik_llvm_raw_buffer_load_v4f32(i32x4 rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.buffer.load.v4f32");

// persistent kernels: this workgroup's contiguous run [t_begin, t_end) of
// ntiles tiles, the runs ordered per XCD (xcd_slot)
__device__ __forceinline__ void xtile_run(int ntiles, int& t_begin, int& t_end) {
    const int nwg = gridDim.x, s = xcd_slot(blockIdx.x, nwg);
    t_begin = (int)((long long)s * ntiles / nwg);
    t_end = (int)((long long)(s + 1) * ntiles / nwg);
}

// -DTIK_XTRACE phase clock of a persistent kernel: stamp(on, i) adds the time
// since the last stamp to phase i (i < 0: starts the clock). In a normal
// build `on` is a constexpr false and all of it folds away
template <int N>
struct XPhaseClock {
    unsigned long long ph[N] = {}, tlast = 0, tstart = 0;
    __device__ __forceinline__ void stamp(bool on, int i) {
        if (!on) return;
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        if (i >= 0) ph[i] += t - tlast;
        else tstart = t;
        tlast = t;
    }
    __device__ __forceinline__ void store(unsigned long long* o) const {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = ph[i];
    }
};

// EPI_SKIN: body b and transform row k of a lane's 4 GEMM rows rb .. rb + 3
// (rb % 4 == 0, so they never straddle bodies). 16 rows per body: k == 3 is
// the [0 0 0 1] row (not stored); 12 rows per body: the 3x4 part only
__device__ __forceinline__ void xskin_row(int rb, int srows, int& b, int& k) {
    const int q = rb >> 2;
    if (srows == 12) {
        b = q / 3;
        k = q - 3 * b;
    } else {
        b = q >> 2;
        k = q & 3;
    }
}

template <int BN, int EPI, int NW_>
struct XCfg {
    // NW = 4 waves of 32 rows (two 16-row fragments) each: a 128-row workgroup
    // of <= 80 KB LDS, two per CU, so one workgroup's prologue and epilogue run
    // under the other's main loop
    static_assert(NW_ == 4, "one tile shape");
    static constexpr int NW = NW_, NT = 64 * NW, BM = 32 * NW, FM = 2, FN = BN / 16, RW = 32;
    static constexpr bool TR = EPI == EPI_BIAS;   // transposed MFMA: each lane ends with 4 channels of a row
    static constexpr int ABYTES = BM * 128;
    static constexpr int PLANE = BN * 64;
    static constexpr int BBYTES = 3 * PLANE;
    // A rows are DMA'd and consumed by the same wave (wave w fills and reads rows
    // 32w..32w+31), so the A ring needs no barrier: 2 slots, issued 2 steps ahead
    // (a slot is free once its step's fragments were split, one step early).
    // B (weights) is shared by all waves, one barrier per step: issued LB = 1 step
    // ahead into NSB = 2 slots (the wait for B(k+1) sits after step k's MFMAs, so
    // the DMA has a whole step to land)
    static constexpr int LB = 1, NSA = 2, NSB = 2;
    static constexpr int RING = NSA * ABYTES + NSB * BBYTES;
    static constexpr int NIA = ABYTES / 1024 / NW;   // A DMA instructions per wave per stage
    static constexpr int NIB_TOT = BBYTES / 1024;
    static constexpr int NIBW = NIB_TOT / NW;   // B DMA instructions per wave per stage
    static constexpr int RT = EPI == EPI_GRAPH ? BM / 17 * 17 : BM;   // valid rows per tile (whole frames for the mix)
    static constexpr int LDCG = BN + 4;
    // C tile (+ the bias2 slice for the graph mix)
    static constexpr int CT = EPI == EPI_GRAPH ? BM * LDCG * 4 + 17 * BN * 4 : BM * LDCG * 4;
    static constexpr int SMEM = RING > CT ? RING : CT;
    static constexpr int WG_PER_CU = 2;
    static_assert(NIA * 1024 * NW == ABYTES && NIA * 8 == RW, "A DMA split");
    static_assert(NIBW * NW == NIB_TOT, "B DMA split: every wave issues NIBW");
    static_assert(SMEM * WG_PER_CU <= 160 * 1024, "LDS");
};

}  // namespace tik
