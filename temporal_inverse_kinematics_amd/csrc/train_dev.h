// train_dev.h — what the training kernels (train_bn.hip, train_wgrad.hip,
// train_head.hip, train_batch.hip) share, each written once: the launch
// helpers with the float4 preamble, the folded ReLU backward, the fixed-order
// reductions, the finalize kernels' prologue and the descriptor-batch walk.
#pragma once
#include "dev_common.h"   // f32x4
#include "train.h"

namespace tik {

static inline unsigned nblk(long long n, int b) { return (unsigned)((n + b - 1) / b); }

// kernel<<<grid, block, 0, st>>>(a...) and the launch's error
template <class K, class... A>
hipError_t launch(K kernel, dim3 grid, dim3 block, hipStream_t st, A... a) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, a...);
    return hipGetLastError();
}
// one thread per element, 256 per workgroup: nothing to launch at n == 0, n < 0 (f4_count) refused
template <class K, class... A>
hipError_t launch_n(K kernel, long long n, hipStream_t st, A... a) {
    if (n <= 0) return n ? hipErrorInvalidValue : hipSuccess;
    return launch(kernel, nblk(n, 256), 256, st, a...);
}
// the float4 launch preamble: n floats in rows of C as float4s under a 32-bit index, -1 where that cannot be
static inline long long f4_count(long long n, int C) { return n && (C % 4 || n / 4 >= (1LL << 31)) ? -1 : n / 4; }

// ReLU backward folded into a consumer of g: g where the ReLU output m is positive
__device__ __forceinline__ f32x4 relu_gate(f32x4 g, const f32x4 m) {
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = m[e] > 0.f ? g[e] : 0.f;
    return g;
}

// sum of s over the NT threads of the workgroup (all of them call), the same
// on every run: the halving tree over red[NT] in LDS
template <int NT>
__device__ __forceinline__ double block_sum(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// sum over chunks of base[z * stride]: the 64 lanes of a wave stride the
// chunks, then a fixed xor-shuffle tree across the wave
__device__ __forceinline__ double chunk_sum64(const double* __restrict__ base, int nchunk, size_t stride, int lane) {
    double s = 0.0;
    for (int z = lane; z < nchunk; z += 64) s += base[(size_t)z * stride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// The finalize kernels' prologue: 256 threads = 4 columns, one wave (64 chunk
// lanes) each. s[k] = the sum over chunks of part[z][c][k], k < NS, for this
// wave's column c of C (PER doubles per column and chunk). True on the one
// lane that writes the column; false on the others and past the last column.
template <int NS, int PER>
__device__ __forceinline__ bool column_sums(const double* __restrict__ part, int nchunk, int C, int& c,
                                            double (&s)[NS]) {
    const int lane = threadIdx.x & 63;
    c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return false;
#pragma unroll
    for (int k = 0; k < NS; ++k) s[k] = chunk_sum64(part + (size_t)PER * c + k, nchunk, (size_t)PER * C, lane);
    return lane == 0;
}

// Descriptor batches: every descriptor of a table (D has count() and block0)
// in one launch, 1024 elements per 256-thread workgroup. The host lays the
// block ranges out and returns the grid size; workgroup b calls f(q, i) for
// the descriptor q whose range holds b, 4 elements i per thread at stride 256.
template <class D>
long long batch_blocks(D* descs, int nd) {
    long long b = 0;
    for (int d = 0; d < nd; ++d) {
        descs[d].block0 = b;
        b += (descs[d].count() + 1023) / 1024;
    }
    return b;
}
template <class D, class F>
__device__ __forceinline__ void batch_visit(const D* __restrict__ descs, int nd, F f) {
    int d = 0;
    while (d + 1 < nd && descs[d + 1].block0 <= (long long)blockIdx.x) ++d;
    const D& q = descs[d];
    const long long n = q.count();
    for (long long i = (blockIdx.x - q.block0) * 1024LL + threadIdx.x, e = 0; e < 4; ++e, i += 256) {
        if (i >= n) return;
        f(q, i);
    }
}

}  // namespace tik
