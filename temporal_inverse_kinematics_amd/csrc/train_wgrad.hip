// train_wgrad.hip — the reductions over rows that are products of two
// activations: the weight-gradient GEMM with the temporal conv's im2col and
// zero-upsample, and the graph-mix einsum with its edge-importance gradient
// (gconv_origin.py:64, st_gcn_aaai18.py:104-108,129).
#include "train_dev.h"

namespace tik {

// C[m][n] = sum_r A[r][m] B[r][n]: 64 x 64 output tile per workgroup, 4 waves
// of 32 x 32 (2 x 2 v_mfma_f32_16x16x4_f32 fragments), 16 rows per LDS step
// (A and B staged [row][64 + 16 pad] so a 16-lane group reads 16 consecutive
// floats of one row and the four groups land on distinct banks). MFMA
// operands: A-op lane l = A^T[m = l&15][k = l>>4] = As[k][m], B-op =
// Bs[k][n]; D lane l holds rows 4(l>>4)+e, column l&15.
// Tap mode (g.C > 0): B is the conv input itself, read through the temporal
// conv's row map (implicit im2col): column n = tap*C + ci of row r is
// B[(nw*tin + s*t + tap - pad)*V + v][ci] (zero outside the window), r =
// (nw*tout + t)*V + v; a 64-column tile never straddles taps (C % 64 == 0).
__global__ __launch_bounds__(256) void wgrad_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B,
                                                    int ldb, int M, int N, long long R, long long rows_per,
                                                    float* __restrict__ part, WgradTaps g) {
    constexpr int LDS_LD = 80;
    __shared__ float As[16 * LDS_LD];
    __shared__ float Bs[16 * LDS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const long long r0 = (long long)blockIdx.z * rows_per;
    const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
    const int lr = tid >> 4, c4 = (tid & 15) * 4;
    const bool avec = (lda % 4 == 0) && (m0 + c4 + 3 < M);
    const bool bvec = (ldb % 4 == 0) && (n0 + c4 + 3 < N);
    const int tap = g.C ? n0 / g.C : 0;
    const int bcol = g.C ? n0 - tap * g.C : n0;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // tap mode: this thread's row r0 + lr decoded once into (window, frame,
    // joint), then advanced incrementally by 16 rows per step (V = 17 > 16:
    // at most one joint wrap and one frame wrap per step; no 64-bit divides
    // in the loop)
    int tv = 0, tt = 0;
    long long tn = 0;
    if (g.C) {
        const long long row = r0 + lr;
        tv = (int)(row % g.V);
        const long long q = row / g.V;
        tt = (int)(q % g.tout);
        tn = q / g.tout;
    }
    // rows r .. r+15 of A and B into registers (zero past the chunk / matrix edge)
    auto load = [&](long long r, f32x4& av, f32x4& bv) {
        av = f32x4{0.f, 0.f, 0.f, 0.f};
        bv = f32x4{0.f, 0.f, 0.f, 0.f};
        const long long row = r + lr;
        long long brow = row;
        bool bok = true;
        if (g.C) {
            const int ts = g.s * tt + tap - g.pad;
            bok = ts >= 0 && ts < g.tin;
            brow = (tn * g.tin + ts) * g.V + tv;
            tv += 16;
            if (tv >= g.V) {
                tv -= g.V;
                if (++tt >= g.tout) { tt = 0; ++tn; }
            }
        }
        if (row < r1) {
            const float* ap = A + row * lda + m0 + c4;
            const float* bp = B + brow * ldb + bcol + c4;
            if (avec) av = *reinterpret_cast<const f32x4*>(ap);
            else
                for (int e = 0; e < 4; ++e) av[e] = (m0 + c4 + e < M) ? ap[e] : 0.f;
            if (!bok) {
            } else if (bvec) {
                bv = *reinterpret_cast<const f32x4*>(bp);
            } else {
                for (int e = 0; e < 4; ++e) bv[e] = (n0 + c4 + e < N) ? bp[e] : 0.f;
            }
        }
    };
    f32x4 av, bv;
    load(r0, av, bv);
    for (long long r = r0; r < r1; r += 16) {
        __syncthreads();
        *reinterpret_cast<f32x4*>(As + lr * LDS_LD + c4) = av;
        *reinterpret_cast<f32x4*>(Bs + lr * LDS_LD + c4) = bv;
        __syncthreads();
        // the next 16 rows' global loads are in flight during this step's MFMAs
        if (r + 16 < r1) load(r + 16, av, bv);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[k * LDS_LD + wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[k * LDS_LD + wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float* o = part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + wm * 32 + i * 16 + 4 * (lane >> 4) + e;
                const int n = n0 + wn * 32 + j * 16 + (lane & 15);
                if (m < M && n < N) o[(size_t)m * N + n] = acc[i][j][e];
            }
}

// sum of the row-split partials; tap mode stores column tap*C + ci at ci*kt + tap
__global__ void wgrad_reduce_kernel(const float* __restrict__ part, int splits, int M, int N, float* C, int ldc,
                                    int tapC, int kt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)M * N) return;
    const size_t st = (size_t)M * N;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int z = 0;
    for (; z + 3 < splits; z += 4) {
        s0 += part[(size_t)z * st + i];
        s1 += part[(size_t)(z + 1) * st + i];
        s2 += part[(size_t)(z + 2) * st + i];
        s3 += part[(size_t)(z + 3) * st + i];
    }
    for (; z < splits; ++z) s0 += part[(size_t)z * st + i];
    const int n = (int)(i % N);
    const int col = tapC ? (n % tapC) * kt + n / tapC : n;
    C[(i / N) * ldc + col] = (s0 + s1) + (s2 + s3);
}

hipError_t launch_wgrad(const float* A, int lda, const float* B, int ldb, int M, int N, long long R, float* C,
                        int ldc, float* part, long long part_cap, hipStream_t st, const WgradTaps& g) {
    if (M <= 0 || N <= 0) return hipSuccess;
    if (g.C && (g.C % 64 || N != g.kt * g.C || g.V <= 16 || g.tout <= 0)) return hipErrorInvalidValue;
    const int gx = (M + 63) / 64, gy = (N + 63) / 64;
    constexpr int target = 512;   // workgroups (256 -3 %, 1024 +-0.3 %: profiles/r02_t15_train_ab.txt)
    long long splits = target / (gx * gy);
    const long long max_by_rows = (R + 255) / 256;   // >= 256 rows per split
    if (splits > max_by_rows) splits = max_by_rows;
    if ((long long)M * N > part_cap) return hipErrorInvalidValue;
    if (splits > part_cap / ((long long)M * N)) splits = part_cap / ((long long)M * N);
    if (splits < 1) splits = 1;
    long long rows_per = (R + splits - 1) / splits;
    rows_per = (rows_per + 15) / 16 * 16;
    if (rows_per < 16) rows_per = 16;
    splits = R > 0 ? (R + rows_per - 1) / rows_per : 1;
    hipLaunchKernelGGL(wgrad_kernel, dim3(gx, gy, (unsigned)splits), dim3(256), 0, st, A, lda, B, ldb, M, N, R,
                       rows_per, part, g);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(nblk((long long)M * N, 256)), dim3(256), 0, st, part, (int)splits, M,
                       N, C, ldc, g.C, g.kt);
    return hipGetLastError();
}

// ---------------------------------------------------------------- temporal-conv helpers
__global__ void im2col_kernel(float* __restrict__ col, const float* __restrict__ src, int lds, int C, int kt, int s,
                              int pad, long long n_out, int tin, int tout, int V) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out * C) return;
    const long long r = i / C;
    const int ci = (int)(i % C);
    const int v = (int)(r % V);
    const long long q = r / V;
    const int t = (int)(q % tout);
    const long long n = q / tout;
    float* o = col + r * ((long long)C * kt) + (long long)ci * kt;
    for (int tap = 0; tap < kt; ++tap) {
        const int ts = s * t + tap - pad;
        o[tap] = (ts >= 0 && ts < tin) ? src[((n * tin + ts) * V + v) * lds + ci] : 0.f;
    }
}

hipError_t launch_im2col(float* col, const float* src, int lds, int C, int kt, int s, int pad, int N, int tin,
                         int tout, int V, hipStream_t st) {
    const long long n_out = (long long)N * tout * V;
    return launch_n(im2col_kernel, n_out * C, st, col, src, lds, C, kt, s, pad, n_out, tin, tout, V);
}

// float4 per thread, 32-bit index arithmetic (counts < 2^31 in float4 units)
__global__ void upsample_kernel(float* __restrict__ up, const float* __restrict__ src, unsigned C4, int s,
                                unsigned n4, unsigned tin, unsigned tout, unsigned V) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const unsigned r = i / C4, c4 = i - r * C4;
    const unsigned q = r / V, v = r - q * V;
    const unsigned n = q / tin, t = q - n * tin;
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (t % s == 0) val = reinterpret_cast<const f32x4*>(src)[((n * tout + t / s) * V + v) * C4 + c4];
    reinterpret_cast<f32x4*>(up)[i] = val;
}

hipError_t launch_upsample(float* up, const float* src, int C, int s, int N, int tin, int tout, int V, hipStream_t st) {
    const long long n4 = f4_count((long long)N * tin * V * C, C);
    return launch_n(upsample_kernel, n4, st, up, src, (unsigned)(C / 4), s, (unsigned)n4, (unsigned)tin, (unsigned)tout,
                    (unsigned)V);
}

// ---------------------------------------------------------------- graph mix
// one thread per (frame, 4 channels): the 17 joint rows in registers, the
// 17x17 matrix in LDS (broadcast reads)
__global__ __launch_bounds__(256) void mix_kernel(float* __restrict__ out, const float* __restrict__ in,
                                                  const float* __restrict__ A, int trans, long long frames, int C) {
    __shared__ float As[17 * 17];
    for (int i = threadIdx.x; i < 289; i += 256) {
        const int v = i / 17, w = i % 17;
        As[i] = trans ? A[w * 17 + v] : A[i];
    }
    __syncthreads();
    const int C4 = C / 4;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames * C4) return;
    const long long f = idx / C4;
    const int c = (int)(idx % C4) * 4;
    const float* src = in + f * 17 * C + c;
    f32x4 y[17];
#pragma unroll
    for (int v = 0; v < 17; ++v) y[v] = *reinterpret_cast<const f32x4*>(src + (size_t)v * C);
    float* dst = out + f * 17 * C + c;
#pragma unroll
    for (int w = 0; w < 17; ++w) {
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 17; ++v) z += As[v * 17 + w] * y[v];
        *reinterpret_cast<f32x4*>(dst + (size_t)w * C) = z;
    }
}

hipError_t launch_mix(float* out, const float* in, const float* A, int trans, long long frames, int C, hipStream_t st) {
    if (C % 4) return hipErrorInvalidValue;
    return launch_n(mix_kernel, frames * (C / 4), st, out, in, A, trans, frames, C);
}

// part[chunk][v*17 + w] = sum over the chunk's frames and all channels of
// Y[f][v][c] * dZ[f][w][c]: both 17 x C frame images staged in LDS (rows
// padded by one float), one (v, w) pair per thread (threads 0..32 take two)
constexpr int MIXG_CMAX = 256;
__global__ __launch_bounds__(256) void mix_grad_kernel(const float* __restrict__ Y, const float* __restrict__ G,
                                                       long long frames, int C, long long fpc,
                                                       double* __restrict__ part) {
    __shared__ float Ys[17 * (MIXG_CMAX + 1)];
    __shared__ float Gs[17 * (MIXG_CMAX + 1)];
    const int tid = threadIdx.x;
    const int ld = C + 1;
    const int p0 = tid, p1 = tid + 256;
    const int v0 = p0 / 17, w0 = p0 % 17;
    const int v1 = p1 / 17, w1 = p1 % 17;
    double acc0 = 0.0, acc1 = 0.0;
    const long long f0 = (long long)blockIdx.x * fpc;
    const long long f1 = f0 + fpc < frames ? f0 + fpc : frames;
    for (long long f = f0; f < f1; ++f) {
        const float* ys = Y + f * 17 * C;
        const float* gs = G + f * 17 * C;
        for (int i = tid; i < 17 * C; i += 256) {
            const int v = i / C, c = i - v * C;
            Ys[v * ld + c] = ys[i];
            Gs[v * ld + c] = gs[i];
        }
        __syncthreads();
        float s0 = 0.f, s1 = 0.f;
        for (int c = 0; c < C; ++c) {
            s0 += Ys[v0 * ld + c] * Gs[w0 * ld + c];
            if (p1 < 289) s1 += Ys[v1 * ld + c] * Gs[w1 * ld + c];
        }
        acc0 += s0;
        acc1 += s1;
        __syncthreads();
    }
    double* o = part + (size_t)blockIdx.x * 289;
    o[p0] = acc0;   // p0 < 256 < 289
    if (p1 < 289) o[p1] = acc1;
}

__global__ __launch_bounds__(256) void mix_grad_finalize_kernel(const double* __restrict__ part, int nchunk,
                                                                const float* __restrict__ A, float* dE) {
    int i;   // one wave per (v, w)
    double s[1];
    if (column_sums<1, 1>(part, nchunk, 289, i, s)) dE[i] = (float)s[0] * A[i];
}

hipError_t launch_mix_grad(const float* Y, const float* dZ, long long frames, int C, const float* A, float* dE,
                           double* part, int max_chunks, hipStream_t st) {
    if (C > MIXG_CMAX) return hipErrorInvalidValue;
    long long nc = frames < 512 ? frames : 512;
    if (nc > max_chunks) nc = max_chunks;
    if (nc < 1) nc = 1;
    const long long fpc = (frames + nc - 1) / nc;
    nc = frames > 0 ? (frames + fpc - 1) / fpc : 0;
    if (nc > 0)
        hipLaunchKernelGGL(mix_grad_kernel, dim3((unsigned)nc), dim3(256), 0, st, Y, dZ, frames, C, fpc, part);
    hipLaunchKernelGGL(mix_grad_finalize_kernel, dim3(nblk(289, 4)), dim3(256), 0, st, part, (int)nc, A, dE);
    return hipGetLastError();
}

}  // namespace tik
