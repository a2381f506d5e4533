// train_bn.hip — train-mode BatchNorm (batch statistics, running-stat
// momentum update, st_gcn_aaai18.py:74-75,178,186,203), its backward, and the
// elementwise passes around it: affine + residual + ReLU, ReLU backward.
//
// Layout: activations are channels-last rows r = (n*T + t)*17 + v of C fp32.
// The per-channel reductions (BatchNorm statistics, bias and BN-parameter
// gradients) are column reductions over those rows: 64 consecutive columns
// per workgroup (coalesced 256-B row segments), rows split over chunks,
// double partial sums reduced in a fixed order (run-to-run deterministic).
#include "train_dev.h"

namespace tik {

// Workgroup = 16 column quads (64 columns, float4 loads: one 256-B row
// segment per 16 lanes) x 16 row lanes over a chunk of rows; double
// accumulators; the 16 row lanes reduced through LDS in a fixed order.
constexpr int CS_ROWS = 128;   // rows per chunk
__global__ __launch_bounds__(256) void colstats_kernel(const float* __restrict__ A, const float* __restrict__ G,
                                                       const float* __restrict__ M, const float* __restrict__ mean,
                                                       long long R, int C, long long rows_per,
                                                       double* __restrict__ part) {
    __shared__ double red[2][16][64];
    const int tid = threadIdx.x, q = tid & 15, rl = tid >> 4;
    const int c = blockIdx.x * 64 + 4 * q;
    const long long r0 = (long long)blockIdx.y * rows_per;
    const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < C) {
        f32x4 mu = {0.f, 0.f, 0.f, 0.f};
        if (G && mean) mu = *reinterpret_cast<const f32x4*>(mean + c);
        for (long long r = r0 + rl; r < r1; r += 16) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(A + r * C + c);
            if (G) {
                f32x4 g = *reinterpret_cast<const f32x4*>(G + r * C + c);
                if (M) g = relu_gate(g, *reinterpret_cast<const f32x4*>(M + r * C + c));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s1[e] += g[e];
                    s2[e] += (double)g[e] * (double)(a[e] - mu[e]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s1[e] += a[e];
                    s2[e] += (double)a[e] * a[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[0][rl][4 * q + e] = s1[e];
        red[1][rl][4 * q + e] = s2[e];
    }
    __syncthreads();
    if (tid < 128) {
        const int k = tid >> 6, cl = tid & 63;
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[k][i][cl];
        const int col = blockIdx.x * 64 + cl;
        if (col < C) part[((size_t)blockIdx.y * C + col) * 2 + k] = t;
    }
}

hipError_t launch_colstats(const float* A, const float* G, const float* M, const float* mean, long long R, int C,
                           double* part, int max_chunks, int* nchunk, hipStream_t st) {
    if (C % 4) return hipErrorInvalidValue;
    const int gx = (C + 63) / 64;
    constexpr int cs_rows = CS_ROWS;   // 128 measured best (256 -5 %, 64 +-0.3 %: profiles/r02_t15_train_ab.txt)
    long long nc = (R + cs_rows - 1) / cs_rows;
    if (nc > max_chunks) nc = max_chunks;
    if (nc < 1) nc = 1;
    const long long rows_per = R > 0 ? (R + nc - 1) / nc : 1;
    nc = R > 0 ? (R + rows_per - 1) / rows_per : 1;
    *nchunk = (int)nc;
    hipLaunchKernelGGL(colstats_kernel, dim3(gx, (unsigned)nc), dim3(256), 0, st, A, G, M, mean, R, C, rows_per, part);
    return hipGetLastError();
}

// finalize kernels: one wave per column (column_sums), lane 0 writes
__global__ __launch_bounds__(256) void bn_fwd_finalize_kernel(const double* __restrict__ part, int nchunk, long long R,
                                                              int C, const int* __restrict__ cmap,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* run_mean,
                                                              float* run_var, float momentum, float eps,
                                                              float* __restrict__ stat) {
    int c;
    double s[2];
    if (!column_sums<2, 2>(part, nchunk, C, c, s)) return;
    const double s1 = s[0], s2 = s[1];
    const int p = cmap ? cmap[c] : c;
    if (p < 0) {
        stat[c] = 0.f; stat[C + c] = 0.f; stat[2 * C + c] = 0.f; stat[3 * C + c] = 0.f;
        return;
    }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    const float m = (float)mean;
    const float sc = gamma[p] * is;
    stat[c] = m;
    stat[C + c] = is;
    stat[2 * C + c] = sc;
    stat[3 * C + c] = beta[p] - m * sc;
    if (run_mean) {
        const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
        run_mean[p] = (1.f - momentum) * run_mean[p] + momentum * m;
        run_var[p] = (1.f - momentum) * run_var[p] + momentum * (float)unb;
    }
}

hipError_t launch_bn_fwd_finalize(const double* part, int nchunk, long long R, int C, const int* cmap,
                                  const float* gamma, const float* beta, float* run_mean, float* run_var,
                                  float momentum, float eps, float* stat, hipStream_t st) {
    return launch(bn_fwd_finalize_kernel, nblk(C, 4), 256, st, part, nchunk, R, C, cmap, gamma, beta, run_mean, run_var,
                  momentum, eps, stat);
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int nchunk, long long R,
                                                              int C, const int* __restrict__ cmap,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ stat, float* dgamma,
                                                              float* dbeta, float* __restrict__ k) {
    int c;
    double s[2];
    if (!column_sums<2, 2>(part, nchunk, C, c, s)) return;
    const double s1 = s[0], s2 = s[1];
    const int p = cmap ? cmap[c] : c;
    if (p < 0) {
        k[c] = 0.f; k[C + c] = 0.f; k[2 * C + c] = 0.f;
        return;
    }
    const double is = stat[C + c];
    const double g = gamma[p];
    dgamma[p] = (float)(s2 * is);
    dbeta[p] = (float)s1;
    // dx = g*is*(dy - mean(dy) - xhat*mean(dy*xhat))
    k[c] = (float)(g * is);
    k[C + c] = (float)(-g * is * is * is * s2 / (double)R);
    k[2 * C + c] = (float)(-g * is * s1 / (double)R);
}

hipError_t launch_bn_bwd_finalize(const double* part, int nchunk, long long R, int C, const int* cmap,
                                  const float* gamma, const float* stat, float* dgamma, float* dbeta, float* k,
                                  hipStream_t st) {
    return launch(bn_bwd_finalize_kernel, nblk(C, 4), 256, st, part, nchunk, R, C, cmap, gamma, stat, dgamma, dbeta, k);
}

__global__ __launch_bounds__(256) void colsum_finalize_kernel(const double* __restrict__ part, int nchunk, int C,
                                                              float* dst) {
    int c;
    double s[1];
    if (column_sums<1, 2>(part, nchunk, C, c, s)) dst[c] = (float)s[0];
}

hipError_t launch_colsum_finalize(const double* part, int nchunk, int C, float* dst, hipStream_t st) {
    return launch(colsum_finalize_kernel, nblk(C, 4), 256, st, part, nchunk, C, dst);
}

// ---------------------------------------------------------------- elementwise
// float4 per thread (every C here is a multiple of 4); the channel index from
// 32-bit arithmetic (element counts stay below 2^31 in float4 units)
__global__ void affine_kernel(float* __restrict__ out, const float* __restrict__ X, const float* __restrict__ sc,
                              const float* __restrict__ sh, const float* __restrict__ R2,
                              const float* __restrict__ sc2, const float* __restrict__ sh2, unsigned n4, unsigned C4,
                              int relu) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const unsigned c = (i % C4) * 4;
    const f32x4 x = reinterpret_cast<const f32x4*>(X)[i];
    const f32x4 a = *reinterpret_cast<const f32x4*>(sc + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(sh + c);
    f32x4 v = x * a + b;
    if (R2) {
        const f32x4 r = reinterpret_cast<const f32x4*>(R2)[i];
        if (sc2) v += r * *reinterpret_cast<const f32x4*>(sc2 + c) + *reinterpret_cast<const f32x4*>(sh2 + c);
        else v += r;
    }
    if (relu)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
    reinterpret_cast<f32x4*>(out)[i] = v;
}

hipError_t launch_affine(float* out, const float* X, const float* sc, const float* sh, const float* R2,
                         const float* sc2, const float* sh2, long long R, int C, int relu, hipStream_t st) {
    const long long n4 = f4_count(R * C, C);
    return launch_n(affine_kernel, n4, st, out, X, sc, sh, R2, sc2, sh2, (unsigned)n4, (unsigned)(C / 4), relu);
}

__global__ void bn_bwd_apply_kernel(float* __restrict__ out, const float* __restrict__ G,
                                    const float* __restrict__ M, const float* __restrict__ X,
                                    const float* __restrict__ stat, const float* __restrict__ k, unsigned n4,
                                    unsigned C4) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const unsigned c = (i % C4) * 4, C = C4 * 4;
    f32x4 g = reinterpret_cast<const f32x4*>(G)[i];
    if (M) g = relu_gate(g, reinterpret_cast<const f32x4*>(M)[i]);
    const f32x4 x = reinterpret_cast<const f32x4*>(X)[i];
    const f32x4 mu = *reinterpret_cast<const f32x4*>(stat + c);
    const f32x4 k0 = *reinterpret_cast<const f32x4*>(k + c);
    const f32x4 k1 = *reinterpret_cast<const f32x4*>(k + C + c);
    const f32x4 k2 = *reinterpret_cast<const f32x4*>(k + 2 * C + c);
    reinterpret_cast<f32x4*>(out)[i] = g * k0 + (x - mu) * k1 + k2;
}

hipError_t launch_bn_bwd_apply(float* out, const float* G, const float* M, const float* X, const float* stat,
                               const float* k, long long R, int C, hipStream_t st) {
    const long long n4 = f4_count(R * C, C);
    return launch_n(bn_bwd_apply_kernel, n4, st, out, G, M, X, stat, k, (unsigned)n4, (unsigned)(C / 4));
}

__global__ void relu_bwd_kernel(float* __restrict__ out, const float* __restrict__ G, const float* __restrict__ M,
                                long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = M[i] > 0.f ? G[i] : 0.f;   // G read only where it passes
}

hipError_t launch_relu_bwd(float* out, const float* G, const float* M, long long n, hipStream_t st) {
    return launch_n(relu_bwd_kernel, n, st, out, G, M, n);
}

}  // namespace tik
