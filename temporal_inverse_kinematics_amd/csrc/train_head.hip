// train_head.hip — the head's LeakyReLU + Dropout(0.7) (pose_trainer.py:89-92),
// the losses (nn.MSELoss, pose_trainer.py:46-49; the keypoint term; the eval
// pass's MSE) and torch.optim.Adam (configure_optimizers,
// pose_trainer.py:196-197). Every loss sum is block_sum's fixed tree.
#include "train_dev.h"

namespace tik {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void dropout_mask_kernel(float* mask, long long n, float keep, unsigned long long seed) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long h = splitmix64(seed ^ splitmix64((unsigned long long)i));
    const float u = (float)(h >> 40) * (1.0f / 16777216.0f);   // 24-bit uniform in [0, 1)
    mask[i] = u < keep ? 1.f : 0.f;
}

hipError_t launch_dropout_mask(float* mask, long long n, float keep, unsigned long long seed, hipStream_t st) {
    return launch_n(dropout_mask_kernel, n, st, mask, n, keep, seed);
}

__global__ void leaky_dropout_kernel(float* __restrict__ D, const float* __restrict__ P, const float* __restrict__ mask,
                                     float scale, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p = P[i];
    const float l = p > 0.f ? p : 0.01f * p;
    D[i] = l * (mask[i] * scale);
}

hipError_t launch_leaky_dropout(float* D, const float* P, const float* mask, float scale, long long n, hipStream_t st) {
    return launch_n(leaky_dropout_kernel, n, st, D, P, mask, scale, n);
}

__global__ void leaky_dropout_bwd_kernel(float* dP, const float* dD, const float* __restrict__ P,
                                         const float* __restrict__ mask, float scale, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float g = dD[i] * (mask[i] * scale);
    dP[i] = P[i] > 0.f ? g : g * 0.01f;
}

hipError_t launch_leaky_dropout_bwd(float* dP, const float* dD, const float* P, const float* mask, float scale,
                                    long long n, hipStream_t st) {
    return launch_n(leaky_dropout_bwd_kernel, n, st, dP, dD, P, mask, scale, n);
}

// one workgroup: the loss is a few thousand to a few hundred thousand elements
__global__ __launch_bounds__(1024) void mse_kernel(const float* __restrict__ O, int ldo, const float* __restrict__ T,
                                                   long long rows, int cols, float* __restrict__ dO,
                                                   float* __restrict__ loss) {
    __shared__ double red[1024];
    const long long n = rows * cols;
    const float inv = 2.f / (float)n;
    double s = 0.0;
    for (long long i = threadIdx.x; i < rows * ldo; i += blockDim.x) {
        const long long r = i / ldo;
        const int c = (int)(i % ldo);
        if (c < cols) {
            const float d = O[i] - T[r * cols + c];
            s += (double)d * d;
            dO[i] = inv * d;
        } else {
            dO[i] = 0.f;
        }
    }
    s = block_sum<1024>(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}

hipError_t launch_mse(const float* O, int ldo, const float* T, long long rows, int cols, float* dO, float* loss,
                      hipStream_t st) {
    return launch(mse_kernel, 1, 1024, st, O, ldo, T, rows, cols, dO, loss);
}

// one workgroup: thread i adds rows i, i + 1024, .. in double, then block_sum
__global__ __launch_bounds__(1024) void kp_loss_reduce_kernel(const float* __restrict__ lf, long long rows, float weight,
                                                              const float* pose_mse, float* loss, float* parts) {
    __shared__ double red[1024];
    double s = 0.0;
    for (long long i = threadIdx.x; i < rows; i += blockDim.x) s += (double)lf[i];
    s = block_sum<1024>(s, red);
    if (threadIdx.x == 0) {
        const float pm = pose_mse[0];
        const float km = (float)(2.0 * s / (51.0 * (double)rows));
        if (parts) {
            parts[0] = pm;
            parts[1] = km;
        }
        loss[0] = weight > 0.f ? fmaf(weight, km, pm) : pm;
    }
}

hipError_t launch_kp_loss_reduce(const float* lf, long long rows, float weight, const float* pose_mse, float* loss,
                                 float* parts, hipStream_t st) {
    return launch(kp_loss_reduce_kernel, 1, 1024, st, lf, rows, weight, pose_mse, loss, parts);
}

// validation loss: workgroup b sums its contiguous chunk of (O - T)^2 in double
// (threads strided inside the chunk, LDS tree), part[b]; the finalize workgroup
// adds the partials in a fixed order. No gradient, no atomics.
constexpr int MSE_CHUNK = 4096;    // elements per workgroup pass
constexpr int MSE_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void mse_eval_kernel(const float* __restrict__ O, int ldo, const float* __restrict__ T,
                                                       long long n, int cols, long long per_block,
                                                       double* __restrict__ part) {
    __shared__ double red[256];
    const long long lo = (long long)blockIdx.x * per_block;
    const long long hi = lo + per_block < n ? lo + per_block : n;
    double s = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const long long r = i / cols;
        const int c = (int)(i - r * cols);
        const float d = O[r * ldo + c] - T[i];
        s += (double)d * d;
    }
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void mse_eval_finalize_kernel(const double* __restrict__ part, int nb, long long n,
                                                                float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)n);
}

int mse_eval_blocks(long long n) {
    const long long b = (n + MSE_CHUNK - 1) / MSE_CHUNK;
    return (int)(b < 1 ? 1 : (b > MSE_MAX_BLOCKS ? MSE_MAX_BLOCKS : b));
}

hipError_t launch_mse_eval(const float* O, int ldo, const float* T, long long rows, int cols, float* loss, double* part,
                           hipStream_t st) {
    const long long n = rows * cols;
    if (n <= 0 || cols > ldo) return hipErrorInvalidValue;
    const int nb = mse_eval_blocks(n);
    const long long per_block = (n + nb - 1) / nb;
    hipLaunchKernelGGL(mse_eval_kernel, dim3(nb), dim3(256), 0, st, O, ldo, T, n, cols, per_block, part);
    hipLaunchKernelGGL(mse_eval_finalize_kernel, dim3(1), dim3(256), 0, st, part, nb, n, loss);
    return hipGetLastError();
}

// ---------------------------------------------------------------- Adam
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float w1, float b2, float w2, float step_size,
                            float bc2_sqrt, float eps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    float mi = m[i];
    mi = mi + w1 * (gi - mi);                 // exp_avg.lerp_(grad, 1 - beta1)
    float vi = v[i] * b2;                     // exp_avg_sq.mul_(beta2)
    vi = vi + w2 * gi * gi;                   //           .addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] + step_size * (mi / denom);   // param.addcdiv_(exp_avg, denom, value=-step_size)
    m[i] = mi;
    v[i] = vi;
}

hipError_t launch_adam(float* p, const float* g, float* m, float* v, long long n, float lr, double b1, double b2,
                       float eps, double bc1, double bc2, hipStream_t st) {
    const float w1 = (float)(1.0 - b1), w2 = (float)(1.0 - b2);
    const float step_size = (float)(-(double)lr / bc1);
    const float bc2s = (float)sqrt(bc2);
    return launch_n(adam_kernel, n, st, p, g, m, v, n, w1, (float)b2, w2, step_size, bc2s, eps);
}

}  // namespace tik
