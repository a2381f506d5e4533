// lm_solve.hip — batched damped normal equations for Levenberg-Marquardt (tik_lm_solve):
//   (J^T W J + (mu + lambda_b) I) delta = -(J^T W r + mu prior)          per body b
// for thousands of small systems (n <= 165 unknowns, m <= 768 residual rows).
//
// One workgroup of 256 threads per body, everything in LDS, one launch:
//   1. the lower triangle of J^T W J, packed (entry (i, j <= i) at i (i + 1) / 2 + j), and J^T W r:
//      rows of J pass through LDS in chunks of 8; every entry is an fp32 FMA chain over the rows in
//      ascending order, (J[r][i] w[r]) J[r][j] per term, started from zero;
//   2. the damping on the diagonal, the right-hand side -(g + mu prior);
//   3. Cholesky, left-looking, thread i = row i: at column j every row i >= j takes
//      N[i][j] - sum_{k<j} L[i][k] L[j][k] (k ascending), row j's value is the pivot;
//   4. L y = rhs and L^T delta = y, column oriented, each thread carrying its own unknown.
// A pivot that is not positive (or NaN) sets a flag, the factorisation stops at that column for
// the whole workgroup, and the body's delta is NaN; nothing loops on it. Only delta goes back
// to HBM. A body's arithmetic does not see the batch, so its bits are the same for any B.
#include "common.h"
#include "dev_common.h"

namespace tik {

constexpr int LM_T = 256;     // threads per workgroup
constexpr int LM_RC = 8;      // rows of J per staged chunk
constexpr int LM_MAX_N = 165;
constexpr int LM_MAX_M = 768;

struct LmArgs {
    int B, m, n;
    float mu;
    const float* jac;      // (B,m,n)
    const float* r;        // (B,m)
    const float* prior;    // (B,n) or null
    const float* row_w;    // (m) or null
    const float* lambda;   // (B)
    float* delta;          // (B,n)
};

__host__ __device__ constexpr int lm_tri(int i) { return i * (i + 1) / 2; }
__host__ __device__ constexpr size_t lm_lds_floats(int n) {
    return (size_t)lm_tri(n) + 2 * (size_t)n + (size_t)LM_RC * n + 2 * LM_RC + 4;
}
static_assert(lm_lds_floats(LM_MAX_N) * 4 <= 64 * 1024, "the largest system must fit the workgroup's LDS");

__global__ __launch_bounds__(LM_T) void lm_solve_kernel(LmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, m = a.m, tid = threadIdx.x, ntri = lm_tri(n);
    const size_t b = blockIdx.x;
    float* sN = smem;                 // packed lower triangle, then L in place
    float* sG = sN + ntri;            // J^T W r, then delta
    float* sY = sG + n;               // y of the forward solve
    float* sJ = sY + n;               // LM_RC rows of J
    float* sW = sJ + LM_RC * n;       // their weights
    float* sR = sW + LM_RC;           // their residuals
    float* sP = sR + LM_RC;           // [0] pivot, [1] flag (non-zero: not positive definite)
    for (int e = tid; e < ntri; e += LM_T) sN[e] = 0.f;
    for (int i = tid; i < n; i += LM_T) sG[i] = 0.f;
    if (tid == 0) sP[1] = 0.f;
    __syncthreads();
    // 1. normal matrix and gradient, rows ascending
    const float* J = a.jac + b * m * n;
    for (int r0 = 0; r0 < m; r0 += LM_RC) {
        const int rc = min(LM_RC, m - r0);
        for (int q = tid; q < rc * n; q += LM_T) sJ[q] = J[(size_t)r0 * n + q];
        if (tid < rc) {
            sW[tid] = a.row_w ? a.row_w[r0 + tid] : 1.f;
            sR[tid] = a.r[b * m + r0 + tid];
        }
        __syncthreads();
        for (int e = tid; e < ntri; e += LM_T) {
            int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
            while (lm_tri(i) > e) --i;
            while (lm_tri(i + 1) <= e) ++i;
            const int j = e - lm_tri(i);
            float acc = sN[e];
            for (int rr = 0; rr < rc; ++rr) acc = fmaf(sJ[rr * n + i] * sW[rr], sJ[rr * n + j], acc);
            sN[e] = acc;
        }
        for (int i = tid; i < n; i += LM_T) {
            float acc = sG[i];
            for (int rr = 0; rr < rc; ++rr) acc = fmaf(sJ[rr * n + i] * sW[rr], sR[rr], acc);
            sG[i] = acc;
        }
        __syncthreads();
    }
    // 2. damping and right-hand side; from here thread i owns row i (n <= 165 < LM_T)
    const int i = tid;
    const bool own = i < n;
    const int ti = lm_tri(own ? i : 0);
    float x = 0.f;
    if (own) {
        sN[ti + i] += a.mu + a.lambda[b];
        x = -(a.prior ? fmaf(a.mu, a.prior[b * n + i], sG[i]) : sG[i]);
    }
    __syncthreads();
    // 3. Cholesky
    bool bad = false;
    for (int j = 0; j < n; ++j) {
        const int tj = lm_tri(j);
        float s = 0.f;
        if (own && i >= j) {
            s = sN[ti + j];
            for (int k = 0; k < j; ++k) s = fmaf(-sN[ti + k], sN[tj + k], s);
            if (i == j) {
                const bool ok = s > 0.f;
                if (!ok) sP[1] = 1.f;
                sP[0] = ok ? sqrtf(s) : 1.f;
            }
        }
        __syncthreads();
        const float piv = sP[0];
        bad = sP[1] != 0.f;   // read between the barriers: the same for every thread, and before column j + 1 can set it
        if (own && i >= j) sN[ti + j] = i == j ? piv : s / piv;
        __syncthreads();
        if (bad) break;
    }
    if (bad) {
        if (own) a.delta[b * n + i] = __builtin_nanf("");
        return;
    }
    // 4. L y = rhs, then L^T delta = y
    for (int j = 0; j < n; ++j) {
        if (i == j) sY[j] = x / sN[ti + j];
        __syncthreads();
        if (own && i > j) x = fmaf(-sN[ti + j], sY[j], x);
    }
    if (own) x = sY[i];
    for (int j = n - 1; j >= 0; --j) {
        if (i == j) sG[j] = x / sN[ti + j];
        __syncthreads();
        if (own && i < j) x = fmaf(-sN[lm_tri(j) + i], sG[j], x);
    }
    if (own) a.delta[b * n + i] = sG[i];
}

}  // namespace tik

using namespace tik_host;

extern "C" int tik_lm_solve(const float* jac, const float* r, const float* prior, const float* row_w, const float* lambda,
                            float mu, int B, int m, int n, float* delta, void* stream) {
    if (!jac || !r || !lambda || !delta) return fail(TIK_E_INVALID, "tik_lm_solve: null pointer");
    if (B <= 0) return fail(TIK_E_INVALID, "tik_lm_solve: B must be positive, got %d", B);
    if (n < 1 || n > tik::LM_MAX_N) return fail(TIK_E_INVALID, "tik_lm_solve: n must be 1..%d, got %d", tik::LM_MAX_N, n);
    if (m < 1 || m > tik::LM_MAX_M) return fail(TIK_E_INVALID, "tik_lm_solve: m must be 1..%d, got %d", tik::LM_MAX_M, m);
    if (!(mu >= 0.f)) return fail(TIK_E_INVALID, "tik_lm_solve: mu must be >= 0, got %g", (double)mu);
    tik::LmArgs a{B, m, n, mu, jac, r, prior, row_w, lambda, delta};
    (void)hipGetLastError();
    hipLaunchKernelGGL(tik::lm_solve_kernel, dim3(B), dim3(tik::LM_T), tik::lm_lds_floats(n) * sizeof(float),
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return TIK_OK;
}
