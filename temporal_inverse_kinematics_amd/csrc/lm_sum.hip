// lm_sum.hip — normal equations whose unknowns are shared by the whole batch (tik_lm_accumulate,
// tik_lm_solve_sum): the shape step of a sequence,
//   (sum_b J_b^T W J_b + (mu + lambda) I) delta = -(sum_b J_b^T W r_b + mu prior).
//
// lm_accumulate_kernel: one workgroup of 256 threads per run of LM_RUN = 32 bodies, everything in
// LDS. The packed lower triangle and the gradient start from zero and take the run's bodies in
// ascending order, each body's rows in ascending order (lm_dev.h: the accumulation of lm_solve.hip,
// continued from body to body), so every entry is one fp32 FMA chain and a row of `partial` depends
// on its own bodies only. Row q of partial: the triangle (n (n + 1) / 2 floats), then the gradient (n).
// lm_solve_sum_kernel: one workgroup adds the n_part rows in ascending order, puts mu + lambda on
// the diagonal, forms -(g + mu prior), then factors and solves exactly as lm_solve.hip does
// (lm_dev.h: lm_damp, lm_factor_solve). A pivot that is not positive writes NaN into delta and nothing else.
// No atomics, no waiting between workgroups, plain vector stores.
#include "dev_common.h"
#include "lm_dev.h"

namespace tik {

struct LmAccArgs {
    int B, m, n;
    const float* jac;      // (B,m,n)
    const float* r;        // (B,m)
    const float* row_w;    // (m) or null
    float* partial;        // (ceil(B / LM_RUN), n (n + 1) / 2 + n)
};

struct LmSumArgs {
    int n_part, n;
    float mu, lambda;
    const float* partial;  // (n_part, n (n + 1) / 2 + n)
    const float* prior;    // (n) or null
    float* delta;          // (n)
};

__global__ __launch_bounds__(LM_T) void lm_accumulate_kernel(LmAccArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, m = a.m, tid = threadIdx.x, ntri = lm_tri(n);
    const LmLds s(smem, n);
    lm_clear(s, n);
    __syncthreads();
    const int b0 = blockIdx.x * LM_RUN, b1 = min(a.B, b0 + LM_RUN);
    for (int b = b0; b < b1; ++b) lm_accumulate_body(s, a.jac + (size_t)b * m * n, a.r + (size_t)b * m, a.row_w, m, n);
    float* o = a.partial + (size_t)blockIdx.x * (ntri + n);
    for (int e = tid; e < ntri + n; e += LM_T) o[e] = s.sN[e];
}

__global__ __launch_bounds__(LM_T) void lm_solve_sum_kernel(LmSumArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, tid = threadIdx.x, ntri = lm_tri(n);
    const LmLds s(smem, n);
    for (int e = tid; e < ntri + n; e += LM_T) {
        float acc = a.partial[e];
        for (int q = 1; q < a.n_part; ++q) acc += a.partial[(size_t)q * (ntri + n) + e];
        s.sN[e] = acc;
    }
    if (tid == 0) s.sP[1] = 0.f;
    __syncthreads();
    const float x = -lm_damp(s, n, a.mu + a.lambda, a.mu, a.prior);
    __syncthreads();
    const bool ok = lm_factor_solve(s, n, x);
    const int i = tid;
    if (i < n) a.delta[i] = ok ? s.sG[i] : __builtin_nanf("");
}

}  // namespace tik

using namespace tik_host;

extern "C" int tik_lm_accumulate(const float* jac, const float* r, const float* row_w, int B, int m, int n,
                                 float* partial, void* stream) {
    if (!jac || !r || !partial) return fail(TIK_E_INVALID, "tik_lm_accumulate: null pointer");
    if (B <= 0) return fail(TIK_E_INVALID, "tik_lm_accumulate: B must be positive, got %d", B);
    if (int rc = tik::lm_check_range("tik_lm_accumulate", n, tik::LM_MAX_N, &m, nullptr)) return rc;
    static_assert(tik::LM_RUN == TIK_LM_RUN, "include/tik.h states the run length");
    const tik::LmAccArgs a{B, m, n, jac, r, row_w, partial};
    return tik::lm_launch(tik::lm_accumulate_kernel, (B + tik::LM_RUN - 1) / tik::LM_RUN, tik::lm_lds_floats(n), stream, a);
}

extern "C" int tik_lm_solve_sum(const float* partial, int n_part, const float* prior, float mu, float lambda, int n,
                                float* delta, void* stream) {
    if (!partial || !delta) return fail(TIK_E_INVALID, "tik_lm_solve_sum: null pointer");
    if (n_part <= 0) return fail(TIK_E_INVALID, "tik_lm_solve_sum: n_part must be positive, got %d", n_part);
    if (int rc = tik::lm_check_range("tik_lm_solve_sum", n, tik::LM_MAX_N, nullptr, &mu)) return rc;
    if (!(lambda >= 0.f)) return fail(TIK_E_INVALID, "tik_lm_solve_sum: lambda must be >= 0, got %g", (double)lambda);
    const tik::LmSumArgs a{n_part, n, mu, lambda, partial, prior, delta};
    return tik::lm_launch(tik::lm_solve_sum_kernel, 1, tik::lm_lds_floats(n), stream, a);
}
