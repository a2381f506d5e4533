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
#include "dev_common.h"
#include "lm_dev.h"

// Every numbered step lives in lm_dev.h, shared with lm_sum.hip and lm_chain.hip; so do the entry point's
// range checks and its launch.
namespace tik {

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

__global__ __launch_bounds__(LM_T) void lm_solve_kernel(LmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, m = a.m;
    const size_t b = blockIdx.x;
    const LmLds s(smem, n);
    lm_clear(s, n);
    __syncthreads();
    // 1. normal matrix and gradient, rows ascending
    lm_accumulate_body(s, a.jac + b * m * n, a.r + b * m, a.row_w, m, n);
    // 2. damping and right-hand side; from here thread i owns row i (n <= 165 < LM_T)
    const int i = threadIdx.x;
    const float x = -lm_damp(s, n, a.mu + a.lambda[b], a.mu, a.prior ? a.prior + b * n : nullptr);
    __syncthreads();
    // 3. Cholesky, 4. L y = rhs, then L^T delta = y
    const bool ok = lm_factor_solve(s, n, x);
    if (i < n) a.delta[b * n + i] = ok ? s.sG[i] : __builtin_nanf("");
}

}  // namespace tik

using namespace tik_host;

extern "C" int tik_lm_solve(const float* jac, const float* r, const float* prior, const float* row_w, const float* lambda,
                            float mu, int B, int m, int n, float* delta, void* stream) {
    if (!jac || !r || !lambda || !delta) return fail(TIK_E_INVALID, "tik_lm_solve: null pointer");
    if (B <= 0) return fail(TIK_E_INVALID, "tik_lm_solve: B must be positive, got %d", B);
    if (int rc = tik::lm_check_range("tik_lm_solve", n, tik::LM_MAX_N, &m, &mu)) return rc;
    const tik::LmArgs a{B, m, n, mu, jac, r, prior, row_w, lambda, delta};
    return tik::lm_launch(tik::lm_solve_kernel, B, tik::lm_lds_floats(n), stream, a);
}
