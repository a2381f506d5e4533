// lm_dev.h — the pieces shared by lm_solve.hip (one system per body), lm_sum.hip (one system summed over
// the batch) and lm_chain.hip (the frames of a sequence tied together). On the device: the LDS layout and
// the clearing of the sums, the normal-equation accumulation of one body, the damping with the gradient of the
// right-hand side, the Cholesky and the two triangular solves. Workgroups of LM_T threads; every sum is
// an fp32 FMA chain in a fixed order, so the three files produce the same bits from the same operands.
// On the host: the entry points' range checks and their launch.
#pragma once
#include "common.h"

namespace tik {

constexpr int LM_T = 256;     // threads per workgroup
constexpr int LM_RC = 8;      // rows of J per staged chunk
constexpr int LM_MAX_N = 165;
constexpr int LM_MAX_M = 768;
constexpr int LM_RUN = 32;    // bodies per partial sum of tik_lm_accumulate (include/tik.h: TIK_LM_RUN)

__host__ __device__ constexpr int lm_tri(int i) { return i * (i + 1) / 2; }
__host__ __device__ constexpr size_t lm_lds_floats(int n) {
    return (size_t)lm_tri(n) + 2 * (size_t)n + (size_t)LM_RC * n + 2 * LM_RC + 4;
}
static_assert(lm_lds_floats(LM_MAX_N) * 4 <= 64 * 1024, "the largest system must fit the workgroup's LDS");

// The workgroup's LDS, carved from one dynamic array of lm_lds_floats(n) floats.
struct LmLds {
    float* sN;   // packed lower triangle (entry (i, j <= i) at lm_tri(i) + j), then L in place
    float* sG;   // J^T W r, then delta
    float* sY;   // y of the forward solve
    float* sJ;   // LM_RC rows of J
    float* sW;   // their weights
    float* sR;   // their residuals
    float* sP;   // [0] pivot, [1] flag (non-zero: not positive definite)
    __device__ LmLds(float* smem, int n)
        : sN(smem), sG(sN + lm_tri(n)), sY(sG + n), sJ(sY + n), sW(sJ + LM_RC * n), sR(sW + LM_RC), sP(sR + LM_RC) {}
};

// Row i of entry e of a packed lower triangle; its column is e - lm_tri(i).
__device__ __forceinline__ int lm_untri(int e) {
    int i = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    while (lm_tri(i) > e) --i;
    while (lm_tri(i + 1) <= e) ++i;
    return i;
}

// sN, sG and the flag to zero; the caller's barrier follows.
__device__ __forceinline__ void lm_clear(const LmLds& s, int n) {
    for (int e = threadIdx.x; e < lm_tri(n) + n; e += LM_T) s.sN[e] = 0.f;   // sG follows sN
    if (threadIdx.x == 0) s.sP[1] = 0.f;
}

// sN += J^T W J (packed lower triangle), sG += J^T W r for one body: rows of J (m, n) pass through
// LDS in chunks of LM_RC; every entry is an fp32 FMA chain over the rows in ascending order,
// (J[r][i] w[r]) J[r][j] per term, continued from what sN / sG hold. Called by the whole
// workgroup; ends on a barrier.
__device__ __forceinline__ void lm_accumulate_body(const LmLds& s, const float* J, const float* r, const float* row_w, int m, int n) {
    const int tid = threadIdx.x, ntri = lm_tri(n);
    float *sN = s.sN, *sG = s.sG, *sJ = s.sJ, *sW = s.sW, *sR = s.sR;
    for (int r0 = 0; r0 < m; r0 += LM_RC) {
        const int rc = min(LM_RC, m - r0);
        for (int q = tid; q < rc * n; q += LM_T) sJ[q] = J[(size_t)r0 * n + q];
        if (tid < rc) {
            sW[tid] = row_w ? row_w[r0 + tid] : 1.f;
            sR[tid] = r[r0 + tid];
        }
        __syncthreads();
        for (int e = tid; e < ntri; e += LM_T) {
            const int i = lm_untri(e), j = e - lm_tri(i);
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
}

// Thread i < n (row i): `damp` onto the diagonal of sN. -> g_i + mu prior_i (g_i alone without a prior), the
// gradient whose negative is the right-hand side; 0 for the other threads. The caller's barrier follows.
__device__ __forceinline__ float lm_damp(const LmLds& s, int n, float damp, float mu, const float* prior) {
    const int i = threadIdx.x;
    if (i >= n) return 0.f;
    s.sN[lm_tri(i) + i] += damp;
    return prior ? fmaf(mu, prior[i], s.sG[i]) : s.sG[i];
}

// L y = x and L^T z = y with L in sN; thread i = row i, x its right-hand side -> z in sG. Called by the whole
// workgroup after a barrier behind the last write of sN.
__device__ __forceinline__ void lm_solve_factored(const LmLds& s, int n, float x) {
    float *sN = s.sN, *sG = s.sG, *sY = s.sY;
    const int i = threadIdx.x;
    const bool own = i < n;
    const int ti = lm_tri(own ? i : 0);
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
}

// Cholesky of sN in place, then L y = x and L^T delta = y; thread i = row i (n <= 165 < LM_T), x its
// right-hand side. Left-looking: at column j every row i >= j takes N[i][j] - sum_{k<j} L[i][k] L[j][k]
// (k ascending), row j's value is the pivot. A pivot that is not positive (or NaN) sets the flag and the
// factorisation stops at that column for the whole workgroup: -> false, nothing solved. Otherwise
// -> true with delta in sG. Called by the whole workgroup after a barrier behind the last write of sN.
__device__ __forceinline__ bool lm_factor_solve(const LmLds& s, int n, float x) {
    float *sN = s.sN, *sP = s.sP;
    const int i = threadIdx.x;
    const bool own = i < n;
    const int ti = lm_tri(own ? i : 0);
    bool bad = false;
    for (int j = 0; j < n; ++j) {
        const int tj = lm_tri(j);
        float t = 0.f;
        if (own && i >= j) {
            t = sN[ti + j];
            for (int k = 0; k < j; ++k) t = fmaf(-sN[ti + k], sN[tj + k], t);
            if (i == j) {
                const bool ok = t > 0.f;
                if (!ok) sP[1] = 1.f;
                sP[0] = ok ? sqrtf(t) : 1.f;
            }
        }
        __syncthreads();
        const float piv = sP[0];
        bad = sP[1] != 0.f;   // read between the barriers: the same for every thread, and before column j + 1 can set it
        if (own && i >= j) sN[ti + j] = i == j ? piv : t / piv;
        __syncthreads();
        if (bad) break;
    }
    if (bad) return false;
    lm_solve_factored(s, n, x);   // the factor loop ended on a barrier
    return true;
}

// ---- host: what the entry points (`who`) share
// n within 1..max_n, then m within 1..LM_MAX_M and mu >= 0 where the entry point has them (else null)
inline int lm_check_range(const char* who, int n, int max_n, const int* m, const float* mu) {
    using namespace tik_host;
    if (n < 1 || n > max_n) return fail(TIK_E_INVALID, "%s: n must be 1..%d, got %d", who, max_n, n);
    if (m && (*m < 1 || *m > LM_MAX_M)) return fail(TIK_E_INVALID, "%s: m must be 1..%d, got %d", who, LM_MAX_M, *m);
    if (mu && !(*mu >= 0.f)) return fail(TIK_E_INVALID, "%s: mu must be >= 0, got %g", who, (double)*mu);
    return TIK_OK;
}

// `blocks` workgroups of LM_T threads with lds_floats of LDS
template <class Args>
int lm_launch(void (*kernel)(Args), int blocks, size_t lds_floats, void* stream, const Args& a) {
    using namespace tik_host;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LM_T), lds_floats * sizeof(float), (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return TIK_OK;
}

}  // namespace tik
