// lm_chain.hip — damped normal equations of whole sequences with neighbouring frames tied together
// (tik_lm_solve_chain): per sequence q of frames a .. b - 1, c_f the number of neighbours of f inside it,
//   D_f = J_f^T W_f J_f + ((mu + lambda[q]) + smooth c_f) I
//   b_f = -( fma(mu, prior_f, J_f^T W_f r_f) + smooth (c_f theta_f - theta_{f-1} - theta_{f+1}) )
//   D_f delta_f - smooth delta_{f-1} - smooth delta_{f+1} = b_f
// symmetric positive definite, block tridiagonal, every off-diagonal block -smooth I.
//
// lm_chain_accumulate_kernel: one workgroup of 256 threads per frame, the accumulation of lm_solve.hip
// (lm_dev.h). Row f of the workspace: the packed lower triangle of D_f (n (n + 1) / 2 floats), then b_f (n).
// The Jacobian work is all here, off the sequential path.
// lm_chain_sweep_kernel: one workgroup per sequence, everything in LDS, block Cholesky (block Thomas).
//   forward, frames ascending: S_f = D_f - smooth^2 S_{f-1}^-1 (S_a = D_a), each entry fmaf(-smooth^2, Sinv, D);
//     y_f = fmaf(smooth, x_{f-1}, b_f); S_f = L_f L_f^T and x_f = S_f^-1 y_f by lm_factor_solve; L_f and x_f
//     replace row f; then M = L_f^-1 (thread c = column c by forward substitution, no barrier inside) and
//     S_f^-1 = M^T M (the packed triangle spread over the 256 threads, k ascending) for the next frame;
//   backward, frames descending: delta_{b-1} = x_{b-1}, delta_f = fmaf(smooth, (L_f L_f^T)^-1 delta_{f+1}, x_f),
//     L_f and x_f read back from row f, the two solves by lm_solve_factored.
// lm_dev.h holds every piece named above that lm_solve.hip has too (accumulation, damping, factor, solves, lm_untri).
// The off-diagonal blocks being a multiple of the identity is what keeps this small: no block is ever
// multiplied by another. With smooth == 0, or in a sequence of one frame, no term of the coupling is
// formed at all and delta is bit for bit lm_solve.hip's. A pivot that is not positive (or NaN) at any
// frame writes NaN into the whole sequence's delta and ends that workgroup; nothing loops on it. A
// sequence whose bounds are not 0 <= a < b <= F does no work, and a frame that no such sequence holds is
// skipped: no index leaves [0, F) whatever seq_starts holds. A sequence's arithmetic does not see the
// launch, so its bits are the same for any S. No atomics, no waiting between workgroups.
#include "dev_common.h"
#include "lm_dev.h"

namespace tik {

constexpr int LM_CHAIN_MAX_N = 96;
static_assert(LM_CHAIN_MAX_N == TIK_LM_CHAIN_MAX_N, "include/tik.h states the limit");
static_assert(LM_CHAIN_MAX_N <= LM_T && LM_CHAIN_MAX_N <= LM_MAX_N, "thread i owns row i");

// The sweep's LDS: lm_dev.h's layout (S_f then L_f in sN), then S_{f-1}^-1, M = L_f^-1 and x_{f-1}:
// three packed triangles plus vectors.
__host__ __device__ constexpr size_t lm_chain_lds_floats(int n) {
    return lm_lds_floats(n) + 2 * (size_t)lm_tri(n) + (size_t)n;
}
static_assert(lm_chain_lds_floats(LM_CHAIN_MAX_N) * 4 <= 64 * 1024, "the largest system must fit the workgroup's LDS");

struct LmChainArgs {
    int F, S, m, n, row_w_stride;
    float mu, smooth;
    const float* jac;       // (F,m,n)
    const float* r;         // (F,m)
    const float* prior;     // (F,n) or null
    const float* theta;     // (F,n); null only with smooth == 0
    const float* row_w;     // null, (m) with stride 0 or (F,m) with stride m
    const float* lambda;    // (S)
    const int* seq_starts;  // (S + 1)
    float* ws;              // (F, n (n + 1) / 2 + n)
    float* delta;           // (F,n)
};

__global__ __launch_bounds__(LM_T) void lm_chain_accumulate_kernel(LmChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, m = a.m, tid = threadIdx.x, ntri = lm_tri(n);
    const int f = blockIdx.x;
    // the sequence of f: the last q in [0, S) with seq_starts[q] <= f (every read inside the S + 1 entries)
    int lo = 0, hi = a.S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.seq_starts[mid] <= f) lo = mid; else hi = mid;
    }
    const int q = lo, fa = a.seq_starts[q], fb = a.seq_starts[q + 1];
    if (!(0 <= fa && fa <= f && f < fb && fb <= a.F)) return;   // the whole workgroup, before any barrier
    const LmLds s(smem, n);
    lm_clear(s, n);
    __syncthreads();
    lm_accumulate_body(s, a.jac + (size_t)f * m * n, a.r + (size_t)f * m,
                       a.row_w ? a.row_w + (size_t)f * a.row_w_stride : nullptr, m, n);
    const bool prev = f > fa, next = f + 1 < fb;
    const float c = (float)((int)prev + (int)next);
    // the coupling's share of the diagonal is in lm_damp's one argument; its share of the gradient joins g + mu prior
    // below, before the negation
    float g = lm_damp(s, n, (a.mu + a.lambda[q]) + a.smooth * c, a.mu, a.prior ? a.prior + (size_t)f * n : nullptr);
    if (tid < n) {
        const int i = tid;
        const size_t at = (size_t)f * n + i;
        if (a.smooth != 0.f && c != 0.f) {
            float t = c * a.theta[at];
            if (prev) t -= a.theta[at - n];
            if (next) t -= a.theta[at + n];
            g = g + a.smooth * t;
        }
        s.sG[i] = -g;
    }
    __syncthreads();
    float* o = a.ws + (size_t)f * (ntri + n);
    for (int e = tid; e < ntri + n; e += LM_T) o[e] = s.sN[e];
}

__global__ __launch_bounds__(LM_T) void lm_chain_sweep_kernel(LmChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = a.n, tid = threadIdx.x, ntri = lm_tri(n), w = ntri + n;
    const int q = blockIdx.x;
    const int fa = a.seq_starts[q], fb = a.seq_starts[q + 1];
    if (!(0 <= fa && fa < fb && fb <= a.F)) return;             // the whole workgroup, before any barrier
    const LmLds s(smem, n);
    float* sInv = smem + lm_lds_floats(n);   // S_{f-1}^-1, packed
    float* sM = sInv + ntri;                 // M = L_f^-1, packed lower triangle
    float* sX = sM + ntri;                   // x_{f-1}
    const float sm = a.smooth, nsm2 = -(sm * sm);
    const int i = tid;
    const bool own = i < n;
    if (tid == 0) s.sP[1] = 0.f;
    bool ok = true;
    // forward: S_f, y_f, L_f, x_f; from here thread i owns row i (n <= 96 < LM_T)
    for (int f = fa; f < fb; ++f) {
        float* row = a.ws + (size_t)f * w;
        const bool tied = sm != 0.f && f > fa;
        for (int e = tid; e < ntri; e += LM_T) s.sN[e] = tied ? fmaf(nsm2, sInv[e], row[e]) : row[e];
        float x = 0.f;
        if (own) {
            x = row[ntri + i];
            if (tied) x = fmaf(sm, sX[i], x);
        }
        __syncthreads();
        ok = lm_factor_solve(s, n, x);
        if (!ok) break;
        for (int e = tid; e < w; e += LM_T) row[e] = s.sN[e];   // L_f, then x_f (sG follows sN)
        if (sm == 0.f) {                                        // nothing ties the frames: x_f is delta_f
            if (own) a.delta[(size_t)f * n + i] = s.sG[i];
        } else if (f + 1 < fb) {
            if (own) {
                sX[i] = s.sG[i];
                // column c = i of M = L^-1: M[r][c] = (1[r == c] - sum_{c <= k < r} L[r][k] M[k][c]) / L[r][r],
                // k ascending; this thread reads and writes its own column only
                for (int r = i; r < n; ++r) {
                    const int tr = lm_tri(r);
                    float t = r == i ? 1.f : 0.f;
                    for (int k = i; k < r; ++k) t = fmaf(-s.sN[tr + k], sM[lm_tri(k) + i], t);
                    sM[tr + i] = t / s.sN[tr + r];
                }
            }
            __syncthreads();
            // S_f^-1 = M^T M: entry (p, j <= p) = sum_{k >= p} M[k][p] M[k][j], k ascending
            for (int e = tid; e < ntri; e += LM_T) {
                const int p = lm_untri(e), j = e - lm_tri(p);
                float acc = 0.f;
                for (int k = p; k < n; ++k) acc = fmaf(sM[lm_tri(k) + p], sM[lm_tri(k) + j], acc);
                sInv[e] = acc;
            }
        }
        __syncthreads();   // sInv, sX and the row are written; sN and sG are free again
    }
    if (!ok) {   // the same for every thread (lm_factor_solve)
        if (own) for (int f = fa; f < fb; ++f) a.delta[(size_t)f * n + i] = __builtin_nanf("");
        return;
    }
    if (sm == 0.f) return;
    // backward: delta_{b-1} = x_{b-1} (still in sG), then frames descending
    float d = own ? s.sG[i] : 0.f;
    if (own) a.delta[(size_t)(fb - 1) * n + i] = d;
    __syncthreads();
    for (int f = fb - 2; f >= fa; --f) {
        const float* row = a.ws + (size_t)f * w;
        for (int e = tid; e < ntri; e += LM_T) s.sN[e] = row[e];
        const float xf = own ? row[ntri + i] : 0.f;
        __syncthreads();
        lm_solve_factored(s, n, d);
        if (own) {
            d = fmaf(sm, s.sG[i], xf);
            a.delta[(size_t)f * n + i] = d;
        }
        __syncthreads();
    }
}

}  // namespace tik

using namespace tik_host;

extern "C" size_t tik_lm_chain_workspace_floats(int F, int n) {
    if (F <= 0 || n < 1) return 0;
    return (size_t)F * ((size_t)tik::lm_tri(n) + (size_t)n);
}

extern "C" int tik_lm_solve_chain(const float* jac, const float* r, const float* prior, const float* theta,
                                  const float* row_w, int row_w_stride, const float* lambda, const int* seq_starts,
                                  float mu, float smooth, int F, int S, int m, int n,
                                  float* workspace, float* delta, void* stream) {
    if (!jac || !r || !lambda || !seq_starts || !workspace || !delta)
        return fail(TIK_E_INVALID, "tik_lm_solve_chain: null pointer");
    if (F <= 0) return fail(TIK_E_INVALID, "tik_lm_solve_chain: F must be positive, got %d", F);
    if (S < 1 || S > F) return fail(TIK_E_INVALID, "tik_lm_solve_chain: S must be 1..F = %d, got %d", F, S);
    if (int rc = tik::lm_check_range("tik_lm_solve_chain", n, tik::LM_CHAIN_MAX_N, &m, &mu)) return rc;
    if (!(smooth >= 0.f)) return fail(TIK_E_INVALID, "tik_lm_solve_chain: smooth must be >= 0, got %g", (double)smooth);
    if (!theta && smooth != 0.f) return fail(TIK_E_INVALID, "tik_lm_solve_chain: theta may be null only with smooth == 0");
    if (row_w_stride != 0 && row_w_stride != m)
        return fail(TIK_E_INVALID, "tik_lm_solve_chain: row_w_stride must be 0 or m = %d, got %d", m, row_w_stride);
    const tik::LmChainArgs a{F, S, m, n, row_w_stride, mu, smooth, jac, r, prior, theta, row_w, lambda, seq_starts, workspace, delta};
    if (int rc = tik::lm_launch(tik::lm_chain_accumulate_kernel, F, tik::lm_lds_floats(n), stream, a)) return rc;
    return tik::lm_launch(tik::lm_chain_sweep_kernel, S, tik::lm_chain_lds_floats(n), stream, a);
}
