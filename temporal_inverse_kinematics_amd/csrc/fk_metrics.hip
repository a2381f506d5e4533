// fk_metrics.hip — the pose metrics of a frame in ONE launch (tik_fk_pose_metrics): one workgroup of LM_T = 256 threads per
// frame, everything about the frame in LDS and registers. Per frame f (= rows[b], or b), k < 17 keypoints:
//
//   x_k = rel(FK keypoints(th_f, beta_f)),  y_k = rel(kps_f),  w_k the frame's weights      rel(x) = x - mean of columns 11 / 12
//   W = sum_k w_k,  n = #{k : w_k > 0}
//   out[f][0] mpjpe    = sum_k w_k |x_k - y_k| / W                                          NaN when W = 0
//   out[f][1] pa_mpjpe = sum_k w_k |s R (x_k - mx) - (y_k - my)| / W                        NaN when n < 3
//             mx, my the w-weighted means, R in SO(3) the proper rotation that minimises sum w |s R (x - mx) - (y - my)|^2
//             (Horn 1987), s = sum w (y - my) . R (x - mx) / sum w |x - mx|^2
//   out[f][2] mpjae    = (1/22) sum_{j<22} angle(R_j^T R*_j), R_j = rodrigues_smplx(th_j + pose_mean_j), R*_j the same of
//             target_poses; angle = atan2(|axial(D)|, (tr D - 1) / 2)                       NaN without target_poses
//   out[f][3] weight   = W
//   joints_out[f][k] = x_k (optional)
// A pose value that is not finite gives NaN in all four columns whatever the selection (the pose's mark is added to each;
// the weight included: a mean over W > 0 leaves the frame out).
//
// Phases (frame_setup and fk_eval are lm_refine_dev.h's, the same instructions as in lm_refine_kernel):
//   0  frame_setup: pose, rel(kps), weights (joint_w, the skip rule), betas, the selection, the rest joints    2 barriers
//   1  threads 64 .. 85: R_j of the pose; threads 128 .. 149: R*_j of the target; one rodrigues_smplx in the code, so
//      equal values give equal bits and a pose against itself has the angle 0 exactly. Both into the LDS slab Lds::dR
//      (linearize's, not used here otherwise). No barrier of its own: fk_eval's publish them.
//   2  fk_eval: Rodrigues, the chain by tree depth, the vertex keypoints' blend and skinning, r     maxdepth + 6 barriers
//   3  wave 0 alone, lane k < 17 holds w_k, x_k, y_k (the other lanes zeros), lane j < 22 the angle of
//      R_j^T R*_j (0 without a target) and the pose's mark 0 * R_j[0][0] (NaN for a pose that is not finite). Every sum over the keypoints or the joints
//      is wave_sum, the fixed butterfly: W, n, the angles, the pose's NaN mark, the mpjpe terms, 3 + 3 for the means, 9 + 1 for
//      sum w (x - mx)(y - my)^T and sum w |x - mx|^2, then the scale's numerator and the pa terms: 24 butterflies,
//      the same bits in every lane. Between them every lane runs the same alignment in registers: Horn's 4x4
//      symmetric matrix of the nine sums, FKM_SWEEPS cyclic Jacobi sweeps over its six (p,q) pairs (unrolled at compile
//      time; each pair a rotation by t = sgn(h) / (|h| + sqrt(h^2 + 1)), h = (a_qq - a_pp) / (2 a_pq), t = 0 where
//      a_pq = 0), the eigenvector of the largest diagonal entry picked by selects, normalised, turned into R.
//      Lane 0 writes the four values, lane k its x_k.
// No loop bound depends on data and nothing runs until converged: a NaN falls through to the output. One FK state and
// no lm_dev.h slabs: lds_frame_floats(K, 1) floats of LDS as fk_kploss_kernel (J is carved and not used). No atomics,
// every output element has one writer, and a workgroup sees only its own frame: a frame's bits do not depend on B, on
// its place in the batch or on rows.
#include <cmath>

#include "fk_metrics.h"
#include "fk_model.h"
#include "lm_refine_dev.h"

namespace tik {
namespace {

// One Jacobi rotation in the (P,Q) plane of the symmetric A (both triangles kept), accumulated into the columns of V
template <int P, int Q>
__device__ __forceinline__ void jacobi_pair(float (&A)[4][4], float (&V)[4][4]) {
    const float apq = A[P][Q];
    const float h = (A[Q][Q] - A[P][P]) / (2.f * apq);
    float t = copysignf(1.f, h) / (fabsf(h) + sqrtf(fmaf(h, h, 1.f)));
    t = apq == 0.f ? 0.f : t;              // NaN == 0 is false: a NaN matrix keeps its NaN
    const float c = 1.f / sqrtf(fmaf(t, t, 1.f)), s = t * c;
    A[P][P] = fmaf(-t, apq, A[P][P]);
    A[Q][Q] = fmaf(t, apq, A[Q][Q]);
    A[P][Q] = A[Q][P] = 0.f;               // a NaN a_pq has gone into both diagonal entries
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const float arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = fmaf(c, arp, -s * arq);
            A[r][Q] = A[Q][r] = fmaf(s, arp, c * arq);
        }
        const float vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = fmaf(c, vrp, -s * vrq);
        V[r][Q] = fmaf(s, vrp, c * vrq);
    }
}

// The proper rotation R (row-major) that maximises sum w y . R x, from M[3a+b] = sum w x_a y_b (Horn's quaternion form)
__device__ __forceinline__ void horn_rotation(const float M[9], float R[9]) {
    const float Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
    float A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                     {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                     {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                     {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    float V[4][4] = {{1.f, 0.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 1.f, 0.f}, {0.f, 0.f, 0.f, 1.f}};
#pragma unroll
    for (int sweep = 0; sweep < FKM_SWEEPS; ++sweep) {
        jacobi_pair<0, 1>(A, V); jacobi_pair<0, 2>(A, V); jacobi_pair<0, 3>(A, V);
        jacobi_pair<1, 2>(A, V); jacobi_pair<1, 3>(A, V); jacobi_pair<2, 3>(A, V);
    }
    // the column of the largest eigenvalue, by selects (the first of equal ones)
    float best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int m = 1; m < 4; ++m) {
        const bool up = A[m][m] > best;
        best = up ? A[m][m] : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = up ? V[i][m] : q[i];
    }
    // a NaN anywhere in the matrix must reach R whichever column the selects took
    const float poison = 0.f * (A[0][0] + A[1][1] + A[2][2] + A[3][3]);
    const float inv = 1.f / sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0]))));
    const float q0 = q[0] * inv + poison, qx = q[1] * inv, qy = q[2] * inv, qz = q[3] * inv;
    R[0] = q0 * q0 + qx * qx - qy * qy - qz * qz; R[1] = 2.f * (qx * qy - q0 * qz); R[2] = 2.f * (qx * qz + q0 * qy);
    R[3] = 2.f * (qy * qx + q0 * qz); R[4] = q0 * q0 - qx * qx + qy * qy - qz * qz; R[5] = 2.f * (qy * qz - q0 * qx);
    R[6] = 2.f * (qz * qx - q0 * qy); R[7] = 2.f * (qz * qy + q0 * qx); R[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
}

// angle of A^T B in radians, sound at 0 and at pi: atan2(|axial(D)|, (tr D - 1) / 2), D = A^T B
__device__ __forceinline__ float rotation_angle(const float A[9], const float B[9]) {
    float D[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) D[3 * r + c] = fmaf(A[6 + r], B[6 + c], fmaf(A[3 + r], B[3 + c], A[r] * B[c]));
    const float a0 = 0.5f * (D[7] - D[5]), a1 = 0.5f * (D[2] - D[6]), a2 = 0.5f * (D[3] - D[1]);
    return atan2f(sqrtf(fmaf(a2, a2, fmaf(a1, a1, a0 * a0))), 0.5f * (D[0] + D[4] + D[8] - 1.f));
}

}  // namespace

__global__ __launch_bounds__(LM_T) void fk_metrics_kernel(FkMetricsArgs a) {
    using namespace lmr;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const size_t f = a.rows ? (size_t)a.rows[blockIdx.x] : (size_t)blockIdx.x;
    const int K = skin_count(a);
    const Lds s(smem, K, 1);
    int dj, par;
    frame_setup(a, s, a.poses + f * a.poses_ld, nullptr, nullptr, false, a.kps + f * M, nullptr, a.skip != 0, f, K, 1, dj, par);
    {   // phase 1: wave 1 the pose's rotations, wave 2 the target's, by the same instructions, into the dR slab
        const int g = tid >> 6, j = tid & 63;
        if ((g == 1 || (g == 2 && a.target_poses)) && j < ND) {
            float v[3], Rr[9];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c] = (g == 1 ? s.th[3 * j + c] : a.target_poses[f * a.target_ld + 3 * j + c]) + a.pose_mean[3 * j + c];
            rodrigues_smplx(v[0], v[1], v[2], Rr);
            float* o = s.dR + (g - 1) * (ND * 9) + 9 * j;
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = Rr[e];
        }
    }
    float* S = s.state(0);
    fk_eval(a, s, S, s.th, dj, par, K);
    if (tid >= 64) return;
    // phase 3: wave 0
    const int k = tid;
    float ang = 0.f, mark = 0.f;
    if (k < ND) {
        float Rj[9], Rt[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Rj[e] = s.dR[9 * k + e];
        mark = 0.f * Rj[0];                                 // 0, or NaN for a pose that is not finite
        if (a.target_poses) {
#pragma unroll
            for (int e = 0; e < 9; ++e) Rt[e] = s.dR[ND * 9 + 9 * k + e];
            ang = rotation_angle(Rj, Rt);
        }
    }
    const float asum = wave_sum(ang), bad = wave_sum(mark);
    float w = 0.f, x[3] = {0.f, 0.f, 0.f}, y[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
    if (k < NC) {
        w = s.rw[3 * k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = S[ST_XJ + 3 * k + c] - 0.5f * (S[ST_XJ + 33 + c] + S[ST_XJ + 36 + c]);
            y[c] = s.tgt[3 * k + c];
            d[c] = S[ST_R + 3 * k + c];
        }
    }
    const float W = wave_sum(w), n = wave_sum(w > 0.f ? 1.f : 0.f);
    const float e = wave_sum(w * sqrtf(sq_norm3(d)));
    float mx[3], my[3], xc[3], yc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mx[c] = wave_sum(w * x[c]) / W;
        my[c] = wave_sum(w * y[c]) / W;
        xc[c] = x[c] - mx[c];
        yc[c] = y[c] - my[c];
    }
    float Mxy[9], Rm[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Mxy[3 * r + c] = wave_sum(w * xc[r] * yc[c]);
    const float sxx = wave_sum(w * sq_norm3(xc));
    horn_rotation(Mxy, Rm);
    float rx[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) rx[r] = fmaf(Rm[3 * r + 2], xc[2], fmaf(Rm[3 * r + 1], xc[1], Rm[3 * r] * xc[0]));
    const float sc = wave_sum(w * fmaf(yc[2], rx[2], fmaf(yc[1], rx[1], yc[0] * rx[0]))) / sxx;
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = fmaf(sc, rx[c], -yc[c]);
    const float pa = wave_sum(w * sqrtf(sq_norm3(q)));
    const float nan = __uint_as_float(0x7fc00000u);
    if (k == 0) {
        float* o = a.out + f * FKM_COLS;
        o[0] = e / W + bad;                                 // 0 / 0 = NaN when W = 0; bad is 0, or NaN with the pose
        o[1] = n < 3.f ? nan : pa / W + bad;
        o[2] = a.target_poses ? asum * (1.f / ND) : nan;
        o[3] = W + bad;
    }
    if (a.joints_out && k < NC) {
        float* o = a.joints_out + f * M + 3 * k;
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
    }
}

int fk_metrics_args(const tik_fk* fk, const char* who, const float* poses, int poses_ld, const float* kps, const float* betas,
                    int betas_ld, const float* joint_w, int joint_w_ld, const float* target_poses, int target_ld,
                    const int* sel17, const int* rows, int B, int flags, float* out, float* joints_out, FkMetricsArgs& a) {
    using namespace tik_host;
    if (!fk || !poses || !kps || !out) return fail(TIK_E_INVALID, "%s: null pointer", who);
    if (B <= 0) return fail(TIK_E_INVALID, "%s: B must be positive, got %d", who, B);
    if (poses_ld < LMR_N) return fail(TIK_E_INVALID, "%s: poses_ld must be >= %d, got %d", who, LMR_N, poses_ld);
    if (target_poses && target_ld < LMR_N) return fail(TIK_E_INVALID, "%s: target_ld must be >= %d, got %d", who, LMR_N, target_ld);
    if (betas && betas_ld != 0 && betas_ld < fk->nb)
        return fail(TIK_E_INVALID, "%s: betas_ld must be 0 (one row for all frames) or >= %d, got %d", who, fk->nb, betas_ld);
    if (joint_w && joint_w_ld != 0 && joint_w_ld != LMR_COLS)
        return fail(TIK_E_INVALID, "%s: joint_w_ld must be 0 (shared) or 17 (per frame), got %d", who, joint_w_ld);
    if (flags & ~TIK_REFINE_SKIP_NONFINITE) return fail(TIK_E_INVALID, "%s: unknown bits in flags: 0x%x", who, (unsigned)flags);
    LmRefineArgs m;
    if (int rc = lm_refine_model_args(fk, who, sel17, 0, 1.f, 0.f, 1.f, m)) return rc;   // the LM scalars are unused
    a = FkMetricsArgs{};
    static_cast<LmRefineArgs&>(a) = m;
    a.B = B;
    a.poses = poses; a.poses_ld = poses_ld; a.kps = kps;
    a.betas = betas; a.betas_ld = betas_ld; a.joint_w = joint_w; a.joint_w_ld = joint_w_ld;
    a.target_poses = target_poses; a.target_ld = target_ld;
    a.rows = rows; a.out = out; a.joints_out = joints_out; a.skip = (flags & TIK_REFINE_SKIP_NONFINITE) ? 1 : 0;
    return TIK_OK;
}

int fk_metrics_launch(const FkMetricsArgs& a, void* stream) {
    return lm_launch(fk_metrics_kernel, a.B, lmr::lds_frame_floats(a.nz > 0 ? a.nz : 55, 1), stream, a);
}

}  // namespace tik

extern "C" int tik_fk_pose_metrics(tik_fk_t fk, const float* poses, int poses_ld, const float* kps, const float* betas,
                                   int betas_ld, const float* joint_w, int joint_w_ld, const float* target_poses, int target_ld,
                                   const int* sel17, const int* rows, int B, int flags, float* out, float* joints_out,
                                   void* stream) {
    tik::FkMetricsArgs a;
    if (int rc = tik::fk_metrics_args(fk, "tik_fk_pose_metrics", poses, poses_ld, kps, betas, betas_ld, joint_w, joint_w_ld,
                                      target_poses, target_ld, sel17, rows, B, flags, out, joints_out, a))
        return rc;
    return tik::fk_metrics_launch(a, stream);
}
