// api.cpp — the thin part of libtik.so's C ABI (include/tik.h): last error and
// version, the precision and profile getters and setters, and the four
// stand-alone ops. The handles are built in model.cpp (fold.h first), the
// forward pass is launched from forward.cpp, the debug hooks are in debug.cpp.
#include <hip/hip_runtime.h>

#include "misc.h"
#include "model.h"

using namespace tik_host;

extern "C" {

const char* tik_last_error(void) { return g_err.c_str(); }
const char* tik_version(void) { return "tik 0.4.0 (gfx950; bf16x3 split MFMA (default, fp32 range), exact fp32 MFMA)"; }

int tik_model_set_precision(tik_model_t m, int prec) {
    if (!m || (prec != tik::PREC_F32 && prec != tik::PREC_BF16X3))
        return fail(TIK_E_INVALID, "tik_model_set_precision: precision must be 0 (fp32) or 2 (bf16x3), got %d", prec);
    m->prec = prec;
    return TIK_OK;
}

int tik_model_get_precision(tik_model_t m) {
    if (!m) return fail(TIK_E_INVALID, "null model");
    return m->prec;
}

int tik_block_set_precision(tik_block_t b, int prec) {
    if (!b || (prec != tik::PREC_F32 && prec != tik::PREC_BF16X3))
        return fail(TIK_E_INVALID, "tik_block_set_precision: precision must be 0 (fp32) or 2 (bf16x3), got %d", prec);
    b->prec = prec;
    return TIK_OK;
}

int tik_model_profile(tik_model_t m, int max_launches) {
    if (!m || max_launches < 0) return fail(TIK_E_INVALID, "tik_model_profile: bad arguments");
    m->profiling = max_launches > 0;
    return max_launches > 0 ? m->prof.enable(max_launches) : (m->prof.clear(), TIK_OK);
}

int tik_model_profile_count(tik_model_t m) {
    if (!m) return fail(TIK_E_INVALID, "null model");
    return (int)m->prof.recs.size();
}

int tik_model_profile_read(tik_model_t m, int i, char* label, int label_len, float* ms, double* flops,
                           double* bytes) {
    if (!m) return fail(TIK_E_INVALID, "tik_model_profile_read: null model");
    return m->prof.read(i, label, label_len, ms, flops, bytes);
}

// ---------------------------------------------------------------------------- ops
int tik_gconv_fwd(const float* x, int N, int Cin, int T, int V, const float* A, int K, const float* W,
                  const float* b, int Cout, int t_kernel, int t_stride, int t_padding, int t_dilation, float* out,
                  void* stream) {
    if (!x || !A || !W || !out || N <= 0 || Cin <= 0 || T <= 0 || V <= 0 || K <= 0 || Cout <= 0 || t_kernel <= 0 ||
        t_stride <= 0 || t_padding < 0 || t_dilation <= 0)
        return fail(TIK_E_INVALID, "tik_gconv_fwd: bad arguments");
    const int To = (T + 2 * t_padding - t_dilation * (t_kernel - 1) - 1) / t_stride + 1;
    if (To <= 0) return fail(TIK_E_INVALID, "tik_gconv_fwd: empty temporal output");
    if ((size_t)K * Cout * V * sizeof(float) > 160 * 1024)
        return fail(TIK_E_INVALID, "tik_gconv_fwd: K*Cout*V=%d exceeds the per-frame LDS tile", K * Cout * V);
    HIP_TRY(tik::launch_gconv(x, N, Cin, T, V, A, K, W, b, Cout, t_kernel, t_stride, t_padding, t_dilation, To, out,
                              (hipStream_t)stream));
    return TIK_OK;
}

int tik_aa_to_rotmat(const float* aa, int n, float* R, void* stream) {
    if (!aa || !R || n < 0) return fail(TIK_E_INVALID, "tik_aa_to_rotmat: bad arguments");
    HIP_TRY(tik::launch_aa_to_rotmat(aa, n, R, (hipStream_t)stream));
    return TIK_OK;
}

int tik_moveai_to_coco(const float* joints, int F, int J, const int* map17_host, float* out, void* stream) {
    if (!joints || !map17_host || !out || F < 0 || J < 2) return fail(TIK_E_INVALID, "tik_moveai_to_coco: bad arguments");
    for (int c = 0; c < 17; ++c)
        if (map17_host[c] < -1 || map17_host[c] >= J)
            return fail(TIK_E_INVALID, "tik_moveai_to_coco: map entry %d = %d out of range for %d joints", c, map17_host[c], J);
    HIP_TRY(tik::launch_moveai_to_coco(joints, F, J, map17_host, out, (hipStream_t)stream));
    return TIK_OK;
}

int tik_window_gather(const float* seq, int F, int V, int idx0, int n_idx, int h, int root_a, int root_b,
                      int relative, float* windows, void* stream) {
    if (!seq || !windows || F <= 0 || V <= 0 || n_idx < 0 || h < 0 || idx0 < 0 || idx0 + n_idx > F)
        return fail(TIK_E_INVALID, "tik_window_gather: bad arguments");
    if (relative && (root_a < 0 || root_a >= V || root_b < 0 || root_b >= V))
        return fail(TIK_E_INVALID, "tik_window_gather: root joints out of range");
    // data_amass.py:27-29 raises when h > idx > F - h; a window that overruns
    // both ends of a short sequence comes back shorter than 2h+1 there.
    for (int i = idx0; i < idx0 + n_idx; ++i) {
        if (h > i && i > F - h)
            return fail(TIK_E_INVALID, "h_win_size > idx > arr.shape[0] - h_win_size: %d > %d > %d - %d", h, i, F, h);
        if (i - h < 0 && i + h > F - 1 && i <= F - h)
            return fail(TIK_E_INVALID, "window at idx %d overruns both ends (reference returns a short window)", i);
    }
    HIP_TRY(tik::launch_window_gather(seq, F, V, idx0, n_idx, h, root_a, root_b, relative, windows,
                                      (hipStream_t)stream));
    return TIK_OK;
}

}  // extern "C"
