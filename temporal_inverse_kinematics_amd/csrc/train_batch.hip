// train_batch.hip — the two descriptor batches (train_dev.h's walk): every
// weight re-layout of a step in one launch, and the eval pass's BatchNorm fold
// of every layer in one launch. Both run once per weight version, not per
// batch, and are deliberately plain: a linear scan of the ~40 descriptors.
#include "train_dev.h"

namespace tik {

__global__ __launch_bounds__(256) void permute_batch_kernel(const PermDesc* __restrict__ descs, int nd) {
    batch_visit(descs, nd, [](const PermDesc& q, long long i) {
        const int i2 = (int)(i % q.d2);
        const long long r = i / q.d2;
        const int i1 = (int)(r % q.d1);
        const int i0 = (int)(r / q.d1);
        const long long so = q.soff + i0 * q.ss0 + i1 * q.ss1 + i2 * q.ss2;
        const float v = q.src[so];
        q.dst[i0 * q.ds0 + i1 * q.ds1 + i2 * q.ds2] = q.src2 ? v * q.src2[so] : v;
    });
}

long long permute_batch_blocks(PermDesc* descs, int nd) { return batch_blocks(descs, nd); }

hipError_t launch_permute_batch(const PermDesc* descs_dev, int nd, long long blocks, hipStream_t st) {
    if (nd == 0 || blocks == 0) return hipSuccess;
    return launch(permute_batch_kernel, (unsigned)blocks, 256, st, descs_dev, nd);
}

// ---------------------------------------------------------------- eval pass
// eval-mode BatchNorm of channel c as (scale, shift), the arithmetic of the
// host fold (api.cpp bn_fold): the scale in double, both rounded to fp32 once
__device__ __forceinline__ void bn_eval_affine(const BnRef& b, int c, float eps, float& sc, float& sh) {
    const double s = (double)b.gamma[c] / sqrt((double)b.var[c] + (double)eps);
    sc = (float)s;
    sh = (float)((double)b.beta[c] - (double)b.mean[c] * s);
}

// the eval set: one output element per visit; FOLD_BIAS2's 17-term column sum per thread
__global__ __launch_bounds__(256) void fold_batch_kernel(const FoldDesc* __restrict__ descs, int nd, float eps) {
    batch_visit(descs, nd, [eps](const FoldDesc& q, long long i) {
        const int r = (int)(i / q.cols), c = (int)(i % q.cols);
        float sc, sh;
        if (q.kind == FOLD_SCALE) {
            bn_eval_affine(q.bn, r, eps, sc, sh);
            q.dst[i] = sc * q.src[i];
        } else if (q.kind == FOLD_BIAS2) {
            bn_eval_affine(q.bn, c, eps, sc, sh);
            double colsum = 0.0;
            for (int v = 0; v < q.rows; ++v) colsum += (double)q.aux[v * q.rows + r];
            q.dst[i] = (float)((double)sc * (double)q.src[c] * colsum + (double)sh);
        } else if (q.kind == FOLD_BIAST) {
            bn_eval_affine(q.bn, c, eps, sc, sh);
            float b = (float)((double)sc * (double)q.src[c] + (double)sh);
            if (q.aux) {
                bn_eval_affine(q.bn2, c, eps, sc, sh);
                b += (float)((double)sc * (double)q.aux[c] + (double)sh);
            }
            q.dst[i] = b;
        } else {   // FOLD_DATA
            const int ch = q.cmap[c];
            sc = sh = 0.f;
            if (ch >= 0) bn_eval_affine(q.bn, ch, eps, sc, sh);
            q.dst[i] = r == 0 ? sc : sh;
        }
    });
}

long long fold_batch_blocks(FoldDesc* descs, int nd) { return batch_blocks(descs, nd); }

hipError_t launch_fold_batch(const FoldDesc* descs_dev, int nd, long long blocks, float eps, hipStream_t st) {
    if (nd == 0 || blocks == 0) return hipSuccess;
    return launch(fold_batch_kernel, (unsigned)blocks, 256, st, descs_dev, nd, eps);
}

}  // namespace tik
