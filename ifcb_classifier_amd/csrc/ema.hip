// Exponential moving average of a flat fp32 buffer (TRAIN --ema): ifcbk_ema_flat applies e <- e + w * (x - e), the lerp form of
// torch.optim.swa_utils.get_ema_multi_avg_fn and timm's ModelEmaV3, whose fixed point is x itself (d * e + (1 - d) * x with two rounded
// scalars has the fixed point x (1 - d) / (1 - fl(d))).  The parameters' average is taken INSIDE adam_kernel / sgd_kernel
// (pool_head.hip), from the p those kernels hold in registers; this plain form serves the buffers no optimizer kernel streams: the
// BatchNorm running statistics, once per step.
// HBM-bound, 12 B per element: one 16-byte load of e and of x and one 16-byte store per thread, scalar tail; the grid shape of
// adam_kernel.  e and x are 16-byte aligned (whole torch allocations).  No element at or behind n is read or written.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void ema_kernel(float* e, const float* x, int64_t n, float w) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        float4 ee = *reinterpret_cast<float4*>(e + i), xx = *reinterpret_cast<const float4*>(x + i);
        float* E = &ee.x; float* X = &xx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) E[j] = E[j] + w * (X[j] - E[j]);
        *reinterpret_cast<float4*>(e + i) = ee;
    } else {
        for (int64_t k = i; k < n; ++k) e[k] = e[k] + w * (x[k] - e[k]);
    }
}

}  // namespace

extern "C" int ifcbk_ema_flat(ifcbk_ctx* ctx, float* e, const float* x, int64_t n, float w, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!e || !x) IFCBK_FAIL(ctx, IFCBK_EINVAL, "ema: e or x is NULL");
    if (n < 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "ema: n %lld < 0", (long long)n);
    if (!(w >= 0.f && w <= 1.f)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "ema: w %g outside [0, 1]", (double)w);      // (a NaN fails the comparisons)
    if (((uintptr_t)e & 15) || ((uintptr_t)x & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "ema: e and x must be 16-byte aligned");
    if (n == 0 || w == 0.f) return IFCBK_OK;          // w == 0 is "no update": e keeps its bits, a -0 included
    hipLaunchKernelGGL(ema_kernel, dim3(cdiv(cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, e, x, n, w);
    IFCBK_LAUNCH_CHECK(ctx, "ema");
    return IFCBK_OK;
}
