// Gradient accumulation over a flat fp32 buffer (TRAIN --accumulate): ifcbk_grad_accum_flat sums the gradient g of one batch into the
// accumulator a.  first != 0: a[i] = g[i] -- the old bits of a are never read, so a NaN left there does not survive and the caller never
// zeroes the accumulator; first == 0: a[i] = a[i] + g[i], ONE fp32 add per element (no FMA, no reassociation, no atomics): the bits of
// torch's fp32 a + g, and K calls leave the left-to-right sum ((g1 + g2) + g3) ...  The engine calls it between programs, once per batch
// behind backward (the whole of G), and per finished bucket [lo, hi) in the last data-parallel micro-step; the optimizer op of an
// accumulating engine then reads a through its G operand with grad_scale = 1 / K.
// HBM-bound, 12 B per element (8 when first): one 16-byte load of a and of g and one 16-byte store per thread, scalar tail for n % 4; the
// grid shape of ema_kernel / adam_kernel.  a and g are 16-byte aligned (whole torch allocations, or slices at a multiple of 4 elements).
// No element at or behind n is read or written; g is never written.
#include "common.h"

namespace {

template <bool FIRST>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* a, const float* g, int64_t n) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        float4 gg = *reinterpret_cast<const float4*>(g + i);
        if (!FIRST) {
            float4 aa = *reinterpret_cast<const float4*>(a + i);
            gg.x = aa.x + gg.x; gg.y = aa.y + gg.y; gg.z = aa.z + gg.z; gg.w = aa.w + gg.w;
        }
        *reinterpret_cast<float4*>(a + i) = gg;
    } else {
        for (int64_t k = i; k < n; ++k) a[k] = FIRST ? g[k] : a[k] + g[k];
    }
}

}  // namespace

extern "C" int ifcbk_grad_accum_flat(ifcbk_ctx* ctx, float* a, const float* g, int64_t n, int first, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!a || !g) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_accum: a or g is NULL");
    if (n < 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_accum: n %lld < 0", (long long)n);
    if (((uintptr_t)a & 15) || ((uintptr_t)g & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_accum: a and g must be 16-byte aligned");
    if (a == g) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_accum: a and g are the same buffer");
    if (n == 0) return IFCBK_OK;
    dim3 grid(cdiv(cdiv(n, 4), 256)), block(256);
    if (first)
        hipLaunchKernelGGL(grad_accum_kernel<true>, grid, block, 0, (hipStream_t)stream, a, g, n);
    else
        hipLaunchKernelGGL(grad_accum_kernel<false>, grid, block, 0, (hipStream_t)stream, a, g, n);
    IFCBK_LAUNCH_CHECK(ctx, "grad_accum");
    return IFCBK_OK;
}
