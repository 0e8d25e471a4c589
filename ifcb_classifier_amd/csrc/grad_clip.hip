// Global gradient-norm clipping (TRAIN --clip-grad): torch.nn.utils.clip_grad_norm_(parameters, max_norm) on the flat gradient buffer.
// ifcbk_grad_norm leaves norm = grad_scale * sqrt(sum g^2) and coef = min(1, max_norm / (norm + 1e-6)) in device memory; adam_kernel /
// sgd_kernel (pool_head.hip) read coef from there and scale the gradient by grad_scale * coef, so the host never waits on the norm.
//
// grad_sumsq_kernel: HBM-bound, 4 B per element.  FIXED geometry, GRAD_CLIP_BLOCKS blocks of 256 threads whatever n is (4 blocks per CU
// of the 256): thread t of block b owns the float4s b * 256 + t + k * GRAD_CLIP_BLOCKS * 256, k = 0, 1, ..., and thread 0 of block 0 the
// n % 4 scalars of the tail, so which thread adds which element -- and with it every bit of the result -- depends on n alone.  A thread
// adds the squares of its float4s into four fp32 accumulators (one per component: four independent chains, loads of four float4s in
// flight), adds the four in fp32, and from there everything is fp64: the wave64 butterfly, the four wave sums through LDS, the block's
// partial, the sum of the partials.  No atomics: every block stores its partial, a block without an element stores 0, so nothing that
// the partial buffer held before the call can be read.  No element at or behind n is read.
// grad_clip_finalize_kernel: one wave; lane l adds partials l, l + 64, ... in that order, then the same butterfly.
#include "common.h"
#include <math.h>

namespace {

constexpr int GRAD_CLIP_BLOCKS = 1024;
constexpr int GRAD_CLIP_THREADS = 256;

// sum over the 64 lanes of a wave, the same order in every lane (xor butterfly): every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(GRAD_CLIP_THREADS) void grad_sumsq_kernel(const float* g, int64_t n, double* partials) {
    const int64_t nvec = n >> 2, stride = (int64_t)GRAD_CLIP_BLOCKS * GRAD_CLIP_THREADS;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int64_t i = (int64_t)blockIdx.x * GRAD_CLIP_THREADS + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        const float4 x0 = g4[i], x1 = g4[i + stride], x2 = g4[i + 2 * stride], x3 = g4[i + 3 * stride];
        a0 += x0.x * x0.x; a1 += x0.y * x0.y; a2 += x0.z * x0.z; a3 += x0.w * x0.w;
        a0 += x1.x * x1.x; a1 += x1.y * x1.y; a2 += x1.z * x1.z; a3 += x1.w * x1.w;
        a0 += x2.x * x2.x; a1 += x2.y * x2.y; a2 += x2.z * x2.z; a3 += x2.w * x2.w;
        a0 += x3.x * x3.x; a1 += x3.y * x3.y; a2 += x3.z * x3.z; a3 += x3.w * x3.w;
    }
    for (; i < nvec; i += stride) {
        const float4 x = g4[i];
        a0 += x.x * x.x; a1 += x.y * x.y; a2 += x.z * x.z; a3 += x.w * x.w;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t k = nvec << 2; k < n; ++k) a0 += g[k] * g[k];
    const double w = wave_sum((double)((a0 + a1) + (a2 + a3)));
    __shared__ double ws[GRAD_CLIP_THREADS / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__global__ __launch_bounds__(64) void grad_clip_finalize_kernel(const double* partials, float gscale, float max_norm, float* state) {
    double s = 0.0;
    for (int k = threadIdx.x; k < GRAD_CLIP_BLOCKS; k += 64) s += partials[k];
    s = wave_sum(s);
    if (threadIdx.x != 0) return;
    // the one rounding to fp32; from here torch's own fp32 arithmetic: clip_coef = max_norm / (total_norm + 1e-6) clamped to 1, which a
    // torch tensor evaluates as reciprocal(total_norm + 1e-6) * max_norm (Tensor.__rtruediv__), two roundings -- the same here, so that
    // the coefficient of a given fp32 norm has torch's bits.  A non-finite norm is not special-cased: inf gives coef 0, NaN gives NaN
    // (NaN > 1 is false), as torch's error_if_nonfinite=False
    const float norm = (float)((double)gscale * sqrt(s));
    const float c = (1.f / (norm + 1e-6f)) * max_norm;
    const float coef = c > 1.f ? 1.f : c;
    state[0] = norm;
    state[1] = coef;
    if (norm > state[2]) state[2] = norm;
    if (coef < 1.f) state[3] += 1.f;
}

}  // namespace

extern "C" size_t ifcbk_grad_clip_state_floats(void) { return 4 + 2 * (size_t)GRAD_CLIP_BLOCKS; }

extern "C" int ifcbk_grad_norm(ifcbk_ctx* ctx, const float* g, int64_t n, float grad_scale, float max_norm, float* state, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!g || !state) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_norm: g or state is NULL");
    if (((uintptr_t)g & 15) || ((uintptr_t)state & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_norm: g and state must be 16-byte aligned");
    if (n < 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_norm: n %lld < 0", (long long)n);
    if (!(max_norm > 0.f && max_norm <= 3.402823466e+38f)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_norm: max_norm %g must be finite and > 0", (double)max_norm);      // (a NaN fails the comparisons)
    if (!(grad_scale > 0.f && grad_scale <= 3.402823466e+38f)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "grad_norm: grad_scale %g must be finite and > 0", (double)grad_scale);
    double* partials = reinterpret_cast<double*>(state + 4);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(GRAD_CLIP_BLOCKS), dim3(GRAD_CLIP_THREADS), 0, (hipStream_t)stream, g, n, partials);
    IFCBK_LAUNCH_CHECK(ctx, "grad_sumsq");
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, grad_scale, max_norm, state);
    IFCBK_LAUNCH_CHECK(ctx, "grad_clip_finalize");
    return IFCBK_OK;
}
