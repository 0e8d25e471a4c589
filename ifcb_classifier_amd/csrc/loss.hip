// Class-weighted cross-entropy: nn.CrossEntropyLoss(weight=w), mean reduction (TRAIN --class-norm).  The unweighted loss keeps its
// own kernel and entry point (pool_head.hip); this file is reached only when the engine holds class weights.
#include "common.h"
#include <math.h>

namespace {

// softmax_xent_kernel's shape -- one 1024-thread block, 4 lanes per sample (classes j = sub, sub+4, ...), fixed butterflies, fixed-order
// final sum: bitwise reproducible -- behind a pre-pass for the normaliser W = sum_n w[t_n]: per-slot partial sums in LDS (slot s takes
// the samples s, s + 256, ... in order), summed in slot order by thread 0 and broadcast.
//   c_n = weight * (w[t_n] / W),   d[n][j] = c_n * (p[n][j] - onehot),   loss = (sum_slots sum_n w[t_n] l_n) * (1 / W) * weight
// With all-ones class weights W == N exactly (a sum of ones below 2^24) and 1 / W == 1.f / N, so every operation has the operands
// it has in softmax_xent_kernel: loss and dlogits are then bit-equal to the unweighted kernel's.
// A target outside [0, NC) is the caller's fault, as there.
__global__ __launch_bounds__(1024) void softmax_xent_w_kernel(const float* logits, const int64_t* target, const float* class_weight,
                                                              int N, int NC, float weight, float* loss_out, int loss_acc,
                                                              float* dlogits) {
    __shared__ float sl[256];
    __shared__ float sW;
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2;
    if (sub == 0) {
        float wsum = 0.f;
        for (int n = slot; n < N; n += 256) wsum += class_weight[(int)target[n]];
        sl[slot] = wsum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += sl[i];
        sW = s;
    }
    __syncthreads();
    const float W = sW;
    const float invW = 1.f / W;
    float local = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        float mx = -INFINITY;
        for (int j = sub; j < NC; j += 4) mx = fmaxf(mx, l[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        float s = 0.f;
        for (int j = sub; j < NC; j += 4) s += expf(l[j] - mx);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        const int tg = ok ? (int)target[n] : 0;
        const float wt = ok ? class_weight[tg] : 0.f;
        if (ok && sub == 0) {
            const float li = mx + logf(s) - l[tg];
            local += wt * li;
        }
        if (ok && dlogits) {
            float* d = dlogits + (size_t)n * NC;
            const float is = 1.f / s;
            const float c = weight * (wt / W);
            for (int j = sub; j < NC; j += 4) d[j] = c * (expf(l[j] - mx) * is - (j == tg ? 1.f : 0.f));
        }
    }
    __syncthreads();                       // (thread 0 has finished reading the W partials)
    if (sub == 0) sl[slot] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += sl[i];
        s = s * invW * weight;
        loss_out[0] = loss_acc ? loss_out[0] + s : s;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int ifcbk_softmax_xent_w(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* class_weight, int N, int NC,
                                    float weight, float* loss_out, int loss_accumulate, float* dlogits, void* stream) {
    if (N <= 0 || NC <= 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_w: empty");
    if (!class_weight) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_w: class_weight is NULL (the unweighted loss is ifcbk_softmax_xent)");
    if (!logits || !target || !loss_out) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_w: NULL operand");
    hipLaunchKernelGGL(softmax_xent_w_kernel, dim3(1), dim3(1024), 0, ST, logits, target, class_weight, N, NC, weight, loss_out,
                       loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_w");
    return IFCBK_OK;
}
