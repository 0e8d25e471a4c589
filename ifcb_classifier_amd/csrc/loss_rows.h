// The row reduction that the six fused loss kernels share: softmax_xent_kernel (pool_head.hip) and softmax_xent_w / _ls / _focal /
// _mix / _distill_kernel (loss.hip).
//
// The shape, stated here once.  A loss kernel is ONE block of 1024 threads.  Four adjacent lanes (a quad) share a sample: lane
// sub = tid & 3 of slot = tid >> 2 takes the classes j = sub, sub + 4, ..., so adjacent lanes read adjacent logits, and a round of the
// sample loop covers LOSS_SLOTS = 256 samples (slot s takes the samples s, s + 256, ... in order).  A row quantity is reduced over its
// quad by a fixed two-step butterfly, after which all four lanes hold the same bits.  A block quantity (the normaliser W, the class sum
// SW, the loss) is reduced in two fixed stages: each slot's partial goes to LDS, and thread 0 adds the 256 partials in slot order.  No
// atomics, no order that depends on timing: every output is bitwise reproducible, and two kernels that put the same operands through
// these pieces produce the same bits (with all-ones class weights softmax_xent_w_kernel's outputs are softmax_xent_kernel's).
//
// The library is built with -ffp-contract=on: a multiply and an add fuse exactly when they stand in one source expression, and inlining
// does not change that.  So every piece here takes over WHOLE statements of the kernels: it accumulates through a reference or returns the
// finished value, and an argument that is a product is consumed only by a multiply.  What could not be cut that way stays in the kernels:
//   - the sample loop `for (int n0 = 0; n0 < N; n0 += 256)` and the row's address: the pieces work on a row, not on the loop;
//   - the fused loops of _focal (s and so from one expf) and _distill (mx with mz; s, sr, sq; q with kl): they call the butterflies and
//     smooth_q_add on their own accumulators;
//   - _mix's dlogits element, the two-target form `A p - [j == a] ha - [j == b] hb - eC w[j]`: a second one-hot term inside the chain of
//     subtractions; passing it a zero through smooth_dlogit would be a mode flag;
//   - each slot's pre-pass partial (_mix sums h_n, the others w[t_n]): the caller forms it and passes it in;
//   - _distill's final pair of sums: slot_put2 and two slot_total calls, since a broadcast there would add a barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

constexpr int LOSS_SLOTS = 256;          // samples per round: 1024 threads / 4 lanes

__device__ __forceinline__ int loss_sub() { return threadIdx.x & 3; }
__device__ __forceinline__ int loss_slot() { return threadIdx.x >> 2; }

// ---------------------------------------------------------------- a quad
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    return fmaxf(v, __shfl_xor(v, 2));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 1);
    return v + __shfl_xor(v, 2);
}

// ---------------------------------------------------------------- a row
__device__ __forceinline__ float row_max(const float* l, int NC, int sub) {
    float mx = -INFINITY;
    for (int j = sub; j < NC; j += 4) mx = fmaxf(mx, l[j]);
    return quad_max(mx);
}
// >= 1: the row's maximum contributes expf(0) == 1 to a sum of non-negative terms
__device__ __forceinline__ float row_expsum(const float* l, float mx, int NC, int sub) {
    float s = 0.f;
    for (int j = sub; j < NC; j += 4) s += expf(l[j] - mx);
    return quad_sum(s);
}

// class_weight == NULL: all ones
__device__ __forceinline__ float class_w(const float* class_weight, int j) { return class_weight ? class_weight[j] : 1.f; }

// ---------------------------------------------------------------- label smoothing (_ls, _mix, _distill)
// The smoothing term sum_j w[j] (-log p[j]) is summed as the non-negative pieces w[j] * ((mx - l[j]) + log s): mx >= l[j] and s >= 1;
// sum w * lse - sum w * l would cancel.  One piece (a subtract, an add, a multiply-add), ls = logf(s):
__device__ __forceinline__ void smooth_q_add(float& q, float wj, float mx, float lj, float ls) { q += wj * ((mx - lj) + ls); }
__device__ __forceinline__ float smooth_q(const float* l, const float* class_weight, float mx, float ls, int NC, int sub) {
    float q = 0.f;
    for (int j = sub; j < NC; j += 4) smooth_q_add(q, class_w(class_weight, j), mx, l[j], ls);
    return quad_sum(q);
}
// One element of the smoothed hard gradient, g * (A p - [j == t] hard - eC w[j]) with g = weight / W, A = hard + eC SW, p the softmax
// and hot = (j == t ? hard : 0): a multiply-subtract, a multiply-subtract, a multiply.
__device__ __forceinline__ float smooth_dlogit(float g, float A, float p, float hot, float eC, float wj) {
    return g * (A * p - hot - eC * wj);
}

// ---------------------------------------------------------------- the block
// Thread 0's sum of the 256 partials, in slot order.
__device__ __forceinline__ float slot_total(const float* sl) {
    float s = 0.f;
    for (int i = 0; i < LOSS_SLOTS; ++i) s += sl[i];
    return s;
}
// v: the slot's partial, as its lane sub == 0 holds it.  Returns the sum over the slots to thread 0 (0 to the others); one barrier.
__device__ __forceinline__ float slot_sum0(float* sl, float v) {
    if (loss_sub() == 0) sl[loss_slot()] = v;
    __syncthreads();
    return threadIdx.x == 0 ? slot_total(sl) : 0.f;
}
// ... broadcast to every thread through *bc; two barriers.
__device__ __forceinline__ float slot_sum(float* sl, float* bc, float v) {
    const float s = slot_sum0(sl, v);
    if (threadIdx.x == 0) *bc = s;
    __syncthreads();
    return *bc;
}
// Two quantities behind the same barriers: sl[0] and sl[1] take the partials, bc[0] and bc[1] the sums.
__device__ __forceinline__ void slot_put2(float (*sl)[LOSS_SLOTS], float a, float b) {
    if (loss_sub() == 0) {
        sl[0][loss_slot()] = a;
        sl[1][loss_slot()] = b;
    }
    __syncthreads();
}
__device__ __forceinline__ float2 slot_sum2(float (*sl)[LOSS_SLOTS], float* bc, float a, float b) {
    slot_put2(sl, a, b);
    if (threadIdx.x == 0) {
        const float s = slot_total(sl[0]), k = slot_total(sl[1]);
        bc[0] = s;
        bc[1] = k;
    }
    __syncthreads();
    return make_float2(bc[0], bc[1]);
}

__device__ __forceinline__ void loss_store(float* loss_out, int loss_acc, float v) { loss_out[0] = loss_acc ? loss_out[0] + v : v; }
