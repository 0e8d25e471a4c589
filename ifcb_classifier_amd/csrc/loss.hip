// Class-weighted cross-entropy: nn.CrossEntropyLoss(weight=w), mean reduction (TRAIN --class-norm).  The unweighted loss keeps its
// own kernel and entry point (pool_head.hip); this file is reached only when the engine holds class weights -- or a label-smoothing
// factor (TRAIN --label-smoothing: softmax_xent_ls_kernel, with or without class weights), or a focusing exponent (TRAIN --focal-gamma:
// softmax_xent_focal_kernel, with or without class weights), or the factors of a mixed batch (TRAIN --mixup / --cutmix:
// softmax_xent_mix_kernel, two targets per image, with or without class weights and smoothing), or a teacher's logits (TRAIN --distill:
// softmax_xent_distill_kernel, with or without class weights and smoothing).
#include "common.h"
#include "loss_rows.h"
#include <float.h>
#include <math.h>

namespace {

// Every kernel below has the shape loss_rows.h states (one 1024-thread block, four lanes per sample, fixed butterflies, fixed-order slot
// sums: bitwise reproducible) and is built from its pieces; a kernel's comment gives its own formulas and the notes on its arithmetic.

// softmax_xent_kernel behind a pre-pass for the normaliser W = sum_n w[t_n] (a slot sum, broadcast):
//   c_n = weight * (w[t_n] / W),   d[n][j] = c_n * (p[n][j] - onehot),   loss = (sum_slots sum_n w[t_n] l_n) * (1 / W) * weight
// With all-ones class weights W == N exactly (a sum of ones below 2^24) and 1 / W == 1.f / N, so every operation has the operands
// it has in softmax_xent_kernel: loss and dlogits are then bit-equal to the unweighted kernel's.
// A target outside [0, NC) is the caller's fault, as there.
__global__ __launch_bounds__(1024) void softmax_xent_w_kernel(const float* logits, const int64_t* target, const float* class_weight,
                                                              int N, int NC, float weight, float* loss_out, int loss_acc,
                                                              float* dlogits) {
    __shared__ float sl[LOSS_SLOTS];
    __shared__ float sW;
    const int sub = loss_sub(), slot = loss_slot();
    float wsum = 0.f;
    if (sub == 0)
        for (int n = slot; n < N; n += 256) wsum += class_weight[(int)target[n]];
    const float W = slot_sum(sl, &sW, wsum);
    const float invW = 1.f / W;
    float local = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        const float mx = row_max(l, NC, sub);
        const float s = row_expsum(l, mx, NC, sub);
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
    const float total = slot_sum0(sl, local);
    if (threadIdx.x == 0) loss_store(loss_out, loss_acc, total * invW * weight);
}

// Label-smoothed cross-entropy: nn.CrossEntropyLoss(weight=w, label_smoothing=eps), mean reduction (TRAIN --label-smoothing).  With C = NC,
// p = softmax(l), w = class_weight (NULL: all ones), W = sum_n w[t_n], SW = sum_k w[k], c1 = 1 - eps, eC = eps / C:
//   loss      = weight / W * sum_n [ c1 w[t_n] (-log p[n][t_n]) + eC sum_j w[j] (-log p[n][j]) ]
//   d[n][j]   = weight / W * [ (c1 w[t_n] + eC SW) p[n][j] - c1 w[t_n] [j == t_n] - eC w[j] ]
// The normaliser stays W (torch does not rescale it by eps).  W and SW come from one pre-pass (slot s takes the samples / classes
// s, s + 256, ... in order).  The smoothing term is smooth_q's sum of non-negative pieces.  Per sample: 2 NC expf and one logf as in the
// kernels above, and for the smoothing NC (subtract, add, multiply-add) + 2 butterfly adds for the loss, NC (multiply, multiply-subtract)
// for dlogits.
// eps == 0 computes softmax_xent_w's function through this kernel's own operations (not bit-equal to it).
// A target outside [0, NC) is the caller's fault, as there; so is W == 0 (every target in a zero-weight class: torch gives NaN too).
__global__ __launch_bounds__(1024) void softmax_xent_ls_kernel(const float* logits, const int64_t* target, const float* class_weight,
                                                               int N, int NC, float weight, float eps, float* loss_out, int loss_acc,
                                                               float* dlogits) {
    __shared__ float sl[2][LOSS_SLOTS];
    __shared__ float sW[2];
    const int sub = loss_sub(), slot = loss_slot();
    float wsum = 0.f, ksum = 0.f;
    if (sub == 0) {
        for (int n = slot; n < N; n += 256) wsum += class_w(class_weight, (int)target[n]);
        for (int k = slot; k < NC; k += 256) ksum += class_w(class_weight, k);
    }
    const float2 sums = slot_sum2(sl, sW, wsum, ksum);
    const float W = sums.x, SW = sums.y;
    const float invW = 1.f / W;
    const float g = weight / W;
    const float c1 = 1.f - eps, eC = eps / (float)NC;
    float local = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        const float mx = row_max(l, NC, sub);
        const float s = row_expsum(l, mx, NC, sub);
        const float ls = logf(s);
        const float q = smooth_q(l, class_weight, mx, ls, NC, sub);
        const int tg = ok ? (int)target[n] : 0;
        const float wt = ok ? class_w(class_weight, tg) : 0.f;
        const float hard = c1 * wt;
        if (ok && sub == 0) {
            const float li = mx + ls - l[tg];
            local += c1 * (wt * li) + eC * q;
        }
        if (ok && dlogits) {
            float* d = dlogits + (size_t)n * NC;
            const float is = 1.f / s;
            const float A = hard + eC * SW;
            for (int j = sub; j < NC; j += 4)
                d[j] = smooth_dlogit(g, A, expf(l[j] - mx) * is, j == tg ? hard : 0.f, eC, class_w(class_weight, j));
        }
    }
    __syncthreads();                       // (thread 0 has finished reading the pre-pass partials)
    const float total = slot_sum0(sl[0], local);
    if (threadIdx.x == 0) loss_store(loss_out, loss_acc, total * invW * weight);
}

// Focal loss (TRAIN --focal-gamma): with p = softmax(l), w = class_weight (NULL: all ones), W = sum_n w[t_n], g = gamma >= 0,
//   u_n = 1 - p[n][t_n],  L_n = -log p[n][t_n]
//   loss    = weight / W * sum_n w[t_n] u_n^g L_n
//   d[n][j] = weight / W * w[t_n] (p[n][j] - [j == t_n]) (u_n^g + g p[n][t_n] u_n^(g-1) L_n)
// The normaliser stays W, so g -> 0 is softmax_xent_w's function and the class weights are focal loss's per-class alpha.
// One pre-pass for W.  Three points of the arithmetic:
//   u is so / s with so = sum_{j != t} expf(l_j - mx), the sum s with the target's term left out: non-negative terms, no cancellation
//     (1 - p_t and s - e_t cancel when the target is the row's maximum: e_t == 1).  Term by term so's chain is below s's, so u <= 1.
//     The target's dlogits element is -u, not p_t - 1, for the same reason.
//   u^g is expf(g * logf(u)) for u > 0; for u == 0 it is 0 (g > 0) or 1 (g == 0).
//   the bracket is pw + (g p_t) (pw (L / u)) with L / u taken as 0 when u == 0: both terms non-negative and finite for every g > 0, g < 1
//     included (u^(g-1) alone is infinite at 0).  L = (mx + log s) - l_t >= 0: s >= 1, and rounding is monotone.  When u is below 2^-25
//     the target is the maximum, s rounds to 1 and L is exactly 0, so L / u cannot overflow.
// A row whose other classes' exponentials all flush to zero (u == 0; NC == 1 always) gives a loss term of 0 and a zero dlogits row for
// g > 0.  Per sample: NC expf, one logf for L, logf + expf for the power, two divisions (u, L / u) and 1 / s; for dlogits NC more expf and
// NC products.  g == 0 computes softmax_xent_w's function through this kernel's own operations (not bit-equal to it).
// A target outside [0, NC) is the caller's fault, as there; so is W == 0 (NaN).
__global__ __launch_bounds__(1024) void softmax_xent_focal_kernel(const float* logits, const int64_t* target, const float* class_weight,
                                                                  int N, int NC, float weight, float gam, float* loss_out, int loss_acc,
                                                                  float* dlogits) {
    __shared__ float sl[LOSS_SLOTS];
    __shared__ float sW;
    const int sub = loss_sub(), slot = loss_slot();
    float wsum = 0.f;
    if (sub == 0)
        for (int n = slot; n < N; n += 256) wsum += class_w(class_weight, (int)target[n]);
    const float W = slot_sum(sl, &sW, wsum);
    const float invW = 1.f / W;
    float local = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        const int tg = ok ? (int)target[n] : 0;
        const float mx = row_max(l, NC, sub);
        float s = 0.f, so = 0.f;
        for (int j = sub; j < NC; j += 4) {
            const float e = expf(l[j] - mx);
            s += e;
            so += j == tg ? 0.f : e;
        }
        s = quad_sum(s);
        so = quad_sum(so);
        const float wt = ok ? class_w(class_weight, tg) : 0.f;
        const float li = mx + logf(s) - l[tg];
        const float u = so / s;
        const float pw = u > 0.f ? expf(gam * logf(u)) : (gam == 0.f ? 1.f : 0.f);
        if (ok && sub == 0) local += wt * (pw * li);
        if (ok && dlogits) {
            float* d = dlogits + (size_t)n * NC;
            const float is = 1.f / s;
            const float pt = expf(l[tg] - mx) * is;
            const float r = u > 0.f ? li / u : 0.f;
            const float br = pw + (gam * pt) * (pw * r);
            const float cb = weight * (wt / W) * br;
            for (int j = sub; j < NC; j += 4) d[j] = cb * (j == tg ? -u : expf(l[j] - mx) * is);
        }
    }
    __syncthreads();                       // (thread 0 has finished reading the W partials)
    const float total = slot_sum0(sl, local);
    if (threadIdx.x == 0) loss_store(loss_out, loss_acc, total * invW * weight);
}

// Two-target loss of a mixed batch (TRAIN --mixup / --cutmix; ifcbk_batch_mix pairs image n with m = N - 1 - n): with a = target[n],
// b = target[N - 1 - n], lam_n = lam[n], p = softmax(l), w = class_weight (NULL: all ones), c1 = 1 - eps, eC = eps / NC, SW = sum_k w[k]:
//   h_n     = lam_n w[a] + (1 - lam_n) w[b],    W = sum_n h_n
//   loss    = weight / W * sum_n [ c1 (lam_n w[a] (-log p[n][a]) + (1 - lam_n) w[b] (-log p[n][b])) + eC sum_j w[j] (-log p[n][j]) ]
//   d[n][j] = weight / W * [ (c1 h_n + eC SW) p[n][j] - c1 lam_n w[a] [j == a] - c1 (1 - lam_n) w[b] [j == b] - eC w[j] ]
// Without weights W == N and this is timm's SoftTargetCrossEntropy on mixup_target; at lam == 1 it is softmax_xent_ls_kernel's function
// (eps == 0: softmax_xent_w_kernel's), through this kernel's own operations.  a == b is legal: both one-hot terms land on one element.
// The pre-pass for W and SW and the smoothing term are softmax_xent_ls_kernel's.  Per sample, on top of that kernel: 1 - lam_n, two
// products and an add for h_n (computed the same way in the pre-pass and in the row), a second -log p.
// A target outside [0, NC) or a lam outside [0, 1] is the caller's fault; so is W == 0.
__global__ __launch_bounds__(1024) void softmax_xent_mix_kernel(const float* logits, const int64_t* target, const float* lam,
                                                                const float* class_weight, int N, int NC, float weight, float eps,
                                                                float* loss_out, int loss_acc, float* dlogits) {
    __shared__ float sl[2][LOSS_SLOTS];
    __shared__ float sW[2];
    const int sub = loss_sub(), slot = loss_slot();
    float wsum = 0.f, ksum = 0.f;
    if (sub == 0) {
        for (int n = slot; n < N; n += 256) {
            const float lm = lam[n];
            const float ta = lm * class_w(class_weight, (int)target[n]);
            const float tb = (1.f - lm) * class_w(class_weight, (int)target[N - 1 - n]);
            wsum += ta + tb;
        }
        for (int k = slot; k < NC; k += 256) ksum += class_w(class_weight, k);
    }
    const float2 sums = slot_sum2(sl, sW, wsum, ksum);
    const float W = sums.x, SW = sums.y;
    const float invW = 1.f / W;
    const float g = weight / W;
    const float c1 = 1.f - eps, eC = eps / (float)NC;
    float local = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        const float mx = row_max(l, NC, sub);
        const float s = row_expsum(l, mx, NC, sub);
        const float ls = logf(s);
        const float q = smooth_q(l, class_weight, mx, ls, NC, sub);
        const int ta_i = ok ? (int)target[n] : 0, tb_i = ok ? (int)target[N - 1 - n] : 0;
        const float lm = ok ? lam[n] : 1.f;
        const float ta = ok ? lm * class_w(class_weight, ta_i) : 0.f;
        const float tb = ok ? (1.f - lm) * class_w(class_weight, tb_i) : 0.f;
        const float h = ta + tb;
        if (ok && sub == 0) {
            const float lia = mx + ls - l[ta_i], lib = mx + ls - l[tb_i];
            local += c1 * (ta * lia + tb * lib) + eC * q;
        }
        if (ok && dlogits) {
            float* d = dlogits + (size_t)n * NC;
            const float is = 1.f / s;
            const float ha = c1 * ta, hb = c1 * tb;
            const float A = c1 * h + eC * SW;
            for (int j = sub; j < NC; j += 4)
                d[j] = g * (A * (expf(l[j] - mx) * is) - (j == ta_i ? ha : 0.f) - (j == tb_i ? hb : 0.f) - eC * class_w(class_weight, j));
        }
    }
    __syncthreads();                       // (thread 0 has finished reading the pre-pass partials)
    const float total = slot_sum0(sl[0], local);
    if (threadIdx.x == 0) loss_store(loss_out, loss_acc, total * invW * weight);
}

// Knowledge distillation (TRAIN --distill): Hinton's loss, the smoothed hard loss of softmax_xent_ls_kernel mixed with the KL divergence
// from a teacher's softened scores.  a = weight, T = temperature, s = logits, z = teacher, r = softmax(s / T), q = softmax(z / T), and
// H, Dh = loss and dlogits of softmax_xent_ls_kernel at weight 1 (same class_weight, eps and normaliser W = sum_n w[t_n]):
//   K       = 1 / N * sum_n sum_j q[n][j] (log q[n][j] - log r[n][j])                        (KL(q || r), "batchmean")
//   loss    = a * ((1 - alpha) * H + alpha T^2 * K)
//   d[n][j] = a * ((1 - alpha) * Dh[n][j] + alpha T / N * (r[n][j] - q[n][j]))
// Class weights act on the hard term only.  softmax_xent_ls_kernel's pre-pass for W and SW; two final sums (one chain of 256 slots for the
// hard terms, one for the soft ones).  Points of the arithmetic:
//   x / T is a DIVISION of the rounded difference: arg_j = fl(fl(x_j - max) / T), correctly rounded, two roundings per argument (a product
//     with a rounded 1 / T would be three).  T > 0, so the row's maximum is the maximum of x / T as well and its argument is exactly 0:
//     both softened sums are >= 1, as s is.
//   log q - log r is formed from the arguments, never from a stored probability: log q_j = arg_j(z) - log sum_q, each part <= 0, so neither
//     log-probability cancels; the difference of the two does, which is why the bound is taken on q (|log q| + |log r|).
//   a q[n][j] that underflows to 0 contributes exactly 0 to the loss (its finite log difference is not multiplied in), and its dlogits
//     element is a alpha T / N * r[n][j]; no log of 0 is taken anywhere.
//   alpha == 1: 1 - alpha is an exact 0 and multiplies a finite hard term (W != 0), so without class weights neither output depends on
//     target; alpha == 0: alpha T^2 and alpha T / N are exact zeros on finite soft terms, so neither output depends on teacher, and
//     the function is softmax_xent_ls_kernel's (through this kernel's own operations, not its bits).
//   In dlogits the weight a is folded into the two factors: the hard part is a Dh exactly as softmax_xent_ls_kernel forms it
//     (g = a / W), the soft factor is fl(a * fl(fl(alpha T) / N)); at alpha == 0 the element is 1 * (a Dh) + 0.
// Per sample, on top of that kernel: 2 NC divisions, 2 NC expf and 2 logf for the two softened sums, NC (2 subtract, subtract, multiply)
// + 2 butterfly adds for K, and for dlogits NC (2 expf, 2 multiply, subtract, 2 multiply-add).
// A target outside [0, NC) is the caller's fault, as there; so is W == 0 (NaN, also at alpha == 1).
__global__ __launch_bounds__(1024) void softmax_xent_distill_kernel(const float* logits, const int64_t* target, const float* teacher,
                                                                    const float* class_weight, int N, int NC, float weight, float eps,
                                                                    float alpha, float T, float* loss_out, int loss_acc, float* dlogits) {
    __shared__ float sl[2][LOSS_SLOTS];
    __shared__ float sW[2];
    const int sub = loss_sub(), slot = loss_slot();
    float wsum = 0.f, ksum = 0.f;
    if (sub == 0) {
        for (int n = slot; n < N; n += 256) wsum += class_w(class_weight, (int)target[n]);
        for (int k = slot; k < NC; k += 256) ksum += class_w(class_weight, k);
    }
    const float2 sums = slot_sum2(sl, sW, wsum, ksum);
    const float W = sums.x, SW = sums.y;
    const float invW = 1.f / W;
    const float c1 = 1.f - eps, eC = eps / (float)NC;
    const float ch = 1.f - alpha;                     // weight of the hard term
    const float cs = (alpha * T) * T;                 // ... of K in the loss
    const float cd = weight * ((alpha * T) / (float)N);      // ... of r - q in dlogits, the weight folded in
    const float g = weight / W;                       // the hard gradient's factor, as softmax_xent_ls_kernel forms it
    float local = 0.f, localk = 0.f;
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + slot;
        const bool ok = n < N;
        const float* l = logits + (size_t)(ok ? n : 0) * NC;
        const float* z = teacher + (size_t)(ok ? n : 0) * NC;
        float mx = -INFINITY, mz = -INFINITY;
        for (int j = sub; j < NC; j += 4) {
            mx = fmaxf(mx, l[j]);
            mz = fmaxf(mz, z[j]);
        }
        mx = quad_max(mx);
        mz = quad_max(mz);
        float s = 0.f, sr = 0.f, sq = 0.f;
        for (int j = sub; j < NC; j += 4) {
            const float dl = l[j] - mx, dz = z[j] - mz;
            s += expf(dl);
            sr += expf(dl / T);
            sq += expf(dz / T);
        }
        s = quad_sum(s);
        sr = quad_sum(sr);
        sq = quad_sum(sq);
        const float ls = logf(s), lsr = logf(sr), lsq = logf(sq);
        const float isr = 1.f / sr, isq = 1.f / sq;
        float q = 0.f, kl = 0.f;
        for (int j = sub; j < NC; j += 4) {
            smooth_q_add(q, class_w(class_weight, j), mx, l[j], ls);
            const float ar = (l[j] - mx) / T, aq = (z[j] - mz) / T;
            const float qj = expf(aq) * isq;
            const float diff = (aq - lsq) - (ar - lsr);
            const float term = qj * diff;
            kl += qj > 0.f ? term : 0.f;
        }
        q = quad_sum(q);
        kl = quad_sum(kl);
        const int tg = ok ? (int)target[n] : 0;
        const float wt = ok ? class_w(class_weight, tg) : 0.f;
        const float hard = c1 * wt;
        if (ok && sub == 0) {
            const float li = mx + ls - l[tg];
            local += c1 * (wt * li) + eC * q;
            localk += kl;
        }
        if (ok && dlogits) {
            float* d = dlogits + (size_t)n * NC;
            const float is = 1.f / s;
            const float A = hard + eC * SW;
            for (int j = sub; j < NC; j += 4) {
                const float dh = smooth_dlogit(g, A, expf(l[j] - mx) * is, j == tg ? hard : 0.f, eC, class_w(class_weight, j));
                const float rj = expf((l[j] - mx) / T) * isr, qj = expf((z[j] - mz) / T) * isq;
                const float soft = cd * (rj - qj);
                d[j] = ch * dh + soft;
            }
        }
    }
    __syncthreads();                       // (thread 0 has finished reading the pre-pass partials)
    slot_put2(sl, local, localk);
    if (threadIdx.x == 0) {
        const float H = slot_total(sl[0]) * invW;
        const float K = slot_total(sl[1]) * (1.f / (float)N);
        const float soft = cs * K;
        loss_store(loss_out, loss_acc, weight * (ch * H + soft));
    }
}

// softmax that adds into a score buffer (RUN --tta: the mean of the softmax outputs over the views of a batch):
//   acc[n][j] = ((accumulate ? acc[n][j] : 0) + p[n][j]) * scale,   p exactly ifcbk_softmax's value (softmax_row_norm, common.h)
// softmax_kernel's shape: one thread per row, 64-thread blocks, every element read and written by one thread -- bitwise reproducible.
// p, the sum and the product are three statements: under -ffp-contract=on nothing contracts across them, so each is one rounding, and
// accumulate == 0 with scale == 1 stores p's bits (p * 1 is exact).
__global__ void softmax_acc_kernel(const float* logits, int N, int NC, float* acc, int accumulate, float scale) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* l = logits + (size_t)n * NC;
    float* a = acc + (size_t)n * NC;
    float mx;
    const float is = softmax_row_norm(l, NC, mx);
    for (int j = 0; j < NC; ++j) {
        const float p = expf(l[j] - mx) * is;
        float v = p;
        if (accumulate) v = a[j] + p;
        a[j] = v * scale;
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int ifcbk_softmax_acc(ifcbk_ctx* ctx, const float* logits, int N, int NC, float* acc, int accumulate, float scale, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!logits || !acc) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_acc: NULL operand");
    if (N < 1 || NC < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_acc: N %d or NC %d < 1", N, NC);
    if (!(scale > 0.f && scale <= FLT_MAX)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_acc: scale is not a finite positive number");
    hipLaunchKernelGGL(softmax_acc_kernel, dim3(cdiv(N, 64)), dim3(64), 0, ST, logits, N, NC, acc, accumulate, scale);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_acc");
    return IFCBK_OK;
}

// The refusals the five entry points below share.  name: the entry point's, without its ifcbk_ prefix; operands: logits, target and
// loss_out are all there; label_smoothing: 0 from the entry points that have none.
static int loss_refused(ifcbk_ctx* ctx, const char* name, int N, int NC, float label_smoothing, bool operands) {
    if (N <= 0 || NC <= 0) IFCBK_FAIL(ctx, IFCBK_EINVAL, "%s: empty", name);
    if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "%s: label_smoothing outside [0, 1]", name);
    if (!operands) IFCBK_FAIL(ctx, IFCBK_EINVAL, "%s: NULL operand", name);
    return IFCBK_OK;
}

extern "C" int ifcbk_softmax_xent_w(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* class_weight, int N, int NC,
                                    float weight, float* loss_out, int loss_accumulate, float* dlogits, void* stream) {
    if (int e = loss_refused(ctx, "softmax_xent_w", N, NC, 0.f, logits && target && loss_out)) return e;
    if (!class_weight) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_w: class_weight is NULL (the unweighted loss is ifcbk_softmax_xent)");
    hipLaunchKernelGGL(softmax_xent_w_kernel, dim3(1), dim3(1024), 0, ST, logits, target, class_weight, N, NC, weight, loss_out,
                       loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_w");
    return IFCBK_OK;
}

extern "C" int ifcbk_softmax_xent_ls(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* class_weight, int N, int NC,
                                     float weight, float label_smoothing, float* loss_out, int loss_accumulate, float* dlogits,
                                     void* stream) {
    if (int e = loss_refused(ctx, "softmax_xent_ls", N, NC, label_smoothing, logits && target && loss_out)) return e;
    hipLaunchKernelGGL(softmax_xent_ls_kernel, dim3(1), dim3(1024), 0, ST, logits, target, class_weight, N, NC, weight, label_smoothing,
                       loss_out, loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_ls");
    return IFCBK_OK;
}

extern "C" int ifcbk_softmax_xent_focal(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* class_weight, int N, int NC,
                                        float weight, float gamma, float* loss_out, int loss_accumulate, float* dlogits, void* stream) {
    if (int e = loss_refused(ctx, "softmax_xent_focal", N, NC, 0.f, logits && target && loss_out)) return e;
    if (!(gamma >= 0.f && gamma <= FLT_MAX)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_focal: gamma negative or not finite");
    hipLaunchKernelGGL(softmax_xent_focal_kernel, dim3(1), dim3(1024), 0, ST, logits, target, class_weight, N, NC, weight, gamma, loss_out,
                       loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_focal");
    return IFCBK_OK;
}

extern "C" int ifcbk_softmax_xent_mix(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* lam, const float* class_weight,
                                      int N, int NC, float weight, float label_smoothing, float* loss_out, int loss_accumulate,
                                      float* dlogits, void* stream) {
    if (int e = loss_refused(ctx, "softmax_xent_mix", N, NC, label_smoothing, logits && target && loss_out)) return e;
    if (!lam) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_mix: lam is NULL (the one-target losses are ifcbk_softmax_xent_w / _ls)");
    hipLaunchKernelGGL(softmax_xent_mix_kernel, dim3(1), dim3(1024), 0, ST, logits, target, lam, class_weight, N, NC, weight, label_smoothing,
                       loss_out, loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_mix");
    return IFCBK_OK;
}

extern "C" int ifcbk_softmax_xent_distill(ifcbk_ctx* ctx, const float* logits, const int64_t* target, const float* teacher,
                                          const float* class_weight, int N, int NC, float weight, float label_smoothing, float alpha,
                                          float temperature, float* loss_out, int loss_accumulate, float* dlogits, void* stream) {
    if (int e = loss_refused(ctx, "softmax_xent_distill", N, NC, label_smoothing, logits && target && loss_out)) return e;
    if (!teacher) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_distill: teacher is NULL (the losses without a teacher are ifcbk_softmax_xent_w / _ls)");
    if (!(alpha >= 0.f && alpha <= 1.f)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_distill: alpha outside [0, 1]");
    if (!(temperature > 0.f && temperature <= FLT_MAX)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "softmax_xent_distill: temperature is not a finite positive number");
    hipLaunchKernelGGL(softmax_xent_distill_kernel, dim3(1), dim3(1024), 0, ST, logits, target, teacher, class_weight, N, NC, weight,
                       label_smoothing, alpha, temperature, loss_out, loss_accumulate, dlogits);
    IFCBK_LAUNCH_CHECK(ctx, "softmax_xent_distill");
    return IFCBK_OK;
}
