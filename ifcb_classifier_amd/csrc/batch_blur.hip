// Gaussian defocus of a RESIZED batch (TRAIN --blur): ifcbk_batch_blur blurs every image of the batch IN PLACE with its own sigma,
// torchvision's GaussianBlur at a window fixed for the run: radius r, k = 2 r + 1 taps,
//     w[j] = exp(-0.5 ((j - r) / sigma)^2) / sum          j = 0..k-1, fp32 expf, the sum taken in ascending j
//     h[y][x]  = sum_j w[j] x[y][reflect(x - r + j)]       one fmaf chain in ascending j, starting from 0
//     x'[y][x] = sum_j w[j] h[reflect(y - r + j)][x]       likewise
// with torch's 'reflect' border (-1 -> 1, S -> S - 2: the edge is not repeated; r < S, so one reflection lands inside).  sigma[n] == 0
// means "not drawn": the block leaves before it touches memory and the image keeps its bits; so does a sigma that is negative or not
// finite.
//
// A stencil cannot run in place block by block -- the neighbouring block still needs the original halo -- so ONE block owns a whole
// plane: image n of the u8 form, channel c (0..2) of image n of the dense form, whose pad channels 3..7 nobody touches.  The block
// streams the plane top to bottom in bands of BB rows:
//     stage   the raw rows the band still lacks, BB at a time, as fp32 with their reflected halo (S + 2 r floats per row)
//     ring    those rows filtered horizontally into an LDS ring of k + BB - 1 fp32 rows (row q lives in slot q mod ring rows)
//     out     rows y0 .. y0 + BB - 1, written only after row y0 + BB - 1 + r has been read: every raw row a later band stages lies
//             below everything written so far
// Every byte the block reads or writes belongs to its plane, every sum has one fixed order and there are no atomics: an image's
// bits depend on nothing but its own pixels and sigma.  The u8 images start at arbitrary byte addresses (S * S is odd at 299) and are
// read and written byte by byte; the dense elements are read and written one at a time (2 or 4 bytes at a 16- or 32-byte stride).
#include "common.h"

namespace {

constexpr int BT = 512;               // threads per block
constexpr int BB = 4;                 // rows per band
constexpr int BRMAX = 12;             // largest radius (sigma_max 4: r = ceil(3 sigma_max))
constexpr int BHEAD = 64;             // floats in front of the rows: k <= 25 weights, then BB + 2 r <= 28 ring offsets

struct BlurU8 {
    typedef uint8_t T;
    static constexpr int STRIDE = 1, PLANES = 1;
    __device__ static __forceinline__ float load(const T* p) { return (float)*p; }
    // nearest-even (rintf in the default rounding mode), clamped to 0..255
    __device__ static __forceinline__ void store(T* p, float v) { *p = (uint8_t)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }
};
template <class E> struct BlurDense {
    typedef E T;
    static constexpr int STRIDE = 8, PLANES = 3;
    __device__ static __forceinline__ float load(const T* p) { return to_f32(*p); }
    __device__ static __forceinline__ void store(T* p, float v) { *p = from_f32<E>(v); }
};

__device__ __forceinline__ int reflect(int i, int S) {
    i = i < 0 ? -i : i;
    return i >= S ? 2 * (S - 1) - i : i;
}

template <class F>
__global__ __launch_bounds__(BT) void batch_blur_kernel(typename F::T* x, int S, const float* sigma, int r, int ring_rows) {
    extern __shared__ float lds[];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float sg = sigma[n];
    if (!(sg > 0.0f && sg <= 3.402823466e38f)) return;           // 0 = not drawn; NaN fails both comparisons, +inf the second
    const int k = 2 * r + 1, P = S + 2 * r;
    float* w = lds;
    int* slot = reinterpret_cast<int*>(lds + 32);
    float* stage = lds + BHEAD;                                  // [BB][P]
    float* ring = stage + BB * P;                                // [ring_rows][S]
    typename F::T* img = x + ((int64_t)n * S * S) * F::STRIDE + blockIdx.y;

    if (tid < k) {
        const float q = (float)(tid - r) / sg;
        w[tid] = expf(-0.5f * (q * q));
    }
    __syncthreads();
    float sum = 0.0f;
    for (int j = 0; j < k; ++j) sum += w[j];                     // (every thread: the same values in the same order)
    __syncthreads();
    if (tid < k) w[tid] = w[tid] / sum;
    __syncthreads();

    int loaded = 0;                                              // rows [0, loaded) are in the ring (the last ring_rows of them)
    for (int y0 = 0; y0 < S; y0 += BB) {
        const int need = y0 + BB - 1 + r < S - 1 ? y0 + BB - 1 + r : S - 1;
        while (loaded <= need) {
            const int cnt = need + 1 - loaded < BB ? need + 1 - loaded : BB;
            for (int i = tid; i < cnt * P; i += BT) {
                const int row = i / P, px = reflect(i - row * P - r, S);
                stage[i] = F::load(img + ((int64_t)(loaded + row) * S + px) * F::STRIDE);
            }
            __syncthreads();
            for (int i = tid; i < cnt * S; i += BT) {
                const int row = i / S, xx = i - row * S;
                const float* s = stage + row * P + xx;
                float acc = 0.0f;
                for (int j = 0; j < k; ++j) acc = fmaf(w[j], s[j], acc);
                ring[((loaded + row) % ring_rows) * S + xx] = acc;
            }
            __syncthreads();
            loaded += cnt;
        }
        // ring offsets of the rows y0 - r .. y0 + BB - 1 + r (those behind the last band's rows are never used: kept in range)
        if (tid < BB + 2 * r) {
            int q = reflect(y0 - r + tid, S);
            q = q < 0 ? 0 : q;
            slot[tid] = (q % ring_rows) * S;
        }
        __syncthreads();
        const int rows = S - y0 < BB ? S - y0 : BB;
        for (int i = tid; i < rows * S; i += BT) {
            const int row = i / S, xx = i - row * S;
            float acc = 0.0f;
            for (int j = 0; j < k; ++j) acc = fmaf(w[j], ring[slot[row + j] + xx], acc);
            F::store(img + ((int64_t)(y0 + row) * S + xx) * F::STRIDE, acc);
        }
        __syncthreads();                                         // (the next band overwrites slot and the ring's oldest rows)
    }
}

size_t blur_lds_bytes(int S, int r) {
    return ((size_t)BHEAD + (size_t)BB * (S + 2 * r) + (size_t)(2 * r + BB) * S) * sizeof(float);
}

}  // namespace

extern "C" int ifcbk_batch_blur(ifcbk_ctx* ctx, void* x, int kind, int N, int S, const float* sigma, int radius, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!x || !sigma) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: x or sigma is NULL");
    if (N < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: N %d < 1", N);
    if (radius < 1 || radius > BRMAX) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: radius %d outside 1..%d", radius, BRMAX);
    if (radius >= S) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: radius %d >= S %d (the reflected border needs r < S)", radius, S);
    if (kind != IFCBK_MIX_U8 && kind != IFCBK_BF16 && kind != IFCBK_F32) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: kind %d", kind);
    if (kind != IFCBK_MIX_U8 && ((uintptr_t)x & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: a dense tensor must be 16-byte aligned");
    const size_t lds = blur_lds_bytes(S, radius);
    if (lds > 65536) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_blur: S %d at radius %d needs %zu bytes of LDS rows (> 65536)", S, radius, lds);
    hipStream_t st = (hipStream_t)stream;
    const int ring_rows = 2 * radius + BB;                       // k + BB - 1
    if (kind == IFCBK_MIX_U8) {
        hipLaunchKernelGGL(batch_blur_kernel<BlurU8>, dim3((unsigned)N, BlurU8::PLANES), dim3(BT), lds, st, (uint8_t*)x, S, sigma, radius,
                           ring_rows);
    } else if (kind == IFCBK_BF16) {
        hipLaunchKernelGGL(batch_blur_kernel<BlurDense<bf16_t>>, dim3((unsigned)N, 3), dim3(BT), lds, st, (bf16_t*)x, S, sigma, radius,
                           ring_rows);
    } else {
        hipLaunchKernelGGL(batch_blur_kernel<BlurDense<float>>, dim3((unsigned)N, 3), dim3(BT), lds, st, (float*)x, S, sigma, radius,
                           ring_rows);
    }
    IFCBK_LAUNCH_CHECK(ctx, "batch_blur");
    return IFCBK_OK;
}
