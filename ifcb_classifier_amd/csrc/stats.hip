// Exact per-image, per-channel integer moments (sum v, sum v*v) of a u8 plane [n_img][pixels][channels]: what
// neuston_util.py:31-38 (np.mean / np.std over ToTensor output) needs, since ToTensor only divides these bytes by 255.
//
// A latency-bound side kernel (CALC_IMG_NORM reads one resized plane per batch while the CPU loaders decode PNGs): one block
// per image, 16-byte loads on the aligned body of the image's bytes, byte loads on the unaligned head and tail, per-lane
// 64-bit accumulators, wave shuffles + LDS for the block sum.  Integer arithmetic throughout, so the result does not depend
// on the order of the adds.
#include "common.h"

namespace {

constexpr int MOM_THREADS = 256;

// byte at image-local offset L (channel L % C) into the per-lane accumulators; c is runtime, the arrays stay in registers
template <int C>
__device__ __forceinline__ void add_byte(uint64_t* s, uint64_t* q, uint32_t v, int c) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const uint32_t m = c == k ? v : 0u;
        s[k] += m;
        q[k] += m * m;
    }
}

template <int C>
__global__ __launch_bounds__(MOM_THREADS) void u8_moments_kernel(const uint8_t* x, int64_t ppi, uint64_t* out) {
    const int64_t img = blockIdx.x;
    const int64_t nb = ppi * C;                              // bytes of one image
    const uint8_t* base = x + img * nb;
    // body: the 16-byte aligned chunks inside [base, base + nb); head / tail: the bytes before and after it
    const uintptr_t b0 = (uintptr_t)base, b1 = b0 + (uintptr_t)nb;
    uintptr_t a0 = (b0 + 15) & ~(uintptr_t)15, a1 = b1 & ~(uintptr_t)15;
    if (a0 > b1) a0 = b1;
    if (a1 < a0) a1 = a0;
    const int64_t head = (int64_t)(a0 - b0), nchunks = (int64_t)(a1 - a0) / 16, tail0 = (int64_t)(a1 - b0);

    uint64_t s[C], q[C];
#pragma unroll
    for (int k = 0; k < C; ++k) s[k] = q[k] = 0;

    for (int64_t L = threadIdx.x; L < head; L += MOM_THREADS) add_byte<C>(s, q, base[L], (int)(L % C));
    for (int64_t L = tail0 + threadIdx.x; L < nb; L += MOM_THREADS) add_byte<C>(s, q, base[L], (int)(L % C));

    const uint4* body = reinterpret_cast<const uint4*>(a0);
    for (int64_t j = threadIdx.x; j < nchunks; j += MOM_THREADS) {
        const uint4 w = body[j];
        const uint32_t wd[4] = {w.x, w.y, w.z, w.w};
        // chunk byte b belongs to chunk class b % C; class k is channel (k + r) % C with r the chunk's phase (0 unless C == 3)
        uint32_t cs[C], cq[C];                               // <= 16 * 255^2: 32 bits per chunk
#pragma unroll
        for (int k = 0; k < C; ++k) cs[k] = cq[k] = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint32_t v = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu;
            cs[b % C] += v;
            cq[b % C] += v * v;
        }
        const int r = (int)((head + 16 * j) % C);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < C; ++k)
                if ((k + r) % C == c) { s[c] += cs[k]; q[c] += cq[k]; }
    }

    // block reduction: wave shuffles, then one LDS row per wave
    __shared__ uint64_t part[MOM_THREADS / 64][2 * C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s[k] += __shfl_xor(s[k], o, 64);
            q[k] += __shfl_xor(q[k], o, 64);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < C; ++k) { part[wave][2 * k] = s[k]; part[wave][2 * k + 1] = q[k]; }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * C) {
        uint64_t t = 0;
#pragma unroll
        for (int wv = 0; wv < MOM_THREADS / 64; ++wv) t += part[wv][threadIdx.x];
        out[img * 2 * C + threadIdx.x] = t;                  // out[img][c][m], m = 0: sum v, 1: sum v*v
    }
}

}  // namespace

extern "C" int ifcbk_u8_channel_moments(ifcbk_ctx* ctx, const uint8_t* x, int n_img, int64_t pixels_per_img, int channels,
                                        uint64_t* out, void* stream) {
    if (channels < 1 || channels > 4) IFCBK_FAIL(ctx, IFCBK_EINVAL, "u8_channel_moments: channels %d not in 1..4", channels);
    if (pixels_per_img < 0 || n_img < 0)
        IFCBK_FAIL(ctx, IFCBK_EINVAL, "u8_channel_moments: n_img %d, pixels_per_img %lld", n_img, (long long)pixels_per_img);
    if (n_img == 0) return IFCBK_OK;
    if (!x || !out) IFCBK_FAIL(ctx, IFCBK_EINVAL, "u8_channel_moments: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_img), block(MOM_THREADS);
    switch (channels) {
        case 1: hipLaunchKernelGGL(u8_moments_kernel<1>, grid, block, 0, st, x, pixels_per_img, out); break;
        case 2: hipLaunchKernelGGL(u8_moments_kernel<2>, grid, block, 0, st, x, pixels_per_img, out); break;
        case 3: hipLaunchKernelGGL(u8_moments_kernel<3>, grid, block, 0, st, x, pixels_per_img, out); break;
        default: hipLaunchKernelGGL(u8_moments_kernel<4>, grid, block, 0, st, x, pixels_per_img, out); break;
    }
    IFCBK_LAUNCH_CHECK(ctx, "u8_channel_moments");
    return IFCBK_OK;
}
