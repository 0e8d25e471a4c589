// Brightness / contrast jitter of ragged u8 ROIs (TRAIN --jitter): ifcbk_roi_jitter.  Per ROI, with factors fb and fc,
//     img' = ImageEnhance.Contrast(ImageEnhance.Brightness(img).enhance(fb)).enhance(fc)
// of Pillow.  Both enhancements are Image.blend(degenerate, img, f), which is the 256-entry table
//     t = fl32( fl32(m) + fl32( f * fl32(v - m) ) )          two float32 roundings, never a fused multiply-add
//     lut[v] = t <= 0 ? 0 : t >= 255 ? 255 : trunc(t)
// with m = 0 for brightness and, for contrast, m = (2 sum L + n) / (2 n): the rounded mean of the L plane of the image AFTER the
// brightness step over all n pixels (one channel: L = the pixel; three: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16).  The
// same table maps every channel.  A factor that is not finite or is negative counts as 1 (the identity table).
//
// Two kernels over one grid shape, (ROI, chunk of JCHUNK bytes) sized by max_h * max_w * ch; blocks behind a ROI's end exit:
//   roi_jitter_sum_kernel    (contrast only) exact integer sum of L of the brightness-mapped pixels, one 64-bit atomic add per wave into
//                            the ctx workspace: integer sums do not depend on the order, so the result is reproducible bit for bit
//   roi_jitter_apply_kernel  builds the composed table contrast(brightness(v)) in LDS per block and maps the bytes
// ROIs start at arbitrary byte addresses: a ROI is cut into the 16-byte units of its ABSOLUTE address; whole units move as one
// 16-byte vector, the units at its head and tail byte by byte.  Every byte is read and written by the same thread and no byte outside
// [offs[i], offs[i] + h * w * ch) is written, so out may be pixels itself.
#include "common.h"

namespace {

constexpr int JT = 256;                    // threads per block = entries of the table
constexpr int JUNITS = 4;                  // 16-byte units per thread and chunk
constexpr int JCHUNK = JT * JUNITS * 16;   // bytes per chunk

__device__ __forceinline__ float jitter_factor(const float* f, int img) {
    if (!f) return 1.0f;
    const float v = f[img];
    return (v >= 0.0f && v <= 3.402823466e38f) ? v : 1.0f;       // NaN fails both comparisons, +inf the second
}

__device__ __forceinline__ int jitter_lut(float f, int m, int v) {
#pragma clang fp contract(off)
    const float t = __fadd_rn((float)m, __fmul_rn(f, (float)(v - m)));
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// the ROI's byte count; 0 for an empty or negative entry
__device__ __forceinline__ int64_t jitter_len(const int32_t* hs, const int32_t* ws, int img, int ch) {
    const int h = hs[img], w = ws[img];
    return (h > 0 && w > 0) ? (int64_t)h * w * ch : 0;
}

__global__ __launch_bounds__(JT) void roi_jitter_sum_kernel(const uint8_t* pixels, const int64_t* offs, const int32_t* hs, const int32_t* ws,
                                                            int ch, const float* brightness, unsigned long long* sums) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t len = jitter_len(hs, ws, img, ch);
    const uint8_t* src = pixels + offs[img];
    const int64_t head = (int64_t)((uintptr_t)src & 15);
    const int64_t units = (head + len + 15) >> 4;               // 16-byte units of the absolute address that hold a byte of the ROI
    if (len == 0 || (int64_t)blockIdx.y * (JT * JUNITS) >= units) return;
    __shared__ uint8_t lut[JT];
    lut[tid] = (uint8_t)jitter_lut(jitter_factor(brightness, img), 0, tid);
    __syncthreads();
    unsigned long long total = 0;
    if (ch == 1) {
        for (int64_t c = blockIdx.y; c * (JT * JUNITS) < units; c += gridDim.y) {
            unsigned s = 0;
#pragma unroll
            for (int k = 0; k < JUNITS; ++k) {
                const int64_t u = c * (JT * JUNITS) + k * JT + tid;
                if (u >= units) break;
                const int64_t rel = u * 16 - head;              // of the unit's first byte, from the ROI's first
                if (rel >= 0 && rel + 16 <= len) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src + rel);
                    const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 16; ++j) s += lut[(wd[j >> 2] >> (8 * (j & 3))) & 0xff];
                } else {
                    for (int j = 0; j < 16; ++j)
                        if (rel + j >= 0 && rel + j < len) s += lut[src[rel + j]];
                }
            }
            total += s;
        }
    } else {
        // three channels: a pixel's bytes straddle units, so the chunk is cut by pixels (those whose first byte lies in it)
        const int64_t npix = len / 3;
        for (int64_t c = blockIdx.y; c * (JT * JUNITS) < units; c += gridDim.y) {
            const int64_t b0 = c * JCHUNK, b1 = b0 + JCHUNK;
            const int64_t p0 = (b0 + 2) / 3, p1 = (b1 + 2) / 3 < npix ? (b1 + 2) / 3 : npix;
            unsigned s = 0;
            for (int64_t p = p0 + tid; p < p1; p += JT) {
                const uint8_t* q = src + p * 3;
                s += (19595u * lut[q[0]] + 38470u * lut[q[1]] + 7471u * lut[q[2]] + 0x8000u) >> 16;
            }
            total += s;
        }
    }
    for (int off = 32; off > 0; off >>= 1) total += __shfl_down(total, off, 64);
    if ((tid & 63) == 0 && total) atomicAdd(sums + img, total);
}

__global__ __launch_bounds__(JT) void roi_jitter_apply_kernel(const uint8_t* pixels, const int64_t* offs, const int32_t* hs, const int32_t* ws,
                                                              int ch, const float* brightness, const float* contrast,
                                                              const unsigned long long* sums, uint8_t* out, int vec_store) {
    const int img = blockIdx.x, tid = threadIdx.x;
    const int64_t len = jitter_len(hs, ws, img, ch);
    const uint8_t* src = pixels + offs[img];
    uint8_t* dst = out + offs[img];
    const int64_t head = (int64_t)((uintptr_t)src & 15);
    const int64_t units = (head + len + 15) >> 4;
    if (len == 0 || (int64_t)blockIdx.y * (JT * JUNITS) >= units) return;
    __shared__ uint8_t lut[JT];
    {
        int v = jitter_lut(jitter_factor(brightness, img), 0, tid);
        if (contrast) {
            const unsigned long long n = (unsigned long long)(len / ch);
            const int m = (int)((2 * sums[img] + n) / (2 * n));             // <= 255: every L is
            v = jitter_lut(jitter_factor(contrast, img), m, v);
        }
        lut[tid] = (uint8_t)v;
    }
    __syncthreads();
    for (int64_t c = blockIdx.y; c * (JT * JUNITS) < units; c += gridDim.y) {
#pragma unroll
        for (int k = 0; k < JUNITS; ++k) {
            const int64_t u = c * (JT * JUNITS) + k * JT + tid;
            if (u >= units) break;
            const int64_t rel = u * 16 - head;
            if (rel >= 0 && rel + 16 <= len) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + rel);
                unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned x = wd[q];
                    wd[q] = (unsigned)lut[x & 0xff] | ((unsigned)lut[(x >> 8) & 0xff] << 8) | ((unsigned)lut[(x >> 16) & 0xff] << 16) |
                            ((unsigned)lut[x >> 24] << 24);
                }
                if (vec_store) {
                    *reinterpret_cast<uint4*>(dst + rel) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
                } else {                                           // out is not aligned like pixels
#pragma unroll
                    for (int j = 0; j < 16; ++j) dst[rel + j] = (uint8_t)(wd[j >> 2] >> (8 * (j & 3)));
                }
            } else {
                for (int j = 0; j < 16; ++j)
                    if (rel + j >= 0 && rel + j < len) dst[rel + j] = lut[src[rel + j]];
            }
        }
    }
}

}  // namespace

extern "C" size_t ifcbk_roi_jitter_workspace(int n_img) {
    return n_img > 0 ? (size_t)n_img * sizeof(unsigned long long) : 0;
}

extern "C" int ifcbk_roi_jitter(ifcbk_ctx* ctx, const uint8_t* pixels, const int64_t* offs, const int32_t* hs, const int32_t* ws, int n_img,
                                int in_channels, int max_h, int max_w, const float* brightness, const float* contrast, uint8_t* out,
                                void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (n_img < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_jitter: n_img %d < 1", n_img);
    if (in_channels != 1 && in_channels != 3) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_jitter: in_channels %d is neither 1 nor 3", in_channels);
    if (!pixels || !offs || !hs || !ws || !out) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_jitter: pixels, offs, hs, ws or out is NULL");
    if (!brightness && !contrast) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_jitter: brightness and contrast are both NULL");
    if (max_h < 1 || max_w < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_jitter: max dims");
    hipStream_t st = (hipStream_t)stream;
    // units of the largest ROI: its bytes plus up to 15 in front of it in its first unit
    const int64_t units = ((int64_t)max_h * max_w * in_channels + 15 + 15) >> 4;
    int64_t chunks = (units + JT * JUNITS - 1) / (JT * JUNITS);
    if (chunks > 65535) chunks = 65535;                            // the kernels stride over the chunks beyond the grid
    const dim3 grid((unsigned)n_img, (unsigned)chunks);
    unsigned long long* sums = nullptr;
    if (contrast) {
        const size_t need = ifcbk_roi_jitter_workspace(n_img);
        if (need > ctx->ws_bytes) IFCBK_FAIL(ctx, IFCBK_ENOMEM, "roi_jitter: workspace %zu > reserved %zu", need, ctx->ws_bytes);
        sums = (unsigned long long*)ctx->ws;
        IFCBK_HIP(ctx, hipMemsetAsync(sums, 0, need, st));
        hipLaunchKernelGGL(roi_jitter_sum_kernel, grid, dim3(JT), 0, st, pixels, offs, hs, ws, in_channels, brightness, sums);
        IFCBK_LAUNCH_CHECK(ctx, "roi_jitter_sum");
    }
    const int vec_store = (((uintptr_t)out ^ (uintptr_t)pixels) & 15) == 0;
    hipLaunchKernelGGL(roi_jitter_apply_kernel, grid, dim3(JT), 0, st, pixels, offs, hs, ws, in_channels, brightness, contrast, sums, out,
                       vec_store);
    IFCBK_LAUNCH_CHECK(ctx, "roi_jitter_apply");
    return 0;
}
