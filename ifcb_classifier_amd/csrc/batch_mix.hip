// Batch mixing (TRAIN --mixup / --cutmix): ifcbk_batch_mix mixes a resized batch IN PLACE with its reverse (timm's Mixup, batch mode:
// the partner of image n is m = N - 1 - n).  With lam[] one factor per image and the box [y0, y1) x [x0, x1):
//     inside the box    x'[n] = x[m]                                   (a copy of the partner's bytes)
//     outside it        x'[n] = fmaf(lam[n], x[n] - x[m], x[m])        in fp32; lam[n] == 1 keeps x[n]'s bytes
// One block owns a piece of a PAIR (n, m), n < N / 2: it reads both images' bytes of the piece, then writes both, and no other block
// touches those bytes -- that is what makes the in-place form free of races.  The middle image of an odd batch is its own partner
// and is left alone; N == 1 launches nothing.
//
// Dense form ([N,S,S,8] bf16 or fp32): an image is a multiple of 16 bytes, so the partners are aligned alike (the tensor itself has to
// be 16-byte aligned): one 16-byte load and store per chunk and image, chunks grid-strided.
//
// u8 form ([N,S,S] bytes): an image is S * S bytes -- 89,401 at S = 299 -- so neither the images nor the partners relative to each
// other are aligned to anything.  A block takes a chunk of MCH bytes cut on the 16-byte units of image n's ABSOLUTE address ("A-frame"):
//     A side  thread t owns unit t of the chunk: one 16-byte load and one 16-byte store (the image's first and last unit byte by byte)
//     B side  the same relative byte range of image m starts anywhere.  Its aligned body is loaded with 16-byte loads of ITS units into
//             LDS ("B-frame", LDS addresses aligned like the global ones), its ends -- at most 15 bytes each -- byte by byte; thread t
//             then reads the 16 bytes opposite its A unit as two aligned 16-byte LDS words and a funnel shift by the chunk's uniform byte
//             offset.  The results for B go to LDS in the A-frame, and the B units are read back the same way (two words, funnel shift)
//             and stored with 16-byte stores; the ends byte by byte.
// A chunk's range of B is cut out of the middle of image m, so the "ends" of the B side are the ends of the chunk: up to 30 single-byte
// accesses per 4 KiB.  A 16-byte store over a unit that straddles two chunks would race with the neighbouring block.
// No byte outside [0, N * S * S) is read or written.
#include "common.h"

namespace {

constexpr int MT = 256;               // threads per block
constexpr int MCH = MT * 16;          // bytes of a u8 chunk

// 16 bytes starting at byte s (0..15, uniform) of the 32 bytes (lo, hi)
__device__ __forceinline__ uint4 funnel16(const uint4& lo, const uint4& hi, unsigned s) {
    unsigned w0 = lo.x, w1 = lo.y, w2 = lo.z, w3 = lo.w, w4 = hi.x, w5 = hi.y, w6 = hi.z, w7 = hi.w;
    if (s & 8) { w0 = w2; w1 = w3; w2 = w4; w3 = w5; w4 = w6; w5 = w7; }
    if (s & 4) { w0 = w1; w1 = w2; w2 = w3; w3 = w4; w4 = w5; }
    const unsigned r = (s & 3) * 8;
    uint4 o;
    o.x = (unsigned)((((uint64_t)w1 << 32) | w0) >> r);
    o.y = (unsigned)((((uint64_t)w2 << 32) | w1) >> r);
    o.z = (unsigned)((((uint64_t)w3 << 32) | w2) >> r);
    o.w = (unsigned)((((uint64_t)w4 << 32) | w3) >> r);
    return o;
}

__device__ __forceinline__ unsigned mix_u8(float lam, unsigned a, unsigned b) {
    if (lam == 1.0f) return a;
    const float v = fmaf(lam, (float)((int)a - (int)b), (float)b);
    return (unsigned)(uint8_t)(int)(v + 0.5f);
}

__global__ __launch_bounds__(MT) void batch_mix_u8_kernel(uint8_t* x, int N, int S, const float* lam, int y0, int y1, int x0, int x1) {
    __shared__ __attribute__((aligned(16))) uint8_t sB[MCH + 64];      // image m's bytes of the chunk, B-frame
    __shared__ __attribute__((aligned(16))) uint8_t sO[MCH + 64];      // image m's results, A-frame
    const int n = blockIdx.x, m = N - 1 - n, t = threadIdx.x;
    const int64_t L = (int64_t)S * S;
    uint8_t* A = x + (int64_t)n * L;
    uint8_t* B = x + (int64_t)m * L;
    const float la = lam[n], lb = lam[m];
    const int64_t headA = (int64_t)((uintptr_t)A & 15);
    const int64_t nchunk = (headA + L + MCH - 1) / MCH;
    for (int64_t k = blockIdx.y; k < nchunk; k += gridDim.y) {
        const int64_t base = k * MCH - headA;                          // image-relative byte of A-frame index 0 (negative in chunk 0)
        const int64_t lo = base > 0 ? base : 0, hi = base + MCH < L ? base + MCH : L;
        // ---- B side in: [B + lo, B + hi) into sB at index (address - oB), oB = ub0 - 32
        const uintptr_t pb0 = (uintptr_t)(B + lo), pb1 = (uintptr_t)(B + hi);
        const uintptr_t ub0 = (pb0 + 15) & ~(uintptr_t)15, ub1 = pb1 & ~(uintptr_t)15;      // the aligned body [ub0, ub1), empty if ub0 >= ub1
        const uintptr_t hend = ub0 < pb1 ? ub0 : pb1;                                      // head bytes [pb0, hend)
        const uintptr_t tbeg = ub1 > hend ? ub1 : hend;                                    // tail bytes [tbeg, pb1)
        const uintptr_t oB = ub0 - 32;
        {
            const uintptr_t u = ub0 + 16 * (uintptr_t)t;
            if (u + 16 <= ub1) *reinterpret_cast<uint4*>(sB + 32 + 16 * t) = *reinterpret_cast<const uint4*>(u);
            if (pb0 + t < hend) sB[pb0 + t - oB] = *reinterpret_cast<const uint8_t*>(pb0 + t);
            if (tbeg + t < pb1) sB[tbeg + t - oB] = *reinterpret_cast<const uint8_t*>(tbeg + t);
        }
        // ---- A side in: this thread's unit
        const int64_t rel = base + 16 * t;                             // image-relative byte of the unit's first byte
        const bool any = rel + 16 > 0 && rel < L, full = rel >= 0 && rel + 16 <= L;
        unsigned wa[4] = {0, 0, 0, 0};
        if (full) {
            const uint4 v = *reinterpret_cast<const uint4*>(A + rel);
            wa[0] = v.x; wa[1] = v.y; wa[2] = v.z; wa[3] = v.w;
        } else if (any) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (rel + j >= 0 && rel + j < L) wa[j >> 2] |= (unsigned)A[rel + j] << (8 * (j & 3));
        }
        __syncthreads();
        // ---- the 16 bytes of B opposite the unit: sB index 16 t + dB, dB = (B + base) - oB in [2, 32]
        const unsigned dB = (unsigned)((int64_t)pb0 - (lo - base) - (int64_t)oB);
        const unsigned ib = 16 * t + dB;
        const uint4 vb = funnel16(*reinterpret_cast<const uint4*>(sB + (ib & ~15u)), *reinterpret_cast<const uint4*>(sB + (ib & ~15u) + 16), ib & 15);
        const unsigned wb[4] = {vb.x, vb.y, vb.z, vb.w};
        unsigned oa[4] = {0, 0, 0, 0}, ob[4] = {0, 0, 0, 0};
        if (any) {
            const int64_t r0 = rel > 0 ? rel : 0;
            int py = (int)((unsigned)r0 / (unsigned)S), px = (int)((unsigned)r0 - (unsigned)py * (unsigned)S);       // (L <= 2^30)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned a = (wa[j >> 2] >> (8 * (j & 3))) & 0xff, b = (wb[j >> 2] >> (8 * (j & 3))) & 0xff;
                unsigned ra = a, rb = b;
                if (rel + j >= 0 && rel + j < L) {
                    if (py >= y0 && py < y1 && px >= x0 && px < x1) {
                        ra = b; rb = a;
                    } else {
                        ra = mix_u8(la, a, b); rb = mix_u8(lb, b, a);
                    }
                    if (++px == S) { px = 0; ++py; }
                }
                oa[j >> 2] |= ra << (8 * (j & 3));
                ob[j >> 2] |= rb << (8 * (j & 3));
            }
        }
        // ---- A side out
        if (full) {
            *reinterpret_cast<uint4*>(A + rel) = make_uint4(oa[0], oa[1], oa[2], oa[3]);
        } else if (any) {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (rel + j >= 0 && rel + j < L) A[rel + j] = (uint8_t)(oa[j >> 2] >> (8 * (j & 3)));
        }
        // ---- B side out: through sO (A-frame: index i is image-relative byte base + i), read back on B's units
        *reinterpret_cast<uint4*>(sO + 16 * t) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
        __syncthreads();
        {
            const uintptr_t fB = (uintptr_t)((int64_t)pb0 - (lo - base));          // address of B-image byte `base` (may lie in front of B)
            const uintptr_t u = ub0 + 16 * (uintptr_t)t;
            if (u + 16 <= ub1) {
                const unsigned io = (unsigned)(u - fB);                            // 16 t + e, e in [0, 30]
                *reinterpret_cast<uint4*>(u) =
                    funnel16(*reinterpret_cast<const uint4*>(sO + (io & ~15u)), *reinterpret_cast<const uint4*>(sO + (io & ~15u) + 16), io & 15);
            }
            if (pb0 + t < hend) *reinterpret_cast<uint8_t*>(pb0 + t) = sO[pb0 + t - fB];
            if (tbeg + t < pb1) *reinterpret_cast<uint8_t*>(tbeg + t) = sO[tbeg + t - fB];
        }
        __syncthreads();                   // (the next chunk overwrites sB and sO)
    }
}

// dense form: T = bf16_t (8 channels per 16-byte chunk = one pixel) or float (4 channels per chunk, two chunks per pixel)
template <class T>
__global__ __launch_bounds__(MT) void batch_mix_dense_kernel(T* x, int N, int S, const float* lam, int y0, int y1, int x0, int x1) {
    constexpr int CN = Chunk<T>::N, CPP = 8 / CN;
    const int n = blockIdx.x, m = N - 1 - n;
    const int64_t nchunk = (int64_t)S * S * CPP;
    T* A = x + (int64_t)n * nchunk * CN;
    T* B = x + (int64_t)m * nchunk * CN;
    const float la = lam[n], lb = lam[m];
    for (int64_t c = (int64_t)blockIdx.y * MT + threadIdx.x; c < nchunk; c += (int64_t)gridDim.y * MT) {
        const unsigned pix = (unsigned)(c / CPP);                      // (S * S <= 2^30)
        const int py = (int)(pix / (unsigned)S), px = (int)(pix - (unsigned)py * (unsigned)S);
        uint4* pa = reinterpret_cast<uint4*>(A + c * CN);
        uint4* pb = reinterpret_cast<uint4*>(B + c * CN);
        const uint4 ra = *pa, rb = *pb;
        if (py >= y0 && py < y1 && px >= x0 && px < x1) {
            *pa = rb;
            *pb = ra;
            continue;
        }
        float fa[CN], fb[CN], o[CN];
        Chunk<T>::widen(__builtin_bit_cast(typename Chunk<T>::raw_t, ra), fa);
        Chunk<T>::widen(__builtin_bit_cast(typename Chunk<T>::raw_t, rb), fb);
        if (la != 1.0f) {
#pragma unroll
            for (int j = 0; j < CN; ++j) o[j] = fmaf(la, fa[j] - fb[j], fb[j]);
            Chunk<T>::store(A + c * CN, o);
        }
        if (lb != 1.0f) {
#pragma unroll
            for (int j = 0; j < CN; ++j) o[j] = fmaf(lb, fb[j] - fa[j], fa[j]);
            Chunk<T>::store(B + c * CN, o);
        }
    }
}

}  // namespace

extern "C" int ifcbk_batch_mix(ifcbk_ctx* ctx, void* x, int kind, int N, int S, const float* lam, int y0, int y1, int x0, int x1,
                               void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!x || !lam) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: x or lam is NULL");
    if (N < 1 || S < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: N %d or S %d < 1", N, S);
    if (S > 32768) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: S %d > 32768", S);
    if (kind != IFCBK_MIX_U8 && kind != IFCBK_BF16 && kind != IFCBK_F32) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: kind %d", kind);
    if (y0 < 0 || y1 > S || x0 < 0 || x1 > S || y0 > y1 || x0 > x1)
        IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: box [%d, %d) x [%d, %d) is not inside [0, %d] or is reversed", y0, y1, x0, x1, S);
    if (kind != IFCBK_MIX_U8 && ((uintptr_t)x & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_mix: a dense tensor must be 16-byte aligned");
    const int pairs = N / 2;
    if (pairs == 0) return IFCBK_OK;
    hipStream_t st = (hipStream_t)stream;
    // up to 4096 blocks in all (two rounds of 8 per CU); the kernels stride over what lies beyond the grid
    const int64_t L = (int64_t)S * S;
    int64_t work = kind == IFCBK_MIX_U8 ? (L + 15 + MCH - 1) / MCH : (L * (kind == IFCBK_F32 ? 2 : 1) + MT - 1) / MT;
    int64_t gy = 4096 / pairs;
    if (gy > work) gy = work;
    if (gy > 65535) gy = 65535;
    if (gy < 1) gy = 1;
    const dim3 grid((unsigned)pairs, (unsigned)gy);
    if (kind == IFCBK_MIX_U8) {
        hipLaunchKernelGGL(batch_mix_u8_kernel, grid, dim3(MT), 0, st, (uint8_t*)x, N, S, lam, y0, y1, x0, x1);
    } else if (kind == IFCBK_BF16) {
        hipLaunchKernelGGL(batch_mix_dense_kernel<bf16_t>, grid, dim3(MT), 0, st, (bf16_t*)x, N, S, lam, y0, y1, x0, x1);
    } else {
        hipLaunchKernelGGL(batch_mix_dense_kernel<float>, grid, dim3(MT), 0, st, (float*)x, N, S, lam, y0, y1, x0, x1);
    }
    IFCBK_LAUNCH_CHECK(ctx, "batch_mix");
    return IFCBK_OK;
}
