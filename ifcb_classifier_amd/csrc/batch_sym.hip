// Symmetry views of a resized batch (RUN --tta): ifcbk_batch_sym applies one generator of the square's symmetry group to every image of
// a batch IN PLACE, where the batch already lies -- the u8 plane [N][S][S] or the dense tensor [N][S][S][8]:
//     IFCBK_SYM_HFLIP      x'[n][r][c] = x[n][r][S-1-c]
//     IFCBK_SYM_VFLIP      x'[n][r][c] = x[n][S-1-r][c]
//     IFCBK_SYM_TRANSPOSE  x'[n][r][c] = x[n][c][r]
// Every result is a permutation of the input's pixels: bytes are moved, never computed.  Each op is an involution that exchanges the
// pixels of a rectangle A of an image with those of its image rectangle B (A' = f(B), B' = f(A)), and the rectangles of an op tile the
// pixels that move.  The in-place form is free of races for the reason batch_mix.hip states: a block owns a set of bytes that no other
// block touches, reads all of them, then writes them.
//     HFLIP      A = a band of rows x a run of columns left of the middle, B = the same rows x the mirrored run.  The bands and runs of
//                a row band together are whole rows; the middle column of an odd S is left alone.
//     VFLIP      A = a band of rows above the middle x a run of columns, B = the mirrored band.  The middle row of an odd S is left alone.
//     TRANSPOSE  A = tile (I, J), B = tile (J, I), I <= J; a diagonal tile is its own partner (read once, written once).
//
// u8 form ([N][S][S] bytes, any address): at S = 299 neither images nor rows are aligned to anything, so a rectangle's row segment
// [g, g + w) starts anywhere.  It is cut on the 16-byte units of its ABSOLUTE address: a unit that lies inside the segment is one
// 16-byte load / store, a unit that the segment only partly covers (its first and last: at most 15 bytes each) goes byte by byte -- a
// 16-byte store over such a unit would write bytes of the neighbouring rectangle, which another block owns.  Both rectangles are staged
// in LDS row by row in the frame of their global address (LDS byte = global byte mod 16, so the wide accesses are aligned on both
// sides); after the barrier every destination unit is gathered byte by byte from the partner's tile and stored.
//
// Dense form ([N][S][S][8] bf16 or fp32, 16-byte aligned): a pixel is one (bf16) or two (fp32) 16-byte pieces and moves whole.  The
// flips need no staging: a thread owns a piece and its mirror piece, loads both, stores both, and both sides are coalesced.  The
// transpose stages its two tiles of 16 x 16 pixels in LDS so that reads and writes both run along rows.
// No byte outside [0, N * S * S * bytes per pixel) is read or written.  S == 1 launches nothing.
#include "common.h"

namespace {

constexpr int YT = 256;               // threads per block
constexpr int TU = 64;                // u8: edge of a rectangle, pixels
constexpr int UPR = TU / 16 + 1;      // u8: 16-byte units that cover a row segment of up to TU bytes at any address
constexpr int PU = 16 * UPR;          // u8: LDS bytes per rectangle row
constexpr int TD = 16;                // dense transpose: edge of a tile, pixels

struct Rect {
    int r0, c0, h, w;
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// rectangles per image (host and device agree on the count)
static __host__ __device__ inline int64_t sym_items(int op, int S, int T) {
    const int64_t full = (S + T - 1) / T, half = (S / 2 + T - 1) / T;
    return op == IFCBK_SYM_TRANSPOSE ? full * (full + 1) / 2 : full * half;
}

// item `it` of an image -> the rectangle pair (A, B); true when A is its own partner (a diagonal tile of the transpose)
template <int OP>
__device__ __forceinline__ bool sym_rects(int S, int T, int64_t it, Rect& A, Rect& B) {
    const int full = (S + T - 1) / T, half = S / 2;
    if (OP == IFCBK_SYM_HFLIP) {
        const int nc = (half + T - 1) / T;
        const int rb = (int)(it / nc), cb = (int)(it - (int64_t)rb * nc);
        A = {rb * T, cb * T, imin(T, S - rb * T), imin(T, half - cb * T)};
        B = {A.r0, S - A.c0 - A.w, A.h, A.w};
        return false;
    }
    if (OP == IFCBK_SYM_VFLIP) {
        const int rb = (int)(it / full), cb = (int)(it - (int64_t)rb * full);
        A = {rb * T, cb * T, imin(T, half - rb * T), imin(T, S - cb * T)};
        B = {S - A.r0 - A.h, A.c0, A.h, A.w};
        return false;
    }
    int I = 0;
    int64_t p = it;
    while (p >= full - I) {          // row I of the upper triangle holds the tiles (I, I) .. (I, full - 1)
        p -= full - I;
        ++I;
    }
    const int J = I + (int)p;
    A = {I * T, J * T, imin(T, S - I * T), imin(T, S - J * T)};
    B = {J * T, I * T, A.w, A.h};
    return I == J;
}

// pixel (i, j) of a destination rectangle of height h and width w comes from pixel (si, sj) of its partner
template <int OP>
__device__ __forceinline__ void sym_src(int h, int w, int i, int j, int& si, int& sj) {
    if (OP == IFCBK_SYM_HFLIP) { si = i; sj = w - 1 - j; }
    else if (OP == IFCBK_SYM_VFLIP) { si = h - 1 - i; sj = j; }
    else { si = j; sj = i; }
}

// ---- u8 plane.  A tile holds row i of its rectangle at t + i * PU, in the frame of the row's global address: pixel (i, j) lies at
// t[i * PU + ph_i + j], ph_i = (address of the row segment) & 15.  `lo` is the low 4 bits of the image's address.
__device__ __forceinline__ int row_phase(unsigned lo, int S, const Rect& R, int i) {
    return (int)((lo + (unsigned)(R.r0 + i) * (unsigned)S + (unsigned)R.c0) & 15u);       // ((r0 + i) * S + c0 < 2^30)
}

__device__ __forceinline__ void load_u8(uint8_t* t, uintptr_t img, int S, const Rect& R) {
    for (int s = threadIdx.x; s < R.h * UPR; s += YT) {
        const int i = s / UPR, k = s - i * UPR;
        const uintptr_t g = img + (uintptr_t)((int64_t)(R.r0 + i) * S + R.c0);            // the row segment [g, g + w)
        const int ph = (int)(g & 15);
        const int lo = imax(ph - 16 * k, 0), hi = imin(ph + R.w - 16 * k, 16);             // the segment's bytes of unit k: [lo, hi)
        if (hi <= lo) continue;
        const uintptr_t u = g - ph + 16 * k;
        uint8_t* d = t + i * PU + 16 * k;
        if (lo == 0 && hi == 16) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(u);
        } else {
            for (int b = lo; b < hi; ++b) d[b] = *reinterpret_cast<const uint8_t*>(u + b);
        }
    }
}

// the rectangle D of the image from the tile t of its partner Q
template <int OP>
__device__ __forceinline__ void store_u8(uintptr_t img, int S, const Rect& D, const uint8_t* t, const Rect& Q) {
    const unsigned ilo = (unsigned)(img & 15);
    for (int s = threadIdx.x; s < D.h * UPR; s += YT) {
        const int i = s / UPR, k = s - i * UPR;
        const uintptr_t g = img + (uintptr_t)((int64_t)(D.r0 + i) * S + D.c0);
        const int ph = (int)(g & 15);
        const int lo = imax(ph - 16 * k, 0), hi = imin(ph + D.w - 16 * k, 16);
        if (hi <= lo) continue;
        const uintptr_t u = g - ph + 16 * k;
        unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            if (b >= lo && b < hi) {
                int si, sj;
                sym_src<OP>(D.h, D.w, i, 16 * k + b - ph, si, sj);
                o[b >> 2] |= (unsigned)t[si * PU + row_phase(ilo, S, Q, si) + sj] << (8 * (b & 3));
            }
        }
        if (lo == 0 && hi == 16) {
            *reinterpret_cast<uint4*>(u) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b >= lo && b < hi) *reinterpret_cast<uint8_t*>(u + b) = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
        }
    }
}

template <int OP>
__global__ __launch_bounds__(YT) void batch_sym_u8_kernel(uint8_t* x, int S, int64_t per_image, int64_t total) {
    __shared__ __attribute__((aligned(16))) uint8_t sT[2][TU * PU];
    const int64_t L = (int64_t)S * S;
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {       // (block-uniform: every thread meets every barrier)
        const int64_t n = it / per_image;
        Rect A, B;
        const bool self = sym_rects<OP>(S, TU, it - n * per_image, A, B);
        const uintptr_t img = (uintptr_t)x + (uintptr_t)(n * L);
        load_u8(sT[0], img, S, A);
        if (!self) load_u8(sT[1], img, S, B);
        __syncthreads();
        if (self) {
            store_u8<OP>(img, S, A, sT[0], A);
        } else {
            store_u8<OP>(img, S, A, sT[1], B);
            store_u8<OP>(img, S, B, sT[0], A);
        }
        __syncthreads();                   // (the next item overwrites the tiles)
    }
}

// ---- dense tensor, in 16-byte pieces: PC pieces per pixel (1: bf16, 2: fp32)
// the flips: piece q of the `total` pieces that have a partner; a thread loads it and its mirror piece, then stores both
template <int OP, int PC>
__global__ __launch_bounds__(YT) void batch_sym_flip_dense_kernel(uint4* x, int S, int64_t total) {
    const int half = S / 2;
    for (int64_t q = (int64_t)blockIdx.x * YT + threadIdx.x; q < total; q += (int64_t)gridDim.x * YT) {
        const int64_t pix = q / PC;
        const int e = (int)(q - pix * PC);
        int64_t a, b;                      // pixel indices of the pair
        if (OP == IFCBK_SYM_HFLIP) {       // pix = (n * S + r) * half + c
            const int64_t row = pix / half;
            const int c = (int)(pix - row * half);
            a = row * S + c;
            b = row * S + (S - 1 - c);
        } else {                           // pix = (n * half + r) * S + c
            const int64_t nr = pix / S;
            const int c = (int)(pix - nr * S);
            const int64_t n = nr / half;
            const int r = (int)(nr - n * half);
            a = (n * S + r) * S + c;
            b = (n * S + (S - 1 - r)) * S + c;
        }
        uint4* pa = x + a * PC + e;
        uint4* pb = x + b * PC + e;
        const uint4 va = *pa, vb = *pb;
        *pa = vb;
        *pb = va;
    }
}

template <int PC>
__global__ __launch_bounds__(YT) void batch_sym_transpose_dense_kernel(uint4* x, int S, int64_t per_image, int64_t total) {
    constexpr int PD = TD * PC + 1;        // LDS pieces per tile row (odd: the column reads of the write-back spread over the banks)
    __shared__ uint4 sT[2][TD * PD];
    for (int64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t n = it / per_image;
        Rect R[2];
        const bool self = sym_rects<IFCBK_SYM_TRANSPOSE>(S, TD, it - n * per_image, R[0], R[1]);
        uint4* img = x + n * S * S * PC;
        const int nr = self ? 1 : 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nr) break;
            const int rowp = R[k].w * PC;
            for (int s = threadIdx.x; s < R[k].h * rowp; s += YT) {
                const int i = s / rowp, q = s - i * rowp;
                sT[k][i * PD + q] = img[((int64_t)(R[k].r0 + i) * S + R[k].c0) * PC + q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k >= nr) break;
            const uint4* t = sT[self ? 0 : 1 - k];      // pixel (i, j) of R[k] is pixel (j, i) of its partner
            const int rowp = R[k].w * PC;
            for (int s = threadIdx.x; s < R[k].h * rowp; s += YT) {
                const int i = s / rowp, q = s - i * rowp;
                const int j = q / PC, e = q - j * PC;
                img[((int64_t)(R[k].r0 + i) * S + R[k].c0) * PC + q] = t[j * PD + i * PC + e];
            }
        }
        __syncthreads();
    }
}

// up to 4096 blocks (two rounds of 8 per CU); the kernels stride over what lies beyond the grid
inline unsigned sym_grid(int64_t work) { return (unsigned)(work < 4096 ? work : 4096); }

template <int OP>
void launch_sym(void* x, int kind, int N, int S, hipStream_t st) {
    if (kind == IFCBK_MIX_U8) {
        const int64_t per = sym_items(OP, S, TU), total = per * N;
        hipLaunchKernelGGL(batch_sym_u8_kernel<OP>, dim3(sym_grid(total)), dim3(YT), 0, st, (uint8_t*)x, S, per, total);
    } else if (OP == IFCBK_SYM_TRANSPOSE) {
        const int64_t per = sym_items(OP, S, TD), total = per * N;
        if (kind == IFCBK_BF16)
            hipLaunchKernelGGL(batch_sym_transpose_dense_kernel<1>, dim3(sym_grid(total)), dim3(YT), 0, st, (uint4*)x, S, per, total);
        else
            hipLaunchKernelGGL(batch_sym_transpose_dense_kernel<2>, dim3(sym_grid(total)), dim3(YT), 0, st, (uint4*)x, S, per, total);
    } else {
        const int64_t pairs = (int64_t)N * S * (S / 2);
        if (kind == IFCBK_BF16)
            hipLaunchKernelGGL((batch_sym_flip_dense_kernel<OP, 1>), dim3(sym_grid((pairs + YT - 1) / YT)), dim3(YT), 0, st, (uint4*)x, S, pairs);
        else
            hipLaunchKernelGGL((batch_sym_flip_dense_kernel<OP, 2>), dim3(sym_grid((2 * pairs + YT - 1) / YT)), dim3(YT), 0, st, (uint4*)x, S,
                               2 * pairs);
    }
}

}  // namespace

extern "C" int ifcbk_batch_sym(ifcbk_ctx* ctx, void* x, int kind, int N, int S, int op, void* stream) {
    if (!ctx) return IFCBK_EINVAL;
    if (!x) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: x is NULL");
    if (N < 1 || S < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: N %d or S %d < 1", N, S);
    if (S > 32768) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: S %d > 32768", S);
    if (kind != IFCBK_MIX_U8 && kind != IFCBK_BF16 && kind != IFCBK_F32) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: kind %d", kind);
    if (op != IFCBK_SYM_HFLIP && op != IFCBK_SYM_VFLIP && op != IFCBK_SYM_TRANSPOSE)
        IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: op %d is not exactly one of HFLIP (1), VFLIP (2), TRANSPOSE (4)", op);
    if (kind != IFCBK_MIX_U8 && ((uintptr_t)x & 15)) IFCBK_FAIL(ctx, IFCBK_EINVAL, "batch_sym: a dense tensor must be 16-byte aligned");
    if (S == 1) return IFCBK_OK;
    hipStream_t st = (hipStream_t)stream;
    if (op == IFCBK_SYM_HFLIP) launch_sym<IFCBK_SYM_HFLIP>(x, kind, N, S, st);
    else if (op == IFCBK_SYM_VFLIP) launch_sym<IFCBK_SYM_VFLIP>(x, kind, N, S, st);
    else launch_sym<IFCBK_SYM_TRANSPOSE>(x, kind, N, S, st);
    IFCBK_LAUNCH_CHECK(ctx, "batch_sym");
    return IFCBK_OK;
}
