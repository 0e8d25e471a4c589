// Pillow's two-pass 8-bit bilinear resample (antialiased, 22-bit fixed-point taps, a u8 intermediate between the passes), once,
// for the three ROI resize kernel sets: roi.hip (squash), roi_turn.hip (quarter turns), roi_fit.hip (aspect-preserving).
// Restates libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc (roi_taps), ImagingResampleHorizontal_8bpc /
// Vertical_8bpc (two_pass, three_tap).  Each file keeps what is its own: which size feeds which axis, where a pixel of the
// image the resize sees lives in memory, what it stages in LDS, and its dispatch.  Everything here is force-inlined.
#pragma once
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// threads per output row of every resize kernel
inline int roi_row_threads(int S) { return S <= 64 ? 64 : S <= 128 ? 128 : S <= 192 ? 192 : S <= 256 ? 256 : 320; }

// Bounds and int taps of output index xx of an axis resized from inSize to outSize, written to the tap table.
// Table layout [image][axis][field][S] (axis 0 = horizontal; field 0 = first input index, 1 = tap count, 2.. = kmax taps, zeros
// beyond the count): `row` points at field 0 of (image, axis, xx) and fieldStride = S, so the resize kernel's threads (consecutive
// output x) read consecutive words of each field.
// IEEE double with contraction off -- the pragma stands in this body because the library is built with -ffp-contract=on, and it
// has to hold after inlining -- so the taps are bit-identical to the CPU's.
__device__ __forceinline__ void roi_taps(int inSize, int outSize, int xx, int kmax, int32_t* row, int fieldStride) {
#pragma clang fp contract(off)
    double scale = (double)((float)inSize - 0.0f) / (double)outSize;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    double support = 1.0 * filterscale;              // bilinear support = 1.0
    double center = 0.0 + ((double)xx + 0.5) * scale;
    double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    if (xmax > kmax) xmax = kmax;                     // cannot happen when kmax is sized from max dims (roi_fit.hip: ifcbk_fit_kmax)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        double a = ((double)(x + xmin) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        double w = a < 1.0 ? 1.0 - a : 0.0;
        ww += w;
    }
    for (int x = 0; x < kmax; ++x) {
        int kq = 0;
        if (x < xmax) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            double w = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) w = w / ww;
            kq = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
        }
        row[(size_t)(2 + x) * fieldStride] = kq;
    }
    row[0] = xmin;
    row[fieldStride] = xmax;
}

// kernel arguments of the squash and turn kernels; roi_fit.hip extends them
struct RoiArgs {
    const uint8_t* pixels;
    const int64_t* offs;
    const int32_t* hs;     // hs / ws: null in a FitArgs (its kernels read the dims the setup kernel cut, from meta); nothing in this
    const int32_t* ws;     // header reads them
    const uint8_t* flips;  // per-image code byte or null; bit 2 (transpose) counts in roi_turn.hip, and in roi_fit.hip under codemask
    const int32_t* tab;
    void* out;
    int f32;
    uint8_t* out_u8;
    int n_img, S, cin, cout, kmax;
    float mean[3], std[3], tsc[3], tsh[3];
};

// the descriptor's part of the arguments
inline void roi_args_desc(RoiArgs& a, const ifcbk_roi_desc* d, int kmax) {
    a.f32 = d->dtype == IFCBK_F32;
    a.n_img = d->n_img; a.S = d->S; a.cin = d->in_channels; a.cout = d->out_channels; a.kmax = kmax;
    for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.std[i] = d->std[i]; a.tsc[i] = d->tin_scale[i]; a.tsh[i] = d->tin_shift[i]; }
}

// The float stage and the stores for output pixel `i`.  `level` is an expression in `c` for the resized u8 level of channel c
// (`res[c]`, or one scalar from a kernel whose three channels are equal); `cin` is the channel count of the u8 plane: a.cin, or a
// literal 1 from a kernel that runs grey batches only (one byte store).
// A macro, so that the text stands in the kernel and the argument block is read field by field where it is used: a function
// takes the block by reference or by value, and the kernels then keep its fields in registers from the call or from kernel
// entry on (DESIGN 3.1a has the register counts).
#define ROI_STORE_PIXEL(a, i, cin, level)                                                                  \
    do {                                                                                                   \
        const int64_t i_ = (i);                                                                            \
        if ((a).out_u8)                                                                                    \
            for (int c = 0; c < (cin); ++c) (a).out_u8[i_ * (cin) + c] = (uint8_t)(level);                 \
        if ((a).out) {                                                                                     \
            for (int c0_ = 0; c0_ < (a).cout; c0_ += 8) {                                                  \
                float f_[8];                                                                               \
                _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                                         \
                    const int c = c0_ + j_;                                                                \
                    float v_ = 0.f;                                                                        \
                    if (c < 3) {                                                                           \
                        v_ = (float)(level) / 255.0f;                                                      \
                        v_ = (v_ - (a).mean[c]) / (a).std[c];                                              \
                        v_ = v_ * (a).tsc[c] + (a).tsh[c];                                                 \
                    }                                                                                      \
                    f_[j_] = v_;                                                                           \
                }                                                                                          \
                if ((a).f32) {                                                                             \
                    float* o_ = (float*)(a).out + i_ * (a).cout + c0_;                                     \
                    *reinterpret_cast<float4*>(o_) = make_float4(f_[0], f_[1], f_[2], f_[3]);              \
                    *reinterpret_cast<float4*>(o_ + 4) = make_float4(f_[4], f_[5], f_[6], f_[7]);          \
                } else {                                                                                   \
                    *reinterpret_cast<uint4*>((bf16_t*)(a).out + i_ * (a).cout + c0_) = pack8(f_);         \
                }                                                                                          \
            }                                                                                              \
        }                                                                                                  \
    } while (0)

// The two passes for one output pixel and channel.  px(j, k) is the source level under tap j of the vertical window and tap k of
// the horizontal one (an LDS row image or a global address, flips and turns applied by the caller); th / tv point at field 0 of
// the pixel's horizontal / vertical table entry, TS is the field stride.  Horizontal pass first, as Pillow's Image.resize runs
// them, unless vfirst (Pillow's rule for a ROI more than 100 times as tall as wide that shrinks in height: the 8-bit intermediate
// makes the order visible by one level).
template <class Px>
__device__ __forceinline__ int two_pass(Px px, const int32_t* th, int xn, const int32_t* tv, int yn, int TS, bool vfirst) {
    if (vfirst) {
        int acch = 1 << (PRECISION_BITS - 1);
        for (int k = 0; k < xn; ++k) {
            int accv = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < yn; ++j) accv += px(j, k) * tv[(size_t)(2 + j) * TS];
            acch += clip8(accv) * th[(size_t)(2 + k) * TS];
        }
        return clip8(acch);
    }
    int accv = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < yn; ++j) {
        int acch = 1 << (PRECISION_BITS - 1);
        for (int k = 0; k < xn; ++k) acch += px(j, k) * th[(size_t)(2 + k) * TS];
        accv += clip8(acch) * tv[(size_t)(2 + j) * TS];
    }
    return clip8(accv);
}

// ---- the fixed three-tap form (kmax == 3: no ROI larger than the output; always horizontal first, see roi.hip)
// A thread's three columns and horizontal taps.  A window of fewer than three pixels repeats its last column under a zero tap.
struct Tap3 { int c[3], t[3]; };

__device__ __forceinline__ Tap3 tap3_load(const int32_t* th, int TS, bool hflip, int wt) {
    const int xmin = th[0], xn = th[TS];
    Tap3 h;
    h.t[0] = th[2 * TS]; h.t[1] = th[3 * TS]; h.t[2] = th[4 * TS];
    h.c[0] = xmin; h.c[1] = xmin + (xn > 1 ? 1 : 0); h.c[2] = xmin + (xn > 2 ? 2 : xn - 1);
    if (hflip) { h.c[0] = wt - 1 - h.c[0]; h.c[1] = wt - 1 - h.c[1]; h.c[2] = wt - 1 - h.c[2]; }
    return h;
}

// columns clamped to the wl staged ones: a table entry that breaks the kmax == 3 promise (stale maxima from the caller) gives a
// wrong pixel, never an LDS read out of what was staged
__device__ __forceinline__ void tap3_clamp(Tap3& h, int wl) {
#pragma unroll
    for (int k = 0; k < 3; ++k) h.c[k] = h.c[k] < 0 ? 0 : (h.c[k] >= wl ? wl - 1 : h.c[k]);
}

// s0..s2: the LDS images of the three source rows under the vertical window, tv3 their vertical taps
__device__ __forceinline__ int three_tap(const uint8_t* s0, const uint8_t* s1, const uint8_t* s2, const int* tv3, const Tap3& h) {
    const uint8_t* s[3] = {s0, s1, s2};
    int accv = 1 << (PRECISION_BITS - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int acch = (1 << (PRECISION_BITS - 1)) + (int)s[j][h.c[0]] * h.t[0] + (int)s[j][h.c[1]] * h.t[1] + (int)s[j][h.c[2]] * h.t[2];
        accv += clip8(acch) * tv3[j];
    }
    return clip8(accv);
}

// ---- the band staging of roi_turn_resize3_kernel and roi_fit_resize3_kernel: one block per BAND_RPB consecutive output rows of
// one image, everything the block reads brought to LDS before one barrier.
// The block's output rows draw on a band of at most 7 * ht / n + 3 <= 10 consecutive rows of T = transpose^bit2(src) (n = the
// output height; flipped or not, the band is contiguous).  LDS holds that band as strip[band row][column of T]:
//   * unturned, a band row is a source row: coalesced byte loads, each source row once (roi_resize3_kernel fetches a row once per tap);
//   * turned, the band is a strip of `nrun` source COLUMNS: from every source row one contiguous run of nrun bytes.  Consecutive
//     lanes take consecutive bytes of a run, then the next source row's run, so a wave's load touches 64 / nrun source rows
//     (one transaction each) instead of 64, and no byte is fetched per tap.  The transposition happens on the way into LDS:
//     the lanes of one run write one byte into each of nrun strip rows, and the pitch BAND_PITCH = 324 bytes = 81 words (81 mod
//     32 = 17, odd) puts those on nrun different banks; the horizontal pass then reads along a strip row for turned and unturned
//     ROIs alike (neighbouring lanes, neighbouring bytes).
constexpr int BAND_RPB = 8, BAND_ROWS = 12, BAND_PITCH = 324;

struct Band3 {
    int tvv[BAND_RPB][3], kk[BAND_RPB][3];   // per output row of the block: its vertical taps and the strip rows they apply to
    Tap3 h;                                   // the thread's columns, clamped to the staged width
};

// src / stride: the ROI and its row pitch in bytes; (ht, wt): the dims of the image the resize sees; th: field 0 of the thread's
// horizontal table entry, tv: the image's vertical table; the block's output rows are table rows ytab0 .. ytab0 + BAND_RPB - 1,
// of which [ylo, yhi] exist (block-uniform; the others are given yhi's or ylo's entries and are not to be stored from them).
// Band rows are clamped to the nrun staged ones and columns to the min(wt, 320) staged ones, so stale maxima cannot leave the strip
// or the ROI.  The caller's barrier follows.
__device__ __forceinline__ Band3 band3_stage(uint8_t (*strip)[BAND_PITCH], const uint8_t* src, int stride, int ht, int wt, bool vflip,
                                             bool hflip, bool turned, const int32_t* th, const int32_t* tv, int TS, int ytab0, int ylo,
                                             int yhi) {
    const int wl = wt < 320 ? wt : 320;
    // the band: rows rlo .. rhi of V = rows tlo .. tlo + nrun - 1 of T   (block-uniform)
    const int rlo = tv[ylo], rhi = tv[yhi] + tv[TS + yhi] - 1;
    int tlo = vflip ? ht - 1 - rhi : rlo;
    tlo = tlo < 0 ? 0 : (tlo >= ht ? ht - 1 : tlo);
    int nrun = rhi - rlo + 1;
    nrun = nrun < 1 ? 1 : (nrun > BAND_ROWS ? BAND_ROWS : nrun);
    if (nrun > ht - tlo) nrun = ht - tlo;
    if (turned) {
        // T[tlo + k][c] = src[c][tlo + k]: source row c < wl <= h, columns tlo .. tlo + nrun - 1 < ht = w
        for (int idx = (int)threadIdx.x; idx < wl * nrun; idx += (int)blockDim.x) {
            const int c = idx / nrun, k = idx - c * nrun;
            strip[k][c] = src[(size_t)c * stride + tlo + k];
        }
    } else {
        // T[tlo + k][c] = src[tlo + k][c]: source rows tlo .. tlo + nrun - 1 < ht = h, columns c < wl <= w
        for (int k = 0; k < nrun; ++k)
            for (int c = (int)threadIdx.x; c < wl; c += (int)blockDim.x) strip[k][c] = src[(size_t)(tlo + k) * stride + c];
    }
    Band3 b;
#pragma unroll
    for (int r = 0; r < BAND_RPB; ++r) {
        int yy = ytab0 + r;                                            // block-uniform
        yy = yy < ylo ? ylo : (yy > yhi ? yhi : yy);
        const int ymin = tv[yy], yn = tv[TS + yy];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            b.tvv[r][j] = tv[(2 + j) * TS + yy];
            int row = ymin + (j < yn ? j : yn - 1);
            if (vflip) row = ht - 1 - row;
            row -= tlo;
            b.kk[r][j] = row < 0 ? 0 : (row >= nrun ? nrun - 1 : row);
        }
    }
    b.h = tap3_load(th, TS, hflip, wt);
    tap3_clamp(b.h, wl);
    return b;
}

// output row r of the block from the staged band
__device__ __forceinline__ int band3_row(const uint8_t (*strip)[BAND_PITCH], const Band3& b, int r) {
    return three_tap(strip[b.kk[r][0]], strip[b.kk[r][1]], strip[b.kk[r][2]], b.tvv[r], b.h);
}

}  // namespace
