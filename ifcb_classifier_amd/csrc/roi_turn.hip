// ROI preprocessing with quarter turns (TRAIN --rot90): the kernels behind ifcbk_roi_preprocess when flip_bits_valid == 2.
// The code byte gains bit 2 = transpose; the image the resize sees is
//     V = hflip^bit1( vflip^bit0( T ) ),   T = transpose^bit2( src ),   transpose(src)[r][c] = src[c][r]
// so V is ht x wt with (ht, wt) = (w, h) for a turned ROI and (h, w) otherwise: the horizontal tap table is built from wt, the
// vertical one from ht, and Pillow's pass-order rule is evaluated on (ht, wt).  The arithmetic is roi_resample.h's (22-bit taps,
// clip8 between the passes, the float stage and stores), as for roi.hip; only where a pixel of V lives in memory differs:
//     V[r][c] = T[r'][c'],  r' = vflip ? ht - 1 - r : r,  c' = hflip ? wt - 1 - c : c,  T[r'][c'] = turned ? src[c' * w + r'] : src[r' * w + c']
// One kernel set serves every code 0..7 of a batch: whether a run takes these kernels depends on the flag, never on the draw.
#include "roi_resample.h"

namespace {

// roi_coeffs_kernel of roi.hip with the two axes' input sizes swapped for a turned ROI; same table layout
__global__ void roi_turn_coeffs_kernel(const int32_t* hs, const int32_t* ws, const uint8_t* flips, int n_img, int S, int kmax, int32_t* tab) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * 2 * S) return;
    int xx = i % S;
    int axis = (i / S) & 1;
    int img = i / (2 * S);
    const bool turned = flips && (flips[img] & 4);
    int inSize = (axis == 0) != turned ? ws[img] : hs[img];
    int32_t* row = tab + ((size_t)(img * 2 + axis) * (2 + kmax)) * S + xx;
    roi_taps(inSize, S, xx, kmax, row, S);
}

// Every batch the grey training kernel below does not take: one block per (image, output row) like roi_resize_kernel.
// Grey ROIs of up to TLR taps per axis whose turned width fits TLW get their yn rows of V staged in LDS (for a turned ROI a row
// of V is a source column: thread c fetches the yn neighbouring bytes of source row c); wider, larger and RGB ROIs read global memory
// per tap.  Both branches run the vertical pass first where Pillow does, judged on the turned dims.
constexpr int TLR = 5, TLW = 640;
__global__ __launch_bounds__(320) void roi_turn_resize_kernel(RoiArgs a) {
    const int img = (int)(blockIdx.x / (unsigned)a.S);
    const int y = (int)(blockIdx.x - (unsigned)img * (unsigned)a.S);
    const int x0 = blockIdx.y * blockDim.x + threadIdx.x;
    const bool live = x0 < a.S;                          // (no early return: every thread reaches the barrier of the staged path)
    const int x = live ? x0 : a.S - 1;
    const int64_t i = ((int64_t)img * a.S + y) * a.S + x;
    const int h = a.hs[img], w = a.ws[img];
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.flips ? a.flips[img] : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;  // the dims of the image the resize sees
    const int TS = a.S;                                  // field stride of the tap table
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * (2 + a.kmax)) * a.S + x;
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * (2 + a.kmax)) * a.S + y;
    const int xmin = th[0], xn = th[TS], ymin = tv[0], yn = tv[TS];
    // byte offset of V[row][col] (channel 0) after the flips
    auto at = [&](int row, int col) -> size_t {
        if (vflip) row = ht - 1 - row;
        if (hflip) col = wt - 1 - col;
        return turned ? (size_t)col * w + row : (size_t)row * w + col;
    };
    int res[3];
    __shared__ uint8_t srow[TLR][TLW];
    const bool staged = a.cin == 1 && a.kmax <= TLR && wt <= TLW;                  // block-uniform
    const bool vfirst = ht > 100 * wt && ht > a.S;                                 // block-uniform (per image), on the turned dims
    if (staged) {
        // columns unflipped in LDS (the horizontal flip is applied to the tap's column below, as in roi.hip)
        for (int c = threadIdx.x; c < wt; c += blockDim.x)
            for (int j = 0; j < yn; ++j) {
                int row = ymin + j;
                if (vflip) row = ht - 1 - row;
                srow[j][c] = src[turned ? (size_t)c * w + row : (size_t)row * w + c];
            }
        __syncthreads();
        res[0] = two_pass([&](int j, int k) { return (int)srow[j][hflip ? wt - 1 - (xmin + k) : xmin + k]; }, th, xn, tv, yn, TS, vfirst);
    } else
    for (int c = 0; c < a.cin; ++c) {
        res[c] = two_pass([&](int j, int k) { return (int)src[at(ymin + j, xmin + k) * a.cin + c]; }, th, xn, tv, yn, TS, vfirst);
    }
    if (!live) return;
    if (a.cin == 1) res[1] = res[2] = res[0];
    ROI_STORE_PIXEL(a, i, a.cin, res[c]);
}

// The training case -- grey ROIs no larger than the output (three taps per axis), S <= 320 -- in the shape of roi_resize3_kernel:
// one block per BAND_RPB consecutive output rows of one image, the image's scalars and a thread's horizontal taps fetched once per
// block, the band of T = transpose^bit2(src) those rows draw on staged once (band3_stage of roi_resample.h, which also absorbs
// stale maxima): all of the block's rows exist in the table, and a row of T is w bytes from the next.
__global__ __launch_bounds__(320) void roi_turn_resize3_kernel(RoiArgs a) {
    const unsigned nrb = (unsigned)(a.S + BAND_RPB - 1) / BAND_RPB;
    const int img = (int)(blockIdx.x / nrb);
    const int y0 = (int)(blockIdx.x - (unsigned)img * nrb) * BAND_RPB;
    const bool live = (int)threadIdx.x < a.S;
    const int x = live ? (int)threadIdx.x : a.S - 1;
    const int h = a.hs[img] > 0 ? a.hs[img] : 1, w = a.ws[img] > 0 ? a.ws[img] : 1;
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.flips ? a.flips[img] : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;
    const int TS = a.S;
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * 5) * a.S + x;
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * 5) * a.S;
    __shared__ uint8_t strip[BAND_ROWS][BAND_PITCH];
    const int ylast = y0 + BAND_RPB - 1 < a.S ? y0 + BAND_RPB - 1 : a.S - 1;
    const Band3 b = band3_stage(strip, src, w, ht, wt, vflip, hflip, turned, th, tv, TS, y0, y0, ylast);
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int r = 0; r < BAND_RPB; ++r) {
        if (y0 + r >= a.S) break;
        const int v = band3_row(strip, b, r);
        const int res[3] = {v, v, v};
        ROI_STORE_PIXEL(a, ((int64_t)img * a.S + (y0 + r)) * a.S + x, a.cin, res[c]);
    }
}

}  // namespace

// called by ifcbk_roi_preprocess (roi.hip) for flip_bits_valid == 2, after it has checked the descriptor and the workspace
int ifcbk_roi_turn_launch(ifcbk_ctx* ctx, const ifcbk_roi_desc* d, const uint8_t* pixels, const int64_t* offs, const int32_t* hs,
                          const int32_t* ws, const uint8_t* flips, int kmax, void* out, uint8_t* out_u8, hipStream_t st) {
    int nco = d->n_img * 2 * d->S;
    hipLaunchKernelGGL(roi_turn_coeffs_kernel, dim3(cdiv(nco, 256)), dim3(256), 0, st, hs, ws, flips, d->n_img, d->S, kmax, (int32_t*)ctx->ws);
    IFCBK_LAUNCH_CHECK(ctx, "roi_turn_coeffs");
    RoiArgs a;
    a.pixels = pixels; a.offs = offs; a.hs = hs; a.ws = ws; a.flips = flips;
    a.tab = (const int32_t*)ctx->ws; a.out = out; a.out_u8 = out_u8;
    roi_args_desc(a, d, kmax);
    const int tbx = roi_row_threads(d->S);
    if (d->in_channels == 1 && kmax == 3 && d->S <= 320)     // (kmax == 3: no ROI is larger than the output, so wt <= S <= 320)
        hipLaunchKernelGGL(roi_turn_resize3_kernel, dim3((unsigned)(d->n_img * cdiv(d->S, BAND_RPB))), dim3(tbx), 0, st, a);
    else
        hipLaunchKernelGGL(roi_turn_resize_kernel, dim3((unsigned)(d->n_img * d->S), (unsigned)cdiv(d->S, tbx)), dim3(tbx), 0, st, a);
    IFCBK_LAUNCH_CHECK(ctx, "roi_turn_resize");
    return 0;
}
