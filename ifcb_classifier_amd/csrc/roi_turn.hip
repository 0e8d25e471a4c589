// ROI preprocessing with quarter turns (TRAIN --rot90): the kernels behind ifcbk_roi_preprocess when flip_bits_valid == 2.
// The code byte gains bit 2 = transpose; the image the resize sees is
//     V = hflip^bit1( vflip^bit0( T ) ),   T = transpose^bit2( src ),   transpose(src)[r][c] = src[c][r]
// so V is ht x wt with (ht, wt) = (w, h) for a turned ROI and (h, w) otherwise: the horizontal tap table is built from wt, the
// vertical one from ht, and Pillow's pass-order rule is evaluated on (ht, wt).  The arithmetic is that of roi.hip (22-bit taps,
// clip8 between the passes, the same float stage and stores); only where a pixel of V lives in memory differs:
//     V[r][c] = T[r'][c'],  r' = vflip ? ht - 1 - r : r,  c' = hflip ? wt - 1 - c : c,  T[r'][c'] = turned ? src[c' * w + r'] : src[r' * w + c']
// One kernel set serves every code 0..7 of a batch: whether a run takes these kernels depends on the flag, never on the draw.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// roi_coeffs_kernel of roi.hip with the two axes' input sizes swapped for a turned ROI; same table layout
// [image][axis][field][S] (axis 0 = horizontal, field 0 = first input index, 1 = tap count, 2.. = taps)
__global__ void roi_turn_coeffs_kernel(const int32_t* hs, const int32_t* ws, const uint8_t* flips, int n_img, int S, int kmax, int32_t* tab) {
#pragma clang fp contract(off)
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img * 2 * S) return;
    int xx = i % S;
    int axis = (i / S) & 1;
    int img = i / (2 * S);
    const bool turned = flips && (flips[img] & 4);
    int inSize = (axis == 0) != turned ? ws[img] : hs[img];
    int32_t* row = tab + ((size_t)(img * 2 + axis) * (2 + kmax)) * S + xx;
    const int RS_ = S;
    double scale = (double)((float)inSize - 0.0f) / (double)S;
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
    if (xmax > kmax) xmax = kmax;                     // cannot happen when kmax is sized from max dims
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
        row[(size_t)(2 + x) * RS_] = kq;
    }
    row[0] = xmin;
    row[RS_] = xmax;
}

struct TurnArgs {
    const uint8_t* pixels;
    const int64_t* offs;
    const int32_t* hs;
    const int32_t* ws;
    const uint8_t* flips;
    const int32_t* tab;
    void* out;
    int f32;
    uint8_t* out_u8;
    int n_img, S, cin, cout, kmax;
    float mean[3], std[3], tsc[3], tsh[3];
};

// the float stage and the stores of roi.hip's kernels, for output pixel i (res[c]: the resized u8 level of channel c)
__device__ __forceinline__ void store_pixel(const TurnArgs& a, int64_t i, const int* res) {
    if (a.out_u8)
        for (int c = 0; c < a.cin; ++c) a.out_u8[i * a.cin + c] = (uint8_t)res[c];
    if (a.out) {
        for (int c0 = 0; c0 < a.cout; c0 += 8) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int c = c0 + j;
                float v = 0.f;
                if (c < 3) {
                    v = (float)res[c] / 255.0f;
                    v = (v - a.mean[c]) / a.std[c];
                    v = v * a.tsc[c] + a.tsh[c];
                }
                f[j] = v;
            }
            if (a.f32) {
                float* o = (float*)a.out + i * a.cout + c0;
                *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
                *reinterpret_cast<float4*>(o + 4) = make_float4(f[4], f[5], f[6], f[7]);
            } else {
                *reinterpret_cast<uint4*>((bf16_t*)a.out + i * a.cout + c0) = pack8(f);
            }
        }
    }
}

// Every batch the grey training kernel below does not take: one block per (image, output row) like roi_resize_kernel.
// Grey ROIs of up to TLR taps per axis whose turned width fits TLW get their yn rows of V staged in LDS (for a turned ROI a row
// of V is a source column: thread c fetches the yn neighbouring bytes of source row c); wider, larger and RGB ROIs read global memory
// per tap.  Both branches run the vertical pass first where Pillow does, judged on the turned dims.
constexpr int TLR = 5, TLW = 640;
__global__ __launch_bounds__(320) void roi_turn_resize_kernel(TurnArgs a) {
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
        if (vfirst) {
            int acch = 1 << (PRECISION_BITS - 1);
            for (int k = 0; k < xn; ++k) {
                int col = xmin + k;
                if (hflip) col = wt - 1 - col;
                int accv = 1 << (PRECISION_BITS - 1);
                for (int j = 0; j < yn; ++j) accv += (int)srow[j][col] * tv[(size_t)(2 + j) * TS];
                acch += clip8(accv) * th[(size_t)(2 + k) * TS];
            }
            res[0] = clip8(acch);
        } else {
            int accv = 1 << (PRECISION_BITS - 1);
            for (int j = 0; j < yn; ++j) {
                int acch = 1 << (PRECISION_BITS - 1);
                for (int k = 0; k < xn; ++k) {
                    int col = xmin + k;
                    if (hflip) col = wt - 1 - col;
                    acch += (int)srow[j][col] * th[(size_t)(2 + k) * TS];
                }
                accv += clip8(acch) * tv[(size_t)(2 + j) * TS];
            }
            res[0] = clip8(accv);
        }
    } else
    for (int c = 0; c < a.cin; ++c) {
        if (vfirst) {
            int acch = 1 << (PRECISION_BITS - 1);
            for (int k = 0; k < xn; ++k) {
                int accv = 1 << (PRECISION_BITS - 1);
                for (int j = 0; j < yn; ++j) accv += (int)src[at(ymin + j, xmin + k) * a.cin + c] * tv[(size_t)(2 + j) * TS];
                acch += clip8(accv) * th[(size_t)(2 + k) * TS];
            }
            res[c] = clip8(acch);
            continue;
        }
        int accv = 1 << (PRECISION_BITS - 1);
        for (int j = 0; j < yn; ++j) {
            int acch = 1 << (PRECISION_BITS - 1);
            for (int k = 0; k < xn; ++k) acch += (int)src[at(ymin + j, xmin + k) * a.cin + c] * th[(size_t)(2 + k) * TS];
            accv += clip8(acch) * tv[(size_t)(2 + j) * TS];
        }
        res[c] = clip8(accv);
    }
    if (!live) return;
    if (a.cin == 1) res[1] = res[2] = res[0];
    store_pixel(a, i, res);
}

// The training case -- grey ROIs no larger than the output (three taps per axis), S <= 320 -- in the shape of roi_resize3_kernel:
// one block per TRPB consecutive output rows of one image, the image's scalars and a thread's horizontal taps fetched once per
// block, everything the block reads brought to LDS before one barrier.
// The TRPB output rows draw on a band of at most 7 * ht / S + 3 <= 10 consecutive rows of T (flipped or not, the band is
// contiguous).  LDS holds that band as strip[band row][column of T]:
//   * unturned, a band row is a source row: coalesced byte loads, each source row once (roi_resize3_kernel fetches a row once per tap);
//   * turned, the band is a strip of `nrun` source COLUMNS: from every source row one contiguous run of nrun bytes.  Consecutive
//     lanes take consecutive bytes of a run, then the next source row's run, so a wave's load touches 64 / nrun source rows
//     (one transaction each) instead of 64, and no byte is fetched per tap.  The transposition happens on the way into LDS:
//     the lanes of one run write one byte into each of nrun strip rows, and the pitch TLP = 324 bytes = 81 words (81 mod 32 = 17,
//     odd) puts those on nrun different banks; the horizontal pass then reads along a strip row for turned and unturned
//     ROIs alike (neighbouring lanes, neighbouring bytes).
constexpr int TRPB = 8, TBAND = 12, TLP = 324;
__global__ __launch_bounds__(320) void roi_turn_resize3_kernel(TurnArgs a) {
    const unsigned nrb = (unsigned)(a.S + TRPB - 1) / TRPB;
    const int img = (int)(blockIdx.x / nrb);
    const int y0 = (int)(blockIdx.x - (unsigned)img * nrb) * TRPB;
    const bool live = (int)threadIdx.x < a.S;
    const int x = live ? (int)threadIdx.x : a.S - 1;
    const int h = a.hs[img] > 0 ? a.hs[img] : 1, w = a.ws[img] > 0 ? a.ws[img] : 1;
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.flips ? a.flips[img] : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;
    // this kernel is chosen from the caller's max_h / max_w (kmax == 3: no ROI larger than the output).  A table entry that
    // breaks that promise (stale maxima) must not read unstaged LDS or leave the ROI: band rows are clamped to the nrun staged
    // ones, columns to the wl staged ones -- such a ROI comes out wrong (its coefficient table was sized for three taps), never
    // out of bounds
    const int wl = wt < 320 ? wt : 320;
    const int TS = a.S;
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * 5) * a.S + x;
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * 5) * a.S;
    __shared__ uint8_t strip[TBAND][TLP];
    // the band: rows rlo .. rhi of V = rows tlo .. tlo + nrun - 1 of T   (block-uniform)
    const int ylast = y0 + TRPB - 1 < a.S ? y0 + TRPB - 1 : a.S - 1;
    const int rlo = tv[y0], rhi = tv[ylast] + tv[TS + ylast] - 1;
    int tlo = vflip ? ht - 1 - rhi : rlo;
    tlo = tlo < 0 ? 0 : (tlo >= ht ? ht - 1 : tlo);
    int nrun = rhi - rlo + 1;
    nrun = nrun < 1 ? 1 : (nrun > TBAND ? TBAND : nrun);
    if (nrun > ht - tlo) nrun = ht - tlo;
    if (turned) {
        // T[tlo + k][c] = src[c][tlo + k]: source row c < wl <= h, columns tlo .. tlo + nrun - 1 < ht = w
        for (int idx = (int)threadIdx.x; idx < wl * nrun; idx += (int)blockDim.x) {
            const int c = idx / nrun, k = idx - c * nrun;
            strip[k][c] = src[(size_t)c * w + tlo + k];
        }
    } else {
        // T[tlo + k][c] = src[tlo + k][c]: source rows tlo .. tlo + nrun - 1 < ht = h, columns c < wl <= w
        for (int k = 0; k < nrun; ++k)
            for (int c = (int)threadIdx.x; c < wl; c += (int)blockDim.x) strip[k][c] = src[(size_t)(tlo + k) * w + c];
    }
    int tvv[TRPB][3], kk[TRPB][3];
#pragma unroll
    for (int r = 0; r < TRPB; ++r) {
        const int y = y0 + r < a.S ? y0 + r : a.S - 1;                 // block-uniform
        const int ymin = tv[y], yn = tv[TS + y];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            tvv[r][j] = tv[(2 + j) * TS + y];
            int row = ymin + (j < yn ? j : yn - 1);
            if (vflip) row = ht - 1 - row;
            row -= tlo;
            kk[r][j] = row < 0 ? 0 : (row >= nrun ? nrun - 1 : row);
        }
    }
    const int xmin = th[0], xn = th[TS];
    const int t0 = th[2 * TS], t1 = th[3 * TS], t2 = th[4 * TS];
    int c0 = xmin, c1 = xmin + (xn > 1 ? 1 : 0), c2 = xmin + (xn > 2 ? 2 : xn - 1);
    if (hflip) { c0 = wt - 1 - c0; c1 = wt - 1 - c1; c2 = wt - 1 - c2; }
    c0 = c0 < 0 ? 0 : (c0 >= wl ? wl - 1 : c0);
    c1 = c1 < 0 ? 0 : (c1 >= wl ? wl - 1 : c1);
    c2 = c2 < 0 ? 0 : (c2 >= wl ? wl - 1 : c2);
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int r = 0; r < TRPB; ++r) {
        if (y0 + r >= a.S) break;
        int accv = 1 << (PRECISION_BITS - 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint8_t* s = strip[kk[r][j]];
            const int acch = (1 << (PRECISION_BITS - 1)) + (int)s[c0] * t0 + (int)s[c1] * t1 + (int)s[c2] * t2;
            accv += clip8(acch) * tvv[r][j];
        }
        int res[3];
        res[0] = res[1] = res[2] = clip8(accv);
        store_pixel(a, ((int64_t)img * a.S + (y0 + r)) * a.S + x, res);
    }
}

}  // namespace

// called by ifcbk_roi_preprocess (roi.hip) for flip_bits_valid == 2, after it has checked the descriptor and the workspace
int ifcbk_roi_turn_launch(ifcbk_ctx* ctx, const ifcbk_roi_desc* d, const uint8_t* pixels, const int64_t* offs, const int32_t* hs,
                          const int32_t* ws, const uint8_t* flips, int kmax, void* out, uint8_t* out_u8, hipStream_t st) {
    int nco = d->n_img * 2 * d->S;
    hipLaunchKernelGGL(roi_turn_coeffs_kernel, dim3(cdiv(nco, 256)), dim3(256), 0, st, hs, ws, flips, d->n_img, d->S, kmax, (int32_t*)ctx->ws);
    IFCBK_LAUNCH_CHECK(ctx, "roi_turn_coeffs");
    TurnArgs a;
    a.pixels = pixels; a.offs = offs; a.hs = hs; a.ws = ws; a.flips = flips;
    a.tab = (const int32_t*)ctx->ws; a.out = out; a.f32 = d->dtype == IFCBK_F32; a.out_u8 = out_u8;
    a.n_img = d->n_img; a.S = d->S; a.cin = d->in_channels; a.cout = d->out_channels; a.kmax = kmax;
    for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.std[i] = d->std[i]; a.tsc[i] = d->tin_scale[i]; a.tsh[i] = d->tin_shift[i]; }
    const int tbx = d->S <= 64 ? 64 : d->S <= 128 ? 128 : d->S <= 192 ? 192 : d->S <= 256 ? 256 : 320;     // threads per output row
    if (d->in_channels == 1 && kmax == 3 && d->S <= 320)     // (kmax == 3: no ROI is larger than the output, so wt <= S <= 320)
        hipLaunchKernelGGL(roi_turn_resize3_kernel, dim3((unsigned)(d->n_img * cdiv(d->S, TRPB))), dim3(tbx), 0, st, a);
    else
        hipLaunchKernelGGL(roi_turn_resize_kernel, dim3((unsigned)(d->n_img * d->S), (unsigned)cdiv(d->S, tbx)), dim3(tbx), 0, st, a);
    IFCBK_LAUNCH_CHECK(ctx, "roi_turn_resize");
    return 0;
}
