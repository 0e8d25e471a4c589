// Aspect-preserving ROI preprocessing (TRAIN --pad): ifcbk_roi_preprocess_fit.  The image the resize sees,
//     V = hflip^bit1( vflip^bit0( transpose^bit2( src ) ) )        (ht x wt; roi_turn.hip has the index maths)
// is resized to the inner size (nh, nw) of PIL.ImageOps.contain with the Pillow-exact two-pass arithmetic of roi.hip (22-bit taps,
// clip8 between the passes, Pillow's pass-order rule on (ht, wt, nh)), pasted at (oy, ox) = rint((S - n) / 2) into an S x S plane of
// FILL -- PIL.ImageOps.pad(img, (S, S), BILINEAR, color = FILL, centering = (0.5, 0.5)) -- and goes through the same float stage
// and stores as the squash path.  FILL is a level 0..255 or, per ROI and channel, the rounded mean of the source ROI's border
// pixels.  roi_fit_dims.h holds the size, placement, tap-bound and rounding arithmetic (shared with a host-only check program).
//
// Three kernels:
//   roi_fit_setup_kernel    one block per image: dims and placement, the border fill (a block-wide integer reduction over the
//                           2h + 2w - 4 border bytes per channel) and the two tap tables for output sizes nw / nh
//   roi_fit_resize3_kernel  grey ROIs no larger than the output (three taps per axis), S <= 320: the shape of roi_turn_resize3_kernel
//   roi_fit_resize_kernel   everything else, one block per (image, output row): LDS-staged rows for grey ROIs, global loads otherwise
// Output rows outside [oy, oy + nh) neither stage nor read source pixels.
#include "common.h"
#include "roi_fit_dims.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int FIT_META = 16;       // int32 words per image in front of the tap tables:
enum { M_NH = 0, M_NW, M_OY, M_OX, M_FILL /* 3 */, M_H = 7, M_W, M_STRIDE };

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Table layout [image][axis][field][S] as in roi.hip (axis 0 = horizontal, field 0 = first input index, 1 = tap count, 2.. = taps);
// axis 0 holds nw entries for input size wt, axis 1 nh entries for input size ht.  A ROI whose dims exceed the caller's maxima is
// cut to them (its top-left max_h x max_w part is resized), so the tap count stays within kmax by ifcbk_fit_kmax's derivation
// and no window is ever truncated.
__global__ __launch_bounds__(256) void roi_fit_setup_kernel(const uint8_t* pixels, const int64_t* offs, const int32_t* hs, const int32_t* ws,
                                                            const uint8_t* codes, int codemask, int max_h, int max_w, int S, int cin, int kmax,
                                                            int fill, int32_t* meta, int32_t* tab) {
#pragma clang fp contract(off)
    const int img = blockIdx.x;
    const int tid = threadIdx.x;
    const int stride = ws[img] > 0 ? ws[img] : 1;
    int h = hs[img] > 0 ? hs[img] : 1, w = stride;
    if (h > max_h) h = max_h;
    if (w > max_w) w = max_w;
    const bool turned = codes && (codes[img] & codemask & 4);
    const int ht = turned ? w : h, wt = turned ? h : w;
    const ifcbk_fit_dims fd = ifcbk_fit_dims_for(ht, wt, S);

    // ---- border sums (the border set is invariant under flips and transposes: taken on the source)
    unsigned sum[3] = {0u, 0u, 0u};
    const int64_t nb = ifcbk_fit_border_count(h, w);
    if (fill < 0) {
        const uint8_t* src = pixels + offs[img];
        for (int64_t b = tid; b < nb; b += blockDim.x) {
            int r, c;
            ifcbk_fit_border_at(h, w, b, &r, &c);
            const uint8_t* p = src + ((size_t)r * stride + c) * cin;
            sum[0] += p[0];
            if (cin == 3) { sum[1] += p[1]; sum[2] += p[2]; }
        }
    }

    // ---- tap tables: roi_coeffs_kernel's arithmetic with a per-axis output size
    for (int i = tid; i < 2 * S; i += blockDim.x) {
        const int axis = i >= S;
        const int xx = axis ? i - S : i;
        const int inSize = axis ? ht : wt, outSize = axis ? fd.nh : fd.nw;
        if (xx >= outSize) continue;
        int32_t* row = tab + ((size_t)(img * 2 + axis) * (2 + kmax)) * S + xx;
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
        xmax -= xmin;                                     // <= kmax (ifcbk_fit_kmax)
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = ((double)(x + xmin) - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            double wgt = a < 1.0 ? 1.0 - a : 0.0;
            ww += wgt;
        }
        for (int x = 0; x < kmax; ++x) {
            int kq = 0;
            if (x < xmax) {
                double a = ((double)(x + xmin) - center + 0.5) * ss;
                if (a < 0.0) a = -a;
                double wgt = a < 1.0 ? 1.0 - a : 0.0;
                if (ww != 0.0) wgt = wgt / ww;
                kq = wgt < 0.0 ? (int)(-0.5 + wgt * (double)(1 << PRECISION_BITS)) : (int)(0.5 + wgt * (double)(1 << PRECISION_BITS));
            }
            row[(size_t)(2 + x) * S] = kq;
        }
        row[0] = xmin;
        row[S] = xmax;
    }

    // ---- block reduction of the border sums: wave shuffles, then the four waves' partials through LDS
    __shared__ unsigned part[4][3];
    if (fill < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            for (int off = 32; off > 0; off >>= 1) sum[c] += __shfl_down(sum[c], off, 64);
        if ((tid & 63) == 0)
            for (int c = 0; c < 3; ++c) part[tid >> 6][c] = sum[c];
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* m = meta + (size_t)img * FIT_META;
        m[M_NH] = fd.nh; m[M_NW] = fd.nw; m[M_OY] = fd.oy; m[M_OX] = fd.ox;
        for (int c = 0; c < 3; ++c) {
            int f = fill;
            if (fill < 0) {
                const int cc = cin == 3 ? c : 0;
                const uint64_t s = (uint64_t)part[0][cc] + part[1][cc] + part[2][cc] + part[3][cc];
                f = ifcbk_fit_fill(s, (uint64_t)nb);
            }
            m[M_FILL + c] = f;
        }
        m[M_H] = h; m[M_W] = w; m[M_STRIDE] = stride;
    }
}

struct FitArgs {
    const uint8_t* pixels;
    const int64_t* offs;
    const uint8_t* codes;
    const int32_t* meta;
    const int32_t* tab;
    void* out;
    int f32;
    uint8_t* out_u8;
    int n_img, S, cin, cout, kmax, codemask;
    float mean[3], std[3], tsc[3], tsh[3];
};

// the float stage and the stores of roi.hip's kernels, for output pixel i (res[c]: the u8 level of channel c)
__device__ __forceinline__ void store_pixel(const FitArgs& a, int64_t i, const int* res) {
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

// Every batch the grey three-tap kernel below does not take: one block per (image, output row) like roi_resize_kernel.
// A row outside the inner rectangle is FILL and leaves before any table or pixel is read.  A grey ROI whose row window holds at
// most FLR rows of at most FLW pixels gets those rows of V staged in LDS (for a turned ROI a row of V is a source column);
// wider ROIs, longer windows and RGB read global memory per tap.  Both run the vertical pass first where Pillow does.
constexpr int FLR = 5, FLW = 640;
__global__ __launch_bounds__(320) void roi_fit_resize_kernel(FitArgs a) {
    const int img = (int)(blockIdx.x / (unsigned)a.S);
    const int y = (int)(blockIdx.x - (unsigned)img * (unsigned)a.S);
    const int x0 = blockIdx.y * blockDim.x + threadIdx.x;
    const bool live = x0 < a.S;                          // (no early return: every thread reaches the barrier of the staged path)
    const int x = live ? x0 : a.S - 1;
    const int64_t i = ((int64_t)img * a.S + y) * a.S + x;
    const int32_t* m = a.meta + (size_t)img * FIT_META;
    const int nh = m[M_NH], nw = m[M_NW], oy = m[M_OY], ox = m[M_OX];
    int res[3] = {m[M_FILL], m[M_FILL + 1], m[M_FILL + 2]};
    const int yy = y - oy;
    if (yy < 0 || yy >= nh) {                            // block-uniform: a fill row
        if (live) store_pixel(a, i, res);
        return;
    }
    const int h = m[M_H], w = m[M_W], stride = m[M_STRIDE];
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.codes ? a.codes[img] & a.codemask : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;  // the dims of the image the resize sees
    const int TS = a.S;                                  // field stride of the tap table
    const bool inside = x - ox >= 0 && x - ox < nw;
    const int xx = inside ? x - ox : 0;
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * (2 + a.kmax)) * a.S + xx;
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * (2 + a.kmax)) * a.S + yy;
    const int xmin = th[0], xn = th[TS], ymin = tv[0], yn = tv[TS];
    // byte offset of V[row][col] (channel 0) after the flips
    auto at = [&](int row, int col) -> size_t {
        if (vflip) row = ht - 1 - row;
        if (hflip) col = wt - 1 - col;
        return turned ? (size_t)col * stride + row : (size_t)row * stride + col;
    };
    __shared__ uint8_t srow[FLR][FLW];
    const bool staged = a.cin == 1 && yn <= FLR && wt <= FLW;                      // block-uniform
    const bool vfirst = (int64_t)ht > 100 * (int64_t)wt && nh < ht;                // block-uniform (per image), on the seen dims
    if (staged) {
        // columns unflipped in LDS (the horizontal flip is applied to the tap's column below, as in roi.hip)
        for (int c = threadIdx.x; c < wt; c += blockDim.x)
            for (int j = 0; j < yn; ++j) {
                int row = ymin + j;
                if (vflip) row = ht - 1 - row;
                srow[j][c] = src[turned ? (size_t)c * stride + row : (size_t)row * stride + c];
            }
        __syncthreads();
        if (inside) {
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
            res[1] = res[2] = res[0];
        }
    } else if (inside) {
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
        if (a.cin == 1) res[1] = res[2] = res[0];
    }
    if (!live) return;
    store_pixel(a, i, res);
}

// The training case -- grey ROIs no larger than the output (kmax == 3: both scales <= 1), S <= 320 -- in the shape of
// roi_turn_resize3_kernel: one block per FRPB consecutive output rows of one image, the image's scalars and a thread's horizontal taps
// fetched once per block, everything the block reads brought to LDS before one barrier.  The inner rows among the block's FRPB
// draw on a band of at most 7 * ht / nh + 3 <= 10 consecutive rows of T = transpose^bit2(src), staged as strip[band row][column
// of T]: coalesced rows unturned, runs of source columns transposed on the way into LDS when turned (pitch FLP = 324 bytes = 81
// words, odd, as in roi_turn.hip).  A block whose rows are all fill stages nothing and reads no source byte.
constexpr int FRPB = 8, FBAND = 12, FLP = 324;
__global__ __launch_bounds__(320) void roi_fit_resize3_kernel(FitArgs a) {
    const unsigned nrb = (unsigned)(a.S + FRPB - 1) / FRPB;
    const int img = (int)(blockIdx.x / nrb);
    const int y0 = (int)(blockIdx.x - (unsigned)img * nrb) * FRPB;
    const bool live = (int)threadIdx.x < a.S;
    const int x = live ? (int)threadIdx.x : a.S - 1;
    const int32_t* m = a.meta + (size_t)img * FIT_META;
    const int nh = m[M_NH], nw = m[M_NW], oy = m[M_OY], ox = m[M_OX], fill = m[M_FILL];
    const int ylast = y0 + FRPB - 1 < a.S ? y0 + FRPB - 1 : a.S - 1;
    const int ylo = y0 - oy > 0 ? y0 - oy : 0, yhi = ylast - oy < nh - 1 ? ylast - oy : nh - 1;    // the block's inner rows
    if (ylo > yhi) {                                     // block-uniform: fill rows only
        if (!live) return;
        const int res[3] = {fill, fill, fill};
        for (int y = y0; y <= ylast; ++y) store_pixel(a, ((int64_t)img * a.S + y) * a.S + x, res);
        return;
    }
    const int h = m[M_H], w = m[M_W], stride = m[M_STRIDE];
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.codes ? a.codes[img] & a.codemask : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;
    // the setup kernel cut h and w to the caller's maxima, which are <= S <= 320 here; the clamps below keep a table that breaks
    // that promise inside the staged strip all the same
    const int wl = wt < 320 ? wt : 320;
    const int TS = a.S;
    const bool inside = x - ox >= 0 && x - ox < nw;
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * (2 + a.kmax)) * a.S + (inside ? x - ox : 0);
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * (2 + a.kmax)) * a.S;
    __shared__ uint8_t strip[FBAND][FLP];
    // the band: rows rlo .. rhi of V = rows tlo .. tlo + nrun - 1 of T   (block-uniform)
    const int rlo = tv[ylo], rhi = tv[yhi] + tv[TS + yhi] - 1;
    int tlo = vflip ? ht - 1 - rhi : rlo;
    tlo = tlo < 0 ? 0 : (tlo >= ht ? ht - 1 : tlo);
    int nrun = rhi - rlo + 1;
    nrun = nrun < 1 ? 1 : (nrun > FBAND ? FBAND : nrun);
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
    int tvv[FRPB][3], kk[FRPB][3];
#pragma unroll
    for (int r = 0; r < FRPB; ++r) {
        int yy = y0 + r - oy;                                          // block-uniform
        yy = yy < ylo ? ylo : (yy > yhi ? yhi : yy);
        const int ymin = tv[yy], yn = tv[TS + yy];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            tvv[r][j] = tv[(2 + j) * TS + yy];
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
    for (int r = 0; r < FRPB; ++r) {
        const int y = y0 + r;
        if (y >= a.S) break;
        int v = fill;
        if (inside && y - oy >= 0 && y - oy < nh) {
            int accv = 1 << (PRECISION_BITS - 1);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint8_t* s = strip[kk[r][j]];
                const int acch = (1 << (PRECISION_BITS - 1)) + (int)s[c0] * t0 + (int)s[c1] * t1 + (int)s[c2] * t2;
                accv += clip8(acch) * tvv[r][j];
            }
            v = clip8(accv);
        }
        const int res[3] = {v, v, v};
        store_pixel(a, ((int64_t)img * a.S + y) * a.S + x, res);
    }
}

}  // namespace

extern "C" size_t ifcbk_roi_preprocess_fit_workspace(const ifcbk_roi_desc* d, int max_h, int max_w) {
    if (!d || d->n_img <= 0 || d->S < 1 || max_h < 1 || max_w < 1) return 0;
    const int kmax = ifcbk_fit_kmax(max_h, max_w, d->S);
    return (size_t)d->n_img * FIT_META * sizeof(int32_t) + (size_t)d->n_img * 2 * d->S * (2 + kmax) * sizeof(int32_t);
}

extern "C" int ifcbk_roi_preprocess_fit(ifcbk_ctx* ctx, const ifcbk_roi_desc* d, const uint8_t* pixels, const int64_t* offs,
                                        const int32_t* hs, const int32_t* ws, const uint8_t* codes, int max_h, int max_w, int fill,
                                        void* out, uint8_t* out_u8, void* stream) {
    if (!d || d->n_img <= 0) return IFCBK_OK;   // empty bin: nothing to do
    if ((d->dtype != IFCBK_BF16 && d->dtype != IFCBK_F32) || (d->in_channels != 1 && d->in_channels != 3) || d->out_channels % 8 ||
        d->out_channels < 8 || d->S < 1)
        IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_preprocess_fit: bad desc");
    if (max_h < 1 || max_w < 1) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_preprocess_fit: max dims");
    if (fill < -1 || fill > 255) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_preprocess_fit: fill %d is neither a level 0..255 nor -1 (border)", fill);
    if (!out && !out_u8) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_preprocess_fit: out and out_u8 are both NULL");
    if (d->flip_bits_valid && !codes) IFCBK_FAIL(ctx, IFCBK_EINVAL, "roi_preprocess_fit: flip_bits_valid without codes");
    size_t need = ifcbk_roi_preprocess_fit_workspace(d, max_h, max_w);
    if (need > ctx->ws_bytes) IFCBK_FAIL(ctx, IFCBK_ENOMEM, "roi_preprocess_fit: workspace %zu > reserved %zu", need, ctx->ws_bytes);
    const int kmax = ifcbk_fit_kmax(max_h, max_w, d->S);
    hipStream_t st = (hipStream_t)stream;
    int32_t* meta = (int32_t*)ctx->ws;
    int32_t* tab = meta + (size_t)d->n_img * FIT_META;
    const int codemask = d->flip_bits_valid == 2 ? 7 : 3;          // bit 2 counts under flip_bits_valid == 2 only
    const uint8_t* cd = d->flip_bits_valid ? codes : nullptr;
    hipLaunchKernelGGL(roi_fit_setup_kernel, dim3((unsigned)d->n_img), dim3(256), 0, st, pixels, offs, hs, ws, cd, codemask, max_h, max_w, d->S,
                       d->in_channels, kmax, fill, meta, tab);
    IFCBK_LAUNCH_CHECK(ctx, "roi_fit_setup");
    FitArgs a;
    a.pixels = pixels; a.offs = offs; a.codes = cd; a.meta = meta; a.tab = tab;
    a.out = out; a.f32 = d->dtype == IFCBK_F32; a.out_u8 = out_u8;
    a.n_img = d->n_img; a.S = d->S; a.cin = d->in_channels; a.cout = d->out_channels; a.kmax = kmax; a.codemask = codemask;
    for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.std[i] = d->std[i]; a.tsc[i] = d->tin_scale[i]; a.tsh[i] = d->tin_shift[i]; }
    const int fbx = d->S <= 64 ? 64 : d->S <= 128 ? 128 : d->S <= 192 ? 192 : d->S <= 256 ? 256 : 320;     // threads per output row
    if (d->in_channels == 1 && kmax == 3 && d->S <= 320)     // (kmax == 3: no ROI is larger than the output, so wt <= S <= 320)
        hipLaunchKernelGGL(roi_fit_resize3_kernel, dim3((unsigned)(d->n_img * cdiv(d->S, FRPB))), dim3(fbx), 0, st, a);
    else
        hipLaunchKernelGGL(roi_fit_resize_kernel, dim3((unsigned)(d->n_img * d->S), (unsigned)cdiv(d->S, fbx)), dim3(fbx), 0, st, a);
    IFCBK_LAUNCH_CHECK(ctx, "roi_fit_resize");
    return 0;
}
