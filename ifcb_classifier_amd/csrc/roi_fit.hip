// Aspect-preserving ROI preprocessing (TRAIN --pad): ifcbk_roi_preprocess_fit.  The image the resize sees,
//     V = hflip^bit1( vflip^bit0( transpose^bit2( src ) ) )        (ht x wt; roi_turn.hip has the index maths)
// is resized to the inner size (nh, nw) of PIL.ImageOps.contain with the Pillow-exact two-pass arithmetic of roi_resample.h (22-bit taps,
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
#include "roi_resample.h"
#include "roi_fit_dims.h"

namespace {

constexpr int FIT_META = 16;       // int32 words per image in front of the tap tables:
enum { M_NH = 0, M_NW, M_OY, M_OX, M_FILL /* 3 */, M_H = 7, M_W, M_STRIDE };

// Table layout [image][axis][field][S] (roi_resample.h);
// axis 0 holds nw entries for input size wt, axis 1 nh entries for input size ht.  A ROI whose dims exceed the caller's maxima is
// cut to them (its top-left max_h x max_w part is resized), so the tap count stays within kmax by ifcbk_fit_kmax's derivation
// and no window is ever truncated.
__global__ __launch_bounds__(256) void roi_fit_setup_kernel(const uint8_t* pixels, const int64_t* offs, const int32_t* hs, const int32_t* ws,
                                                            const uint8_t* codes, int codemask, int max_h, int max_w, int S, int cin, int kmax,
                                                            int fill, int32_t* meta, int32_t* tab) {
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

    // ---- tap tables, with a per-axis output size
    for (int i = tid; i < 2 * S; i += blockDim.x) {
        const int axis = i >= S;
        const int xx = axis ? i - S : i;
        const int inSize = axis ? ht : wt, outSize = axis ? fd.nh : fd.nw;
        if (xx >= outSize) continue;
        roi_taps(inSize, outSize, xx, kmax, tab + ((size_t)(img * 2 + axis) * (2 + kmax)) * S + xx, S);
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

// RoiArgs with hs / ws unset (the setup kernel's cut dims are in meta) and flips = the codes, of which codemask counts
struct FitArgs : RoiArgs {
    const int32_t* meta;
    int codemask;
};

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
        if (live) ROI_STORE_PIXEL(a, i, a.cin, res[c]);
        return;
    }
    const int h = m[M_H], w = m[M_W], stride = m[M_STRIDE];
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.flips ? a.flips[img] & a.codemask : 0;
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
            res[0] = two_pass([&](int j, int k) { return (int)srow[j][hflip ? wt - 1 - (xmin + k) : xmin + k]; }, th, xn, tv, yn, TS, vfirst);
            res[1] = res[2] = res[0];
        }
    } else if (inside) {
        for (int c = 0; c < a.cin; ++c) {
            res[c] = two_pass([&](int j, int k) { return (int)src[at(ymin + j, xmin + k) * a.cin + c]; }, th, xn, tv, yn, TS, vfirst);
        }
        if (a.cin == 1) res[1] = res[2] = res[0];
    }
    if (!live) return;
    ROI_STORE_PIXEL(a, i, a.cin, res[c]);
}

// The training case -- grey ROIs no larger than the output (kmax == 3: both scales <= 1), S <= 320 -- in the shape of
// roi_turn_resize3_kernel: one block per BAND_RPB consecutive output rows of one image, the image's scalars and a thread's horizontal
// taps fetched once per block, the band of T = transpose^bit2(src) that the inner rows among the block's rows draw on staged once
// (band3_stage of roi_resample.h).  A block whose rows are all fill stages nothing and reads no source byte.
__global__ __launch_bounds__(320) void roi_fit_resize3_kernel(FitArgs a) {
    const unsigned nrb = (unsigned)(a.S + BAND_RPB - 1) / BAND_RPB;
    const int img = (int)(blockIdx.x / nrb);
    const int y0 = (int)(blockIdx.x - (unsigned)img * nrb) * BAND_RPB;
    const bool live = (int)threadIdx.x < a.S;
    const int x = live ? (int)threadIdx.x : a.S - 1;
    const int32_t* m = a.meta + (size_t)img * FIT_META;
    const int nh = m[M_NH], nw = m[M_NW], oy = m[M_OY], ox = m[M_OX], fill = m[M_FILL];
    const int ylast = y0 + BAND_RPB - 1 < a.S ? y0 + BAND_RPB - 1 : a.S - 1;
    const int ylo = y0 - oy > 0 ? y0 - oy : 0, yhi = ylast - oy < nh - 1 ? ylast - oy : nh - 1;    // the block's inner rows
    if (ylo > yhi) {                                     // block-uniform: fill rows only
        if (!live) return;
        const int res[3] = {fill, fill, fill};
        for (int y = y0; y <= ylast; ++y) ROI_STORE_PIXEL(a, ((int64_t)img * a.S + y) * a.S + x, a.cin, res[c]);
        return;
    }
    // (the setup kernel cut h and w to the caller's maxima, which are <= S <= 320 here)
    const int h = m[M_H], w = m[M_W], stride = m[M_STRIDE];
    const uint8_t* src = a.pixels + a.offs[img];
    const int fl = a.flips ? a.flips[img] & a.codemask : 0;
    const bool vflip = fl & 1, hflip = fl & 2, turned = fl & 4;
    const int ht = turned ? w : h, wt = turned ? h : w;
    const int TS = a.S;
    const bool inside = x - ox >= 0 && x - ox < nw;
    const int32_t* th = a.tab + ((size_t)(img * 2 + 0) * (2 + a.kmax)) * a.S + (inside ? x - ox : 0);
    const int32_t* tv = a.tab + ((size_t)(img * 2 + 1) * (2 + a.kmax)) * a.S;
    __shared__ uint8_t strip[BAND_ROWS][BAND_PITCH];
    const Band3 b = band3_stage(strip, src, stride, ht, wt, vflip, hflip, turned, th, tv, TS, y0 - oy, ylo, yhi);
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int r = 0; r < BAND_RPB; ++r) {
        const int y = y0 + r;
        if (y >= a.S) break;
        const int v = inside && y - oy >= 0 && y - oy < nh ? band3_row(strip, b, r) : fill;
        const int res[3] = {v, v, v};
        ROI_STORE_PIXEL(a, ((int64_t)img * a.S + y) * a.S + x, a.cin, res[c]);
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
    a.pixels = pixels; a.offs = offs; a.hs = a.ws = nullptr; a.flips = cd; a.meta = meta; a.tab = tab;
    a.out = out; a.out_u8 = out_u8; a.codemask = codemask;
    roi_args_desc(a, d, kmax);
    const int fbx = roi_row_threads(d->S);
    if (d->in_channels == 1 && kmax == 3 && d->S <= 320)     // (kmax == 3: no ROI is larger than the output, so wt <= S <= 320)
        hipLaunchKernelGGL(roi_fit_resize3_kernel, dim3((unsigned)(d->n_img * cdiv(d->S, BAND_RPB))), dim3(fbx), 0, st, a);
    else
        hipLaunchKernelGGL(roi_fit_resize_kernel, dim3((unsigned)(d->n_img * d->S), (unsigned)cdiv(d->S, fbx)), dim3(fbx), 0, st, a);
    IFCBK_LAUNCH_CHECK(ctx, "roi_fit_resize");
    return 0;
}
