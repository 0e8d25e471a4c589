// Host/device arithmetic of the aspect-preserving ROI resize (roi_fit.hip, TRAIN --pad): inner size, placement, tap bound and the
// border-fill rounding.  Plain C++ so that scripts/roi_fit_dims_check.cpp can compile the same functions for the host alone.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IFCBK_HD __host__ __device__
#else
#define IFCBK_HD
#endif

struct ifcbk_fit_dims {
    int nh, nw;   // inner image (the seen image resized, aspect kept)
    int oy, ox;   // its top-left corner in the S x S output
};

// PIL.ImageOps.contain + ImageOps.pad(centering = (0.5, 0.5)) for a seen image of ht x wt pixels and an S x S output:
//   wt == ht: S x S;  wt > ht: nw = S, nh = round(ht / wt * S);  wt < ht: nh = S, nw = round(wt / ht * S)
// quotient first, then the product, IEEE double, no contraction; round = half to even (rint).  A size that rounds to 0 is
// clamped to 1 (Pillow cannot resize to zero: the one place this goes beyond ImageOps.pad).  The offsets are
// rint((S - n) * 0.5): half to even, so a gap of 1 leaves the line behind the image and a gap of 3 puts two in front.
IFCBK_HD static inline ifcbk_fit_dims ifcbk_fit_dims_for(int ht, int wt, int S) {
#pragma clang fp contract(off)
    ifcbk_fit_dims d;
    d.nh = d.nw = S;
    if (wt > ht) {
        double q = (double)ht / (double)wt;
        d.nh = (int)rint(q * (double)S);
    } else if (wt < ht) {
        double q = (double)wt / (double)ht;
        d.nw = (int)rint(q * (double)S);
    }
    if (d.nh < 1) d.nh = 1;
    if (d.nw < 1) d.nw = 1;
    d.ox = (int)rint((double)(S - d.nw) * 0.5);
    d.oy = (int)rint((double)(S - d.nh) * 0.5);
    return d;
}

// Taps per output index, for every ROI whose dims are within max_h x max_w (turned or not: M = max(max_h, max_w) bounds both seen
// dims).  An axis of input size `in` and output size `n` has scale = in / n, support = max(scale, 1), and a window of
// (int)(c + support + 0.5) - (int)(c - support + 0.5) <= 2 * ceil(support) + 1 taps (Pillow's ksize).
//   * long axis L (output S):  scale = L / S <= M / S.
//   * short axis s <= L, output n = max(1, rint(q)), q = s * S / L:
//       L <= S:  q >= s, s an integer, so n >= s and scale <= 1;
//       L >  S, n == 1:  rint(q) <= 1 means q <= 3/2, so scale = s = q * L / S <= 3/2 * L / S;
//       L >  S, n >= 2:  q >= 3/2 and n >= q - 1/2, so scale <= (L / S) * q / (q - 1/2) <= 3/2 * L / S.
//     (q is computed with two roundings of 2^-53 relative; an exact q lies at least 1 / (2 L) away from a tie it is not on, so the
//      computed rint is the exact one.)
// The squash path's bound, scale <= M / S, therefore does not hold: 598 x 5 at 299 has nw = 2 and scale 2.5 against 2.0.
//   M <= S: 3 taps;   M > S: 2 * ceil(3 M / (2 S)) + 1.
IFCBK_HD static inline int ifcbk_fit_kmax(int max_h, int max_w, int S) {
    int64_t m = max_h > max_w ? max_h : max_w;
    if (m <= S) return 3;
    int64_t c = (3 * m + 2 * (int64_t)S - 1) / (2 * (int64_t)S);
    return (int)c * 2 + 1;
}

// rounded mean of n border bytes with sum `sum`: (2 sum + n) / (2 n), integers
IFCBK_HD static inline int ifcbk_fit_fill(uint64_t sum, uint64_t n) {
    return (int)((2 * sum + n) / (2 * n));
}

// number of border pixels of an h x w ROI (rows 0 and h-1, columns 0 and w-1, each pixel once; h <= 2 or w <= 2: every pixel)
IFCBK_HD static inline int64_t ifcbk_fit_border_count(int h, int w) {
    return (h <= 2 || w <= 2) ? (int64_t)h * w : 2 * (int64_t)w + 2 * (int64_t)(h - 2);
}

// b-th border pixel, b in [0, count): row 0 left to right, row h-1, then the side columns of rows 1 .. h-2 in pairs
IFCBK_HD static inline void ifcbk_fit_border_at(int h, int w, int64_t b, int* r, int* c) {
    if (h <= 2 || w <= 2) { *r = (int)(b / w); *c = (int)(b - (int64_t)*r * w); return; }
    if (b < w) { *r = 0; *c = (int)b; return; }
    if (b < 2 * (int64_t)w) { *r = h - 1; *c = (int)(b - w); return; }
    b -= 2 * (int64_t)w;
    *r = 1 + (int)(b >> 1);
    *c = (b & 1) ? w - 1 : 0;
}
