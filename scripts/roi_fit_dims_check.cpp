// Host-only check of ifcb_classifier_amd/csrc/roi_fit_dims.h (the size, placement, tap-bound and border-fill arithmetic of roi_fit.hip),
// meant to be built with the sanitizers and run on the CPU:
//     clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//         scripts/roi_fit_dims_check.cpp -o /tmp/roi_fit_dims_check && /tmp/roi_fit_dims_check
// 1. every shape of tests/roi_fit_cases.py (both orientations, its output sizes): the window of every output index of both axes,
//    computed with the setup kernel's arithmetic, holds at most ifcbk_fit_kmax(max dims) taps, lies inside the input, and the
//    inner rectangle lies inside the output;
// 2. the same for every (L, s <= L) with L <= 1300, and L in a band around each multiple of S up to 12 S, at S = 40, 224, 299, 384;
// 3. the border enumeration visits each border pixel exactly once and the fill equals a brute-force mask mean.
// Prints the dims of the case shapes and returns non-zero on any failure.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../ifcb_classifier_amd/csrc/roi_fit_dims.h"

static int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++fails < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
        }                                                 \
    } while (0)

// the window of output index xx (roi_fit_setup_kernel): -> tap count, first index in *first
static int window(int inSize, int outSize, int xx, int* first) {
    double scale = (double)((float)inSize - 0.0f) / (double)outSize;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    double support = 1.0 * filterscale;
    double center = 0.0 + ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    *first = xmin;
    return xmax - xmin;
}

static int most_taps(int inSize, int outSize) {
    int worst = 0;
    for (int xx = 0; xx < outSize; ++xx) {
        int first, n = window(inSize, outSize, xx, &first);
        CHECK(n >= 1 && first >= 0 && first + n <= inSize, "window in %d out %d xx %d: first %d n %d", inSize, outSize, xx, first, n);
        if (n > worst) worst = n;
    }
    return worst;
}

static void check_shape(int ht, int wt, int S, int kmax, bool print) {
    ifcbk_fit_dims d = ifcbk_fit_dims_for(ht, wt, S);
    CHECK(d.nh >= 1 && d.nh <= S && d.nw >= 1 && d.nw <= S, "dims %d x %d S %d: %d x %d", ht, wt, S, d.nh, d.nw);
    CHECK(d.oy >= 0 && d.oy + d.nh <= S && d.ox >= 0 && d.ox + d.nw <= S, "placement %d x %d S %d: oy %d ox %d", ht, wt, S, d.oy, d.ox);
    CHECK((ht >= wt ? d.nh : d.nw) == S, "long side %d x %d S %d", ht, wt, S);
    int th = most_taps(wt, d.nw), tv = most_taps(ht, d.nh);
    CHECK(th <= kmax && tv <= kmax, "taps %d x %d S %d: h %d v %d > kmax %d", ht, wt, S, th, tv, kmax);
    if (print) printf("dims %d %d %d -> %d %d %d %d taps %d %d kmax %d\n", ht, wt, S, d.nh, d.nw, d.oy, d.ox, tv, th, kmax);
}

static void check_fill(int h, int w, unsigned seed) {
    std::vector<unsigned char> px((size_t)h * w);
    for (auto& p : px) { seed = seed * 1664525u + 1013904223u; p = (unsigned char)(seed >> 24); }
    std::vector<int> hit((size_t)h * w, 0);
    const int64_t nb = ifcbk_fit_border_count(h, w);
    uint64_t sum = 0;
    for (int64_t b = 0; b < nb; ++b) {
        int r, c;
        ifcbk_fit_border_at(h, w, b, &r, &c);
        CHECK(r >= 0 && r < h && c >= 0 && c < w, "border_at %d x %d b %lld: (%d, %d)", h, w, (long long)b, r, c);
        if (r < 0 || r >= h || c < 0 || c >= w) return;
        hit[(size_t)r * w + c]++;
        sum += px[(size_t)r * w + c];
    }
    uint64_t want_sum = 0, want_n = 0;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const bool border = r == 0 || r == h - 1 || c == 0 || c == w - 1;
            CHECK(hit[(size_t)r * w + c] == (border ? 1 : 0), "border set %d x %d at (%d, %d): %d", h, w, r, c, hit[(size_t)r * w + c]);
            if (border) { want_sum += px[(size_t)r * w + c]; want_n++; }
        }
    CHECK((uint64_t)nb == want_n && sum == want_sum, "border %d x %d: n %lld sum %llu, want %llu %llu", h, w, (long long)nb,
          (unsigned long long)sum, (unsigned long long)want_n, (unsigned long long)want_sum);
    const int f = ifcbk_fit_fill(sum, (uint64_t)nb);
    // round(sum / n) to the nearest, halves up: | 2 n f - 2 sum | <= n
    const long long e = 2 * (long long)nb * f - 2 * (long long)sum;
    CHECK(f >= 0 && f <= 255 && e <= (long long)nb && e > -(long long)nb, "fill %d x %d: %d", h, w, f);
}

int main() {
    // tests/roi_fit_cases.py, by group: {S, shapes...}
    static const int s40[][2] = {{1, 1}, {40, 40}, {40, 39}, {37, 40}, {10, 20}, {20, 10}, {3, 40}, {40, 3}, {1, 40}};
    static const int s299[][2] = {{598, 5}, {5, 598}, {598, 21}, {4, 597}, {640, 3}, {600, 1}, {1, 600}, {597, 598}, {300, 299}, {299, 598}, {7, 301}};
    static const int s224[][2] = {{3, 448}, {448, 448}, {225, 224}, {301, 2}};
    static const int s384[][2] = {{30, 641}, {641, 30}, {200, 321}, {384, 320}};
    static const int rgb[][2] = {{41, 67}, {400, 350}, {5, 700}, {1, 1}};
    struct { int S; const int (*shp)[2]; int n; } groups[] = {{40, s40, 9}, {299, s299, 11}, {224, s224, 4}, {384, s384, 4}, {299, rgb, 4}};
    for (auto& g : groups) {
        int mh = 1, mw = 1;
        for (int i = 0; i < g.n; ++i) { if (g.shp[i][0] > mh) mh = g.shp[i][0]; if (g.shp[i][1] > mw) mw = g.shp[i][1]; }
        const int kmax = ifcbk_fit_kmax(mh, mw, g.S);
        for (int i = 0; i < g.n; ++i) {
            check_shape(g.shp[i][0], g.shp[i][1], g.S, kmax, true);
            check_shape(g.shp[i][1], g.shp[i][0], g.S, kmax, true);
            // and under the bound of its own dims alone
            check_shape(g.shp[i][0], g.shp[i][1], g.S, ifcbk_fit_kmax(g.shp[i][0], g.shp[i][1], g.S), false);
            if ((int64_t)g.shp[i][0] * g.shp[i][1] <= 1 << 20) check_fill(g.shp[i][0], g.shp[i][1], 7u + i);
        }
    }
    static const int sizes[] = {40, 224, 299, 384};
    long long shapes = 0;
    for (int S : sizes) {
        for (int L = 1; L <= 12 * S + 3; ++L) {
            const int near = L % S;
            if (L > 1300 && near > 3 && near < S - 3) continue;
            const int kmax = ifcbk_fit_kmax(L, L, S);
            for (int s = 1; s <= L; ++s) {
                // only the shapes that set the bound need every index: the short axis's scale peaks where n is small
                ifcbk_fit_dims d = ifcbk_fit_dims_for(L, s, S);
                if (L > 1300 && d.nw > 8 && s != L) continue;
                check_shape(L, s, S, kmax, false);
                ++shapes;
            }
        }
    }
    for (int h = 1; h <= 9; ++h)
        for (int w = 1; w <= 9; ++w) check_fill(h, w, 100u * h + w);
    check_fill(1000, 1000, 5u);
    check_fill(2, 777, 6u);
    check_fill(777, 1, 8u);
    printf("%lld grid shapes, %d failures\n", shapes, fails);
    return fails ? 1 : 0;
}
