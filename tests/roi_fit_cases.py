"""Cases, path predicates and helpers for the aspect-preserving resize ifcbk_roi_preprocess_fit (csrc/roi_fit.hip, TRAIN --pad), shared
by tests/test_gpu_roi_fit.py (GPU) and tests/test_roi_fit_cpu.py (CPU twin).  Built on roi_bounds.py and roi_turn_cases.py: the same
pixel generator, code byte, checkers and float-stage bounds.  Everything here runs on the CPU.

Contract: the u8 plane equals PIL.ImageOps.pad(seen, (S, S), Image.BILINEAR, color=FILL, centering=(0.5, 0.5)), where ``seen`` is
the image after the flip / transpose code.  The numpy twin below (``expected_u8``) is fill + paste of the oracle's resize to the
inner size; the CPU test proves it equal to the installed Pillow.  Equality, no tolerance.

Every batch lists its shapes twice as roi_turn_cases does: ROI i of the first half carries code i % 8, its twin in the second half
code (i + 4) % 8, so each shape is fitted once turned and once unturned, and every batch mixes both."""
import numpy as np

import roi_bounds as rb
import roi_turn_cases as tc
from oracle.pil_resize import _coeffs, resize_bilinear_u8, vertical_first

MEAN, STD, TSC, TSH = rb.MEAN, rb.STD, rb.TSC, rb.TSH
seen, seen_dims = tc.seen, tc.seen_dims
META_WORDS = 16           # roi_fit.hip: FIT_META


def fit_dims(ht, wt, S):
    """(nh, nw, oy, ox): ImageOps.contain's inner size (half-to-even round of quotient * S, clamped to >= 1: Pillow cannot resize to
    a zero size) and ImageOps.pad's centred placement (half-to-even round of half the gap)"""
    nh = nw = S
    if wt > ht:
        nh = round(ht / wt * S)
    elif wt < ht:
        nw = round(wt / ht * S)
    nh, nw = max(nh, 1), max(nw, 1)
    return nh, nw, round((S - nh) * 0.5), round((S - nw) * 0.5)


def contain_is_zero(ht, wt, S):
    """ImageOps.contain asks Pillow for a zero size (the clamp shapes: our definition goes beyond ImageOps.pad there)"""
    return (wt > ht and round(ht / wt * S) == 0) or (wt < ht and round(wt / ht * S) == 0)


def border_fill(roi):
    """per channel (2 sum + n) // (2 n) over rows 0 and h-1 and columns 0 and w-1, each pixel once; [cin] ints"""
    a = np.asarray(roi)
    a = a[:, :, None] if a.ndim == 2 else a
    h, w = a.shape[:2]
    if h <= 2 or w <= 2:
        px = a.reshape(-1, a.shape[2])
    else:
        px = np.concatenate([a[0], a[h - 1], a[1:h - 1, 0], a[1:h - 1, w - 1]])
    n = px.shape[0]
    return [int((2 * int(s) + n) // (2 * n)) for s in px.astype(np.int64).sum(0)]


def fit_kmax(max_h, max_w, S):
    """roi_fit_dims.h: ifcbk_fit_kmax"""
    m = max(max_h, max_w)
    if m <= S:
        return 3
    return ((3 * m + 2 * S - 1) // (2 * S)) * 2 + 1


def workspace_bytes(n, S, kmax):
    return n * META_WORDS * 4 + n * 2 * S * (2 + kmax) * 4


def kmax(case):
    return fit_kmax(*rb.maxima(case), case['S'])


def _rows(ht, nh):
    """tap count of every inner output row"""
    return _coeffs(ht, nh)[0][:, 1]


def _resize3(cin, S, kmax, ht, wt):
    return cin == 1 and kmax == 3 and S <= 320


def _staged(cin, S, kmax, ht, wt):
    nh = fit_dims(ht, wt, S)[0]
    return not _resize3(cin, S, kmax, ht, wt) and cin == 1 and wt <= 640 and bool((_rows(ht, nh) <= 5).any())


def _generic(cin, S, kmax, ht, wt):
    nh = fit_dims(ht, wt, S)[0]
    return not _resize3(cin, S, kmax, ht, wt) and (cin != 1 or wt > 640 or bool((_rows(ht, nh) > 5).any()))


def _fill_rows(cin, S, kmax, ht, wt):
    return not _resize3(cin, S, kmax, ht, wt) and fit_dims(ht, wt, S)[0] < S


def _fill_block(cin, S, kmax, ht, wt):
    """a block of 8 output rows of roi_fit_resize3_kernel without an inner row"""
    nh, _, oy, _ = fit_dims(ht, wt, S)
    return _resize3(cin, S, kmax, ht, wt) and any(min(y0 + 7, S - 1) < oy or y0 >= oy + nh for y0 in range(0, S, 8))


# path -> (predicate(cin, S, kmax, ht, wt) on the SEEN dims, the source text of roi_fit.hip it mirrors).  A ROI can take several
# paths of roi_fit_resize_kernel: the choice is made per output row.
PATHS = {
    'roi_fit_resize3_kernel': (_resize3, 'if (d->in_channels == 1 && kmax == 3 && d->S <= 320)'),
    'roi_fit_resize3_kernel fill block': (_fill_block, 'if (ylo > yhi) {'),
    'roi_fit_resize_kernel staged': (_staged, 'const bool staged = a.cin == 1 && yn <= FLR && wt <= FLW;'),
    'roi_fit_resize_kernel generic': (_generic, '} else if (inside) { for (int c = 0; c < a.cin; ++c) {'),
    'roi_fit_resize_kernel fill row': (_fill_rows, 'if (yy < 0 || yy >= nh) {'),
    'roi_fit_setup_kernel': (lambda cin, S, kmax, ht, wt: True,
                             'hipLaunchKernelGGL(roi_fit_setup_kernel, dim3((unsigned)d->n_img), dim3(256), 0, st, pixels, offs, hs, ws, cd, codemask, '
                             'max_h, max_w, d->S, d->in_channels, kmax, fill, meta, tab);'),
}
# further source text the predicates, the case table and the workspace formula rely on (with roi_bounds.QUOTED_SHARED, looked up in
# roi_resample.h)
QUOTED = ('constexpr int FLR = 5, FLW = 640;', '__shared__ uint8_t strip[BAND_ROWS][BAND_PITCH];', 'constexpr int FIT_META = 16;',
          'const int ht = turned ? w : h, wt = turned ? h : w;', 'const bool vfirst = (int64_t)ht > 100 * (int64_t)wt && nh < ht;',
          'const int fbx = roi_row_threads(d->S);',
          'return (size_t)d->n_img * FIT_META * sizeof(int32_t) + (size_t)d->n_img * 2 * d->S * (2 + kmax) * sizeof(int32_t);',
          'if (fill < -1 || fill > 255) IFCBK_FAIL(ctx, IFCBK_EINVAL,')
QUOTED_DIMS = ('if (m <= S) return 3;', 'int64_t c = (3 * m + 2 * (int64_t)S - 1) / (2 * (int64_t)S);', 'return (int)c * 2 + 1;',
               'd.nh = (int)rint(q * (double)S);', 'd.nw = (int)rint(q * (double)S);', 'if (d.nh < 1) d.nh = 1;', 'if (d.nw < 1) d.nw = 1;',
               'd.ox = (int)rint((double)(S - d.nw) * 0.5);', 'd.oy = (int)rint((double)(S - d.nh) * 0.5);',
               'return (int)((2 * sum + n) / (2 * n));')

S40 = [(1, 1), (40, 40), (40, 39), (37, 40), (10, 20), (20, 10), (3, 40), (40, 3), (1, 40)]
S299 = [(598, 5), (5, 598), (598, 21), (4, 597), (640, 3), (600, 1), (1, 600), (597, 598), (300, 299), (299, 598), (7, 301)]
S224 = [(3, 448), (448, 448), (225, 224), (301, 2)]
S384 = [(30, 641), (641, 30), (200, 321), (384, 320)]
RGB299 = [(41, 67), (400, 350), (5, 700), (1, 1)]
# the benchmark's class at its own size (not in the issue's table, which holds no kmax == 3 batch at 299): 299 = 37 * 8 + 3, a tail block
SMALL299 = [(1, 1), (299, 299), (299, 298), (150, 61), (17, 5), (7, 273), (221, 221), (1, 299), (299, 1), (100, 299)]
CLAMP = {(600, 1), (1, 600)}         # the shapes where contain asks for a zero size ((640, 3) and (301, 2) round to 1 on their own)


def _fcase(name, shapes, S, fill, **kw):
    c = tc._tcase(name, shapes, S, **kw)
    c['fill'] = fill
    return c


FIT = [
    # ---- S = 40, three taps: roi_fit_resize3_kernel with 64 threads per row; gaps 0 / 1 / 3 on either axis, upscaling
    _fcase('fit small40', S40, 40, 'border', mean=MEAN, std=STD),
    _fcase('fit small40 fill0 fp32 c16', S40, 40, 0, dtype='fp32', cout=16, pix='fit small40'),
    # ---- S = 299, kmax 9: roi_fit_resize_kernel; vertical-first with nw = 2 / 10 / 1, the zero-size clamp, a 298.5 tie, the tap bound
    _fcase('fit mid299', S299, 299, 'border', mean=MEAN, std=STD),
    _fcase('fit mid299 fill255 u8 only', S299, 299, 255, out=False, pix='fit mid299'),
    # ---- S = 224, fp32
    _fcase('fit mid224 fp32 fill128', S224, 224, 128, dtype='fp32', mean=MEAN, std=STD, tsc=TSC, tsh=TSH),
    # ---- S = 384: the 640-wide staging limit on the seen width, ROIs wider than the 320 threads of a row block
    _fcase('fit stage384', S384, 384, 'border', mean=MEAN, std=STD),
    # ---- RGB: per-channel border fill, the generic loop
    _fcase('fit rgb299', RGB299, 299, 'border', cin=3, mean=MEAN, std=STD),
    # ---- the benchmark's class at 299
    _fcase('fit small299 float only', SMALL299, 299, 'border', u8=False, tsc=TSC, tsh=TSH),
    _fcase('fit small299 fill77', SMALL299, 299, 77, mean=MEAN, std=STD, pix='fit small299 float only'),
]


def fill_arg(case):
    return -1 if case['fill'] == 'border' else int(case['fill'])


def paths(case):
    """the set of paths each ROI of the batch takes"""
    k = kmax(case)
    out = []
    for (h, w), code in zip(case['rois'], case['flips']):
        ht, wt = seen_dims(h, w, code)
        hit = {p for p, (pred, _) in PATHS.items() if pred(case['cin'], case['S'], k, ht, wt)}
        assert ('roi_fit_resize3_kernel' in hit) != bool(hit & {'roi_fit_resize_kernel staged', 'roi_fit_resize_kernel generic'}), (case['name'], h, w, hit)
        out.append(hit)
    return out


def vfirst(case):
    out = []
    for (h, w), code in zip(case['rois'], case['flips']):
        ht, wt = seen_dims(h, w, code)
        out.append(vertical_first(ht, wt, fit_dims(ht, wt, case['S'])[0]))
    return out


def fit_u8(img, S, fill):
    """[S][S][c] u8: the numpy twin of ImageOps.pad(img, (S, S), BILINEAR, color=fill, centering=(0.5, 0.5)); fill: one level per channel"""
    a = np.asarray(img, np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    nh, nw, oy, ox = fit_dims(a.shape[0], a.shape[1], S)
    out = np.empty((S, S, a.shape[2]), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    out[oy:oy + nh, ox:ox + nw] = resize_bilinear_u8(a, nh, nw).reshape(nh, nw, a.shape[2])
    return out


def fills(case, rois):
    """[n][cin] fill levels"""
    cin = case['cin']
    return [border_fill(r) if case['fill'] == 'border' else [int(case['fill'])] * cin for r in rois]


def expected_u8(case, rois, codes=None):
    """[n][S][S][cin] u8: fill + paste of the oracle's resize of each ROI as the resize sees it"""
    codes = case['flips'] if codes is None else codes
    return np.stack([fit_u8(seen(r, c), case['S'], f) for r, c, f in zip(rois, codes, fills(case, rois))])


def inner_mask(case, codes=None):
    """[n][S][S] bool: True inside the inner rectangle"""
    S = case['S']
    codes = case['flips'] if codes is None else codes
    m = np.zeros((len(case['rois']), S, S), bool)
    for i, ((h, w), code) in enumerate(zip(case['rois'], codes)):
        nh, nw, oy, ox = fit_dims(*seen_dims(h, w, code), S)
        m[i, oy:oy + nh, ox:ox + nw] = True
    return m
