"""Cases, path predicates and helpers for the quarter-turn kernels of ifcbk_roi_preprocess (csrc/roi_turn.hip, flip_bits_valid == 2),
shared by tests/test_gpu_roi_turn.py (GPU) and tests/test_roi_turn_cpu.py (CPU twin).  Built on roi_bounds.py: the same pixel
generator, checkers and float-stage bounds.  Everything here runs on the CPU.

Code byte: bit0 = vertical flip, bit1 = horizontal flip, bit2 = transpose; the image the resize sees is
hflip^bit1( vflip^bit0( transpose^bit2( src ) ) ).  `seen(roi, code)` is that image in numpy; the expected u8 plane is the oracle's
resize of it.  Equality, no tolerance.

Every batch lists its shapes twice: ROI i of the first half carries code i % 8, its twin in the second half code (i + 4) % 8, so
each shape is resized once turned and once unturned, and every batch mixes both."""
import numpy as np

import roi_bounds as rb
from oracle.pil_resize import resize_bilinear_u8, vertical_first

MEAN, STD, TSC, TSH = rb.MEAN, rb.STD, rb.TSC, rb.TSH


def seen(roi, code):
    a = np.swapaxes(roi, 0, 1) if code & 4 else roi
    a = a[::-1] if code & 1 else a
    a = a[:, ::-1] if code & 2 else a
    return np.ascontiguousarray(a)


def seen_dims(h, w, code):
    return (w, h) if code & 4 else (h, w)


def _resize3(cin, S, kmax, ht, wt):
    return cin == 1 and kmax == 3 and S <= 320


def _staged(cin, S, kmax, ht, wt):
    return not _resize3(cin, S, kmax, ht, wt) and cin == 1 and kmax <= 5 and wt <= 640


def _generic(cin, S, kmax, ht, wt):
    return not (_resize3(cin, S, kmax, ht, wt) or _staged(cin, S, kmax, ht, wt))


# path -> (predicate(cin, S, kmax, ht, wt) on the TURNED dims, the source text of roi_turn.hip it mirrors)
PATHS = {
    'roi_turn_resize3_kernel': (_resize3, 'if (d->in_channels == 1 && kmax == 3 && d->S <= 320)'),
    'roi_turn_resize_kernel staged': (_staged, 'const bool staged = a.cin == 1 && a.kmax <= TLR && wt <= TLW;'),
    'roi_turn_resize_kernel generic': (_generic, '} else for (int c = 0; c < a.cin; ++c) {'),
    'roi_turn_coeffs_kernel': (lambda cin, S, kmax, ht, wt: True,
                               'hipLaunchKernelGGL(roi_turn_coeffs_kernel, dim3(cdiv(nco, 256)), dim3(256), 0, st, hs, ws, flips, d->n_img, d->S, kmax, (int32_t*)ctx->ws);'),
}
# further source text the predicates and the case table rely on (with roi_bounds.QUOTED_SHARED, looked up in roi_resample.h)
QUOTED = ('constexpr int TLR = 5, TLW = 640;', '__shared__ uint8_t strip[BAND_ROWS][BAND_PITCH];',
          'const int ht = turned ? w : h, wt = turned ? h : w;', 'const bool vfirst = ht > 100 * wt && ht > a.S;',
          'int inSize = (axis == 0) != turned ? ws[img] : hs[img];', 'const int tbx = roi_row_threads(d->S);')
# roi.hip: the only way into roi_turn.hip
BRANCH = 'if (d->flip_bits_valid == 2)'


def _tcase(name, shapes, S, **kw):
    n = len(shapes)
    codes = [i % 8 for i in range(n)] + [(i + 4) % 8 for i in range(n)]
    return rb._case(name, list(shapes) + list(shapes), S, flips=codes, **kw)


TURN = [
    # ---- kmax == 3, S <= 320: roi_turn_resize3_kernel (299: a 3-row tail block; 40: 64 threads per row)
    _tcase('turn small299', rb._small(299), 299, mean=MEAN, std=STD),
    _tcase('turn small299 float only', rb._small(299), 299, u8=False, tsc=TSC, tsh=TSH, pix='turn small299'),
    _tcase('turn small224 fp32 norm tin c16', rb._small(224), 224, dtype='fp32', mean=MEAN, std=STD, tsc=TSC, tsh=TSH, cout=16),
    _tcase('turn small224 u8 only', rb._small(224), 224, out=False, pix='turn small224 fp32 norm tin c16'),
    _tcase('turn small40', rb._small(40), 40, mean=MEAN, std=STD),
    # ---- kmax == 3, S > 320: staged rows; a turned ROI's width is its source height (320 / 321 around the 320 threads of a row)
    _tcase('turn small384', rb._small(384) + [(384, 320), (320, 384), (200, 321), (321, 200)], 384, mean=MEAN, std=STD),
    # ---- kmax == 5: staged.  Turned, (5, 598), (4, 597), (5, 501) run the vertical pass first and (598, 5) does not; unturned it is
    # the reverse; (6, 598) and (5, 500) stay horizontal-first either way
    _tcase('turn mid299', [(5, 598), (598, 5), (4, 597), (6, 598), (5, 501), (5, 500), (598, 598), (300, 299), (299, 598), (7, 301), (1, 1)],
           299, mean=MEAN, std=STD),
    _tcase('turn mid224 fp32', [(3, 448), (4, 401), (4, 400), (448, 448), (225, 224)], 224, dtype='fp32', mean=MEAN, std=STD, tsc=TSC, tsh=TSH),
    # ---- the 640-wide staging limit on the turned width.  At S = 384 a max dim of 641 is still kmax 5 and the limit decides: (30, 641)
    # is staged turned and generic unturned, (641, 30) the reverse.  At S = 299 the same shapes are kmax 7: all generic, and (6, 641)
    # turned runs the vertical pass first there
    _tcase('turn wide384', [(30, 641), (641, 30), (6, 641), (100, 640), (640, 100)], 384, mean=MEAN, std=STD),
    _tcase('turn wide299', [(30, 641), (641, 30), (6, 641), (100, 640), (640, 100)], 299, mean=MEAN, std=STD, pix='turn wide384'),
    # ---- generic loop: kmax 11, RGB
    _tcase('turn big224', [(100, 672), (5, 672), (672, 5), (3, 1000), (1000, 3), (10, 1000)], 224, tsc=TSC, tsh=TSH),
    _tcase('turn rgb299', [(41, 67), (400, 350), (5, 700), (700, 5), (1, 1)], 299, cin=3, mean=MEAN, std=STD),
]


def paths(case):
    """the arithmetic path of each ROI of the batch"""
    k = rb.kmax(case)
    out = []
    for (h, w), code in zip(case['rois'], case['flips']):
        ht, wt = seen_dims(h, w, code)
        hit = [p for p, (pred, _) in PATHS.items() if p != 'roi_turn_coeffs_kernel' and pred(case['cin'], case['S'], k, ht, wt)]
        assert len(hit) == 1, (case['name'], h, w, hit)
        out.append(hit[0])
    return out


def vfirst(case):
    return [vertical_first(*seen_dims(h, w, code), case['S']) for (h, w), code in zip(case['rois'], case['flips'])]


def expected_u8(case, rois, codes=None):
    """[n][S][S][cin] u8: the oracle's resize of each ROI as the resize sees it"""
    S = case['S']
    codes = case['flips'] if codes is None else codes
    return np.stack([resize_bilinear_u8(seen(r, f), S, S).reshape(S, S, case['cin']) for r, f in zip(rois, codes)])
