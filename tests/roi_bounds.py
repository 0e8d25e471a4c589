"""Cases, path predicates and checkers for ifcbk_roi_preprocess (csrc/roi.hip), shared by tests/test_gpu_roi_paths.py (GPU) and
tests/test_roi_paths_cpu.py (CPU twin: oracle == installed Pillow on every case shape, the predicates' source text, the mutations).

A plain helper module like conv_bounds.py / op_bounds.py.  Everything here runs on the CPU.

Paths.  ifcbk_roi_preprocess picks the kernel from the BATCH (in_channels, S, and kmax, which comes from the caller's max_h / max_w),
roi_resize_kernel then picks its arithmetic per ROI.  PATHS restates those conditions on the host; each entry quotes the source
line it mirrors, and the CPU test asserts that line is still in roi.hip (QUOTED_SHARED: in roi_resample.h).

u8 plane.  Expected: oracle.pil_resize.resize_bilinear_u8 of the flipped ROI (the CPU twin proves it equal to Pillow for every shape
of the table).  Equality, no tolerance.

Float stage, as the kernels write it (one fp32 rounding u = 2^-24 per operation, -ffp-contract=on):
    v0 = (float)r / 255.0f            e0 = u |v0|
    v1 = v0 - mean                    e1 = e0 + u (|v1| + e0)
    v2 = v1 / std                     e2 = e1 / |std| + u (|v2| + e1 / |std|)
    v3 = v2 * tsc + tsh               e3 = |tsc| e2 + 2u (|v2 tsc| + |tsc| e2 + |tsh|)      (one rounding if contracted, two if not)
then the storage rounding, 1/2 ulp_out at |v3| + e3 (op_bounds.elem).  mean, std, tsc, tsh are the fp32 values the descriptor holds.
With mean 0, std 1, tsc 1, tsh 0 every step after the division is exact: the output is exactly rne_out(fl32(r / 255)).
"""
import zlib

import numpy as np
import torch

import op_bounds as ob
from oracle.pil_resize import resize_bilinear_u8

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TSC, TSH = (0.458, 0.448, 0.45), (-0.03, -0.088, -0.188)


def kmax_for(max_h, max_w, S):
    """roi.hip: kmax_for"""
    scale = max(max(max_h, max_w) / S, 1.0)
    return int(np.ceil(scale)) * 2 + 1


def block_x(S):
    """roi_resample.h: roi_row_threads (threads per output row)"""
    return 64 if S <= 64 else 128 if S <= 128 else 192 if S <= 192 else 256 if S <= 256 else 320


def _resize3(cin, S, kmax, h, w):
    return cin == 1 and kmax == 3 and S <= 320


def _fast3(cin, S, kmax, h, w):
    return not _resize3(cin, S, kmax, h, w) and cin == 1 and kmax == 3 and w <= block_x(S)


def _lds_ok(cin, S, kmax, h, w):
    return not _resize3(cin, S, kmax, h, w) and not _fast3(cin, S, kmax, h, w) and cin == 1 and kmax <= 5 and w <= 640


def _generic(cin, S, kmax, h, w):
    return not (_resize3(cin, S, kmax, h, w) or _fast3(cin, S, kmax, h, w) or _lds_ok(cin, S, kmax, h, w))


# path -> (predicate(cin, S, kmax, h, w), the source text of roi.hip it mirrors)
PATHS = {
    'roi_resize3_kernel': (_resize3, 'if (d->in_channels == 1 && kmax == 3 && d->S <= 320)'),
    'roi_resize_kernel fast3': (_fast3, 'const bool fast3 = a.cin == 1 && a.kmax == 3 && w <= (int)blockDim.x;'),
    'roi_resize_kernel lds_ok': (_lds_ok, 'const bool lds_ok = !fast3 && a.cin == 1 && a.kmax <= LR && w <= LW;'),
    'roi_resize_kernel generic': (_generic, '} else for (int c = 0; c < a.cin; ++c) {'),
    'roi_coeffs_kernel': (lambda cin, S, kmax, h, w: True, 'hipLaunchKernelGGL(roi_coeffs_kernel, dim3(cdiv(nco, 256)), dim3(256), 0, st, hs, ws, d->n_img, d->S, kmax, (int32_t*)ctx->ws);'),
}
# further source text the predicates rely on (constants and the pass-order rule)
QUOTED = ('constexpr int LR = 5, LW = 640;', 'constexpr int RPB = 8;', 'return (int)ceil(scale) * 2 + 1;',
          'const int bx = roi_row_threads(d->S);', 'const bool vfirst = h > 100 * w && h > a.S;')
# source text of csrc/roi_resample.h, the resampler the three kernel sets share: the threads-per-row ladder (block_x), and the
# constants and the column clamp of the band staging that roi_turn_cases.py and roi_fit_cases.py rely on
QUOTED_SHARED = ('inline int roi_row_threads(int S) { return S <= 64 ? 64 : S <= 128 ? 128 : S <= 192 ? 192 : S <= 256 ? 256 : 320; }',
                 'constexpr int BAND_RPB = 8, BAND_ROWS = 12, BAND_PITCH = 324;', 'const int wl = wt < 320 ? wt : 320;')


def _small(S):
    """ROIs no larger than the output (kmax == 3): the corners of the size range, the row-tail shapes and a few ragged ones"""
    rois = [(1, 1), (1, S), (S, 1), (S, S), (S - 1, S), (2, 3), (S, S - 1), (17, 5), (S // 2 + 1, S // 3), (3, S - 2), (S - 3, 7),
            (min(S, 150), min(S, 61)), (5, 2)]
    # A window of an enlarging axis holds two pixels; a third (the kernels' c2 / third row, tap 0 in front) appears only where the
    # double arithmetic of the bounds rounds up: at S = 299 for input sizes 7, 221 and 273 (one output index each), never at 224, 40
    # or 384 (searched over every size <= S; test_roi_paths_cpu.py checks the 299 batches hold such ROIs in both axes)
    return rois + ([(7, 273), (221, 221), (273, 7)] if S == 299 else [])


def _case(name, rois, S, cin=1, flips='cycle', dtype='bf16', out=True, u8=True, mean=(0, 0, 0), std=(1, 1, 1), tsc=(1, 1, 1), tsh=(0, 0, 0),
          cout=8, maxima=None, pix=None):
    if flips == 'cycle':
        flips = [(i + 1) % 4 for i in range(len(rois))]
    return dict(name=name, rois=rois, S=S, cin=cin, flips=flips, dtype=dtype, out=out, u8=u8, mean=mean, std=std, tsc=tsc, tsh=tsh, cout=cout,
                maxima=maxima, pix=pix or name)


ROI = [
    # ---- kmax == 3, S <= 320: roi_resize3_kernel (299 = 37 * 8 + 3: a 3-row tail block; 224 = 28 * 8: none; 40: 64 threads per row)
    _case('small299', _small(299), 299),
    _case('small299 norm', _small(299), 299, mean=MEAN, std=STD, pix='small299'),
    _case('small299 noflip fp32 norm', _small(299), 299, flips=None, dtype='fp32', mean=MEAN, std=STD),
    _case('small224 norm tin c16', _small(224), 224, mean=MEAN, std=STD, tsc=TSC, tsh=TSH, cout=16),
    _case('small224 noflip u8 only', _small(224), 224, flips=None, out=False),
    _case('small299 float only tin', _small(299), 299, u8=False, tsc=TSC, tsh=TSH),
    _case('small40 fp32 c16', _small(40), 40, dtype='fp32', cout=16),
    _case('small40 noflip', _small(40), 40, flips=None, mean=MEAN, std=STD),
    # ---- kmax == 3, S > 320: roi_resize_kernel fast3 (w <= 320), its wider ROIs take lds_ok
    _case('small384', _small(384) + [(384, 320), (200, 321)], 384, mean=MEAN, std=STD),
    _case('small384 noflip fp32', _small(384) + [(384, 320), (200, 321)], 384, flips=None, dtype='fp32', tsc=TSC, tsh=TSH),
    # ---- kmax == 5: lds_ok; (598, 5), (597, 4), (501, 5), (448, 3), (401, 4) run the vertical pass first, (500, 5), (400, 4), (598, 6) do not
    _case('mid299', [(598, 598), (300, 299), (598, 5), (597, 4), (598, 6), (501, 5), (500, 5), (20, 30), (1, 1), (299, 598), (7, 301),
                     (450, 333)], 299, mean=MEAN, std=STD),
    _case('mid224 noflip fp32', [(448, 448), (225, 224), (448, 3), (401, 4), (400, 4), (448, 5), (2, 3), (224, 448), (61, 150)], 224,
          flips=None, dtype='fp32', mean=MEAN, std=STD, tsc=TSC, tsh=TSH),
    _case('mid384 w640', [(768, 768), (385, 384), (100, 640), (768, 7), (33, 639), (384, 384), (1, 1)], 384),
    # ---- generic loop: w = 641, kmax = 7 and beyond, RGB
    _case('wide299', [(30, 641), (598, 5), (40, 90), (299, 299), (641, 6)], 299, mean=MEAN, std=STD),
    _case('big224 kmax7', [(672, 100), (672, 5), (449, 672), (3, 2), (224, 224), (601, 6), (600, 6)], 224, tsc=TSC, tsh=TSH),
    _case('big224 kmax11 noflip', [(1000, 3), (1000, 10), (1001, 10), (10, 1000), (50, 60)], 224, flips=None, dtype='fp32'),
    _case('rgb299', [(41, 67), (400, 350), (299, 299), (1, 1), (700, 5), (5, 700), (298, 300)], 299, cin=3, mean=MEAN, std=STD),
    _case('rgb224 noflip small', [(41, 67), (224, 224), (1, 2), (100, 7)], 224, cin=3, flips=None, dtype='fp32', cout=16),
    # ---- overstated maxima: the ROIs of a kmax == 3 batch under kmax 5 and 7 (test_overstated_maxima compares the planes)
    _case('small299 as kmax5', _small(299), 299, maxima=(598, 598), mean=MEAN, std=STD, pix='small299'),
    _case('small299 as kmax7', _small(299), 299, maxima=(600, 299), mean=MEAN, std=STD, pix='small299'),
]


def maxima(case):
    if case['maxima']:
        return case['maxima']
    return max(h for h, w in case['rois']), max(w for h, w in case['rois'])


def kmax(case):
    return kmax_for(*maxima(case), case['S'])


def paths(case):
    """the arithmetic path of each ROI of the batch"""
    k = kmax(case)
    out = []
    for h, w in case['rois']:
        hit = [p for p, (pred, _) in PATHS.items() if p != 'roi_coeffs_kernel' and pred(case['cin'], case['S'], k, h, w)]
        assert len(hit) == 1, (case['name'], h, w, hit)
        out.append(hit[0])
    return out


def pixels(case):
    """the batch's ROIs: random u8; the last one all 255, the one before it half 0 (clip8 at both ends)"""
    rng = np.random.default_rng(zlib.crc32(case['pix'].encode()))
    shp = (lambda h, w: (h, w)) if case['cin'] == 1 else (lambda h, w: (h, w, 3))
    rois = [rng.integers(0, 256, shp(h, w), dtype=np.uint8) for h, w in case['rois']]
    if len(rois) > 4:
        rois[-1][:] = 255
        rois[-2][:rois[-2].shape[0] // 2 + 1] = 0
    return rois


def flipped(roi, fl):
    a = roi[::-1] if fl & 1 else roi
    a = a[:, ::-1] if fl & 2 else a
    return np.ascontiguousarray(a)


def expected_u8(case, rois):
    """[n][S][S][cin] u8: the oracle's resize of each (flipped) ROI"""
    S = case['S']
    fl = case['flips'] or [0] * len(rois)
    return np.stack([resize_bilinear_u8(flipped(r, f), S, S).reshape(S, S, case['cin']) for r, f in zip(rois, fl)])


def check_u8(name, got, want):
    """bit-equal u8 planes [n][S][S][c]"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, (name, got.shape, want.shape, got.dtype)
    bad = got != want
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d u8 values differ (largest difference %d); first at (n, y, x, c) = %s: got %d want %d' % (
            name, int(bad.sum()), got.size, int(np.abs(got.astype(int) - want).max()), idx, int(got[idx]), int(want[idx])))


def float_stage(u8, mean, std, tsc, tsh):
    """(want, e) in float64 for u8 values [..., 3] (the last axis is the channel)"""
    r = torch.as_tensor(np.asarray(u8)).double()
    m, s, t, b = (torch.tensor([ob.f32(v) for v in x], dtype=torch.float64) for x in (mean, std, tsc, tsh))
    u = ob.U
    v0 = r / 255.0
    e0 = u * v0.abs()
    v1 = v0 - m
    e1 = e0 + u * (v1.abs() + e0)
    v2 = v1 / s
    e2 = e1 / s.abs() + u * (v2.abs() + e1 / s.abs())
    v3 = v2 * t + b
    e3 = t.abs() * e2 + 2 * u * ((v2 * t).abs() + t.abs() * e2 + b.abs())
    return v3, e3


def is_identity(case):
    return tuple(case['mean']) == (0, 0, 0) and tuple(case['std']) == (1, 1, 1) and tuple(case['tsc']) == (1, 1, 1) and tuple(case['tsh']) == (0, 0, 0)


def check_float(name, got, u8, case, family='roi float stage'):
    """got [n][S][S][cout] (any float dtype) against the float stage of the u8 plane [n][S][S][cin]"""
    out = case['dtype']
    u8 = np.asarray(u8)
    u3 = np.repeat(u8, 3, -1) if u8.shape[-1] == 1 else u8
    got = got.detach().cpu()
    ob.exact(name + ' pad channels', got[..., 3:].double(), torch.zeros_like(got[..., 3:]).double())
    want, e = float_stage(u3, case['mean'], case['std'], case['tsc'], case['tsh'])
    if is_identity(case):
        f = torch.from_numpy(u3.astype(np.float32) / np.float32(255))
        ob.exact(name + ' identity stage', got[..., :3], ob.rne(f.double(), out))
    ob.elem(name, got[..., :3], want, e, out, family, dims=('n', 'y', 'x', 'c'))
