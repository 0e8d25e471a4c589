"""A random affine as RandomAffine(degrees, translate, scale) with nearest sampling does it, in numpy: the coefficient function
(torchvision's inverse matrix, Pillow's FIX), the integer nearest-neighbour model, the border fill, the float stage of the resize
kernels as an exact table, and ONE case table that the CPU test holds against Pillow (a kernel's test would hold the kernel to it).

Nothing here imports the package: the coefficient function is written again from the formulas, and test_affine_cpu.py holds
neuston_data.affine_coefs against it."""
import math
import zlib
from fractions import Fraction

import numpy as np

IDENTITY = (65536, 0, 32768, 0, 65536, 32768)


def matrix(S, angle, translate, scale):
    """torchvision's _get_inverse_affine_matrix(center=(S * 0.5, S * 0.5), angle, translate, scale, shear=(0, 0)): six floats"""
    rot = math.radians(angle)
    cx = cy = S * 0.5
    tx, ty = translate
    a, b, c, d = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [v / scale for v in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def coefs_of(m):
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def coefs(S, angle, translate, scale):
    return coefs_of(matrix(S, angle, translate, scale))


def border_fill(src):
    """per channel the rounded mean (2 sum + cnt) // (2 cnt) of the outermost ring of src [S][S][C]: a list of C ints"""
    S = src.shape[0]
    ring = np.zeros((S, S), bool)
    ring[0] = ring[-1] = ring[:, 0] = ring[:, -1] = True
    cnt = int(ring.sum())
    assert cnt == (4 * S - 4 if S > 1 else 1)
    return [int((2 * int(src[..., c][ring].sum()) + cnt) // (2 * cnt)) for c in range(src.shape[2])]


def model(src, c, fill):
    """src [S][S][C] u8, c six ints, fill 0..255 or -1 -> [S][S][C] u8; every sum in 64 bits, no floating point"""
    S, _, C = src.shape
    f = np.array(border_fill(src) if fill < 0 else [fill] * C, np.uint8)
    c = [np.int64(v) for v in c]
    y, x = np.mgrid[0:S, 0:S].astype(np.int64)
    xin = (c[2] + c[0] * x + c[1] * y) >> 16
    yin = (c[5] + c[3] * x + c[4] * y) >> 16
    ok = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
    out = np.empty_like(src)
    out[:] = f
    out[ok] = src[yin[ok], xin[ok]]
    return out


def model_batch(src, coef, fill):
    return np.stack([model(src[n], coef[n], fill) for n in range(src.shape[0])])


def pillow(src, m, fill):
    """Image.transform((S, S), AFFINE, m, NEAREST, fillcolor) of one image [S][S][C]; fill: an int, or a list of C ints"""
    from PIL import Image
    S, _, C = src.shape
    if C == 1:
        img = Image.fromarray(src[..., 0], 'L')
        fc = int(fill[0] if isinstance(fill, (list, tuple)) else fill)
    else:
        img = Image.fromarray(src, 'RGB')
        fc = tuple(int(v) for v in fill) if isinstance(fill, (list, tuple)) else (int(fill),) * 3
    out = np.asarray(img.transform((S, S), Image.AFFINE, tuple(m), Image.NEAREST, fillcolor=fc))
    return out.reshape(S, S, C)


# ------------------------------------------------------------------------------------------------------------------------ float stage
def _f32(v):
    return float(np.float32(v))


def float_lut(mean, std, tsc, tsh):
    """[256][3] float32: the three float lines of roi.hip for every u8 level and channel -- v = fl(r / 255); v = fl(fl(v - mean) / std);
    v = fma(v, tsc, tsh) (one rounding: -ffp-contract=on fuses the last line) -- each rounding done exactly, through Fractions"""
    def _round(q):                                                     # a Fraction to the nearest float32, ties to even
        lo = np.float32(float(q))                                      # near it; its neighbours decide exactly
        cands = sorted({float(np.nextafter(lo, np.float32(-np.inf))), float(lo), float(np.nextafter(lo, np.float32(np.inf)))})
        best = min(cands, key=lambda t: (abs(Fraction(t) - q), int(np.float32(t).view(np.uint32)) & 1))
        return best

    lut = np.zeros((256, 3), np.float32)
    for ch in range(3):
        m, s, t, b = (Fraction(_f32(x[ch])) for x in (mean, std, tsc, tsh))
        for r in range(256):
            v = Fraction(_round(Fraction(r, 255)))
            v = Fraction(_round(v - m))
            v = Fraction(_round(v / s))
            lut[r, ch] = _round(v * t + b)
    return lut


def dense_bits(u8, lut, dtype, cout=8):
    """the dense tensor [N][S][S][cout] of a u8 batch [N][S][S][C] as raw bits: uint16 (bf16, round to nearest even) or uint32 (fp32)"""
    u3 = np.repeat(u8, 3, -1) if u8.shape[-1] == 1 else u8
    f = np.zeros(u8.shape[:3] + (cout,), np.float32)
    for ch in range(3):
        f[..., ch] = lut[u3[..., ch], ch]
    bits = f.view(np.uint32)
    if dtype == 'fp32':
        return bits
    b = bits.astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


FLOAT_STAGES = {
    'identity': dict(mean=(0, 0, 0), std=(1, 1, 1), tsc=(1, 1, 1), tsh=(0, 0, 0)),
    'norm+tin': dict(mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3), tsc=tuple(s / 0.5 for s in (0.229, 0.224, 0.225)),
                     tsh=tuple((m - 0.5) / 0.5 for m in (0.485, 0.456, 0.406))),
}


# ------------------------------------------------------------------------------------------------------------------------ the cases
def _case(name, S, N, C, params, fill, stage='norm+tin'):
    """params: one (angle, (tx, ty), scale) per image"""
    assert len(params) == N
    return dict(name=name, S=S, N=N, C=C, params=params, fill=fill, stage=stage)


def _rand(seed, N, S, deg=180.0, t=0.3, lo=0.25, hi=4.0):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(-deg, deg)), (int(round(rng.uniform(-t, t) * S)), int(round(rng.uniform(-t, t) * S))), float(rng.uniform(lo, hi)))
            for _ in range(N)]


CASES = [
    _case('S1 identity', 1, 1, 1, [(0.0, (0, 0), 1.0)], 0, 'identity'),
    _case('S1 N2 rgb turned', 1, 2, 3, [(90.0, (0, 0), 1.0), (45.0, (1, 0), 0.25)], -1),
    _case('S5 quarter turns', 5, 3, 1, [(90.0, (0, 0), 1.0), (-90.0, (0, 0), 1.0), (180.0, (0, 0), 1.0)], 255),
    _case('S5 rgb 45 zoom', 5, 2, 3, [(45.0, (0, 0), 4.0), (45.0, (1, -1), 0.25)], -1),
    _case('S7 random', 7, 3, 1, _rand(1, 3, 7), 0),
    _case('S7 rgb random border', 7, 3, 3, _rand(2, 3, 7), -1, 'identity'),
    _case('S7 pushed out', 7, 2, 1, [(30.0, (7, 0), 1.0), (-120.0, (-7, 7), 0.25)], -1),
    _case('S64 random', 64, 3, 1, _rand(3, 3, 64), -1),
    _case('S64 rgb turns and 45', 64, 3, 3, [(90.0, (3, -2), 1.0), (180.0, (0, 5), 4.0), (45.0, (0, 0), 0.25)], 255),
    _case('S64 pushed out', 64, 2, 1, [(10.0, (64, 64), 1.0), (-45.0, (0, -64), 4.0)], 0, 'identity'),
    _case('S64 N1 small angle', 64, 1, 1, [(0.01, (0, 0), 1.0)], -1),
    _case('S299 N3', 299, 3, 1, [(33.3, (12, -30), 0.8), (-147.0, (0, 0), 1.2), (90.0, (-29, 29), 1.0)], -1),
    # unrotated (angle exactly 0: Pillow takes its floating-point routine; exact properties instead)
    _case('S7 identity N2', 7, 2, 3, [(0.0, (0, 0), 1.0)] * 2, 0),
    _case('S64 integer shifts', 64, 3, 1, [(0.0, (5, -9), 1.0), (0.0, (-64, 0), 1.0), (0.0, (0, 63), 1.0)], -1),
    _case('S5 unrotated zoom', 5, 2, 1, [(0.0, (0, 0), 4.0), (0.0, (1, 1), 0.25)], 255),
]


def rotated(case):
    return all(p[0] != 0.0 for p in case['params'])


def source(case):
    """[N][S][S][C] u8: random, with a bright frame on image 0 so that the border fill differs from the interior's mean"""
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    src = rng.integers(0, 256, (case['N'], case['S'], case['S'], case['C']), dtype=np.uint8)
    if case['S'] >= 5:
        src[0, 0] = src[0, -1] = 250
        src[0, :, 0] = src[0, :, -1] = 247
    return src


def case_coefs(case):
    return [coefs(case['S'], *p) for p in case['params']]


def expected(case, src=None):
    src = source(case) if src is None else src
    return model_batch(src, case_coefs(case), case['fill'])


def shifted(src, tx, ty, fill):
    """an integer shift at scale 1: out[y][x] = src[y - ty][x - tx], fill elsewhere"""
    S, _, C = src.shape
    out = np.empty_like(src)
    out[:] = np.array(border_fill(src) if fill < 0 else [fill] * C, np.uint8)
    ys, xs = np.arange(S) - ty, np.arange(S) - tx
    oky, okx = (ys >= 0) & (ys < S), (xs >= 0) & (xs < S)
    out[np.ix_(oky, okx)] = src[np.ix_(ys[oky], xs[okx])]
    return out
