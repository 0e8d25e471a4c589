"""The numpy twin of TRAIN --jitter (csrc/roi_jitter.hip) and the case table of tests/test_gpu_roi_jitter.py; tests/test_jitter_cpu.py proves
the twin equal to the installed Pillow's ImageEnhance chain.  Everything here runs on the CPU.

Both enhancements are Image.blend(degenerate, img, f), which for u8 data is the 256-entry table
    t      = fl32( fl32(m) + fl32( f * fl32(v - m) ) )          two float32 roundings, not a fused multiply-add
    lut[v] = 0 if t <= 0, 255 if t >= 255, else trunc(t)
with m = 0 for brightness and, for contrast, m = (2 sum L + n) // (2 n) over the L plane of the image AFTER the brightness step
(one channel: L = the pixel; three: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16).  A factor that is negative or not finite
counts as 1."""
import zlib

import numpy as np


def sane(f):
    """the factor as the kernel reads it: float32; negative or not finite -> 1"""
    if f is None:
        return np.float32(1)
    f = np.float32(f)
    return f if np.isfinite(f) and f >= 0 else np.float32(1)


def lut(f, m):
    """[256] u8: the blend table for factor f around level m"""
    f = np.float32(f)
    v = np.arange(256, dtype=np.int64)
    prod = (f * (v - m).astype(np.float32)).astype(np.float32)          # numpy rounds each float32 operation on its own
    t = (np.float32(m) + prod).astype(np.float32)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(np.clip(t, 0, 255)))).astype(np.uint8)
    return out


def luma(a):
    """the L plane of a [h][w] or [h][w][3] u8 array (Pillow's convert('L'))"""
    if a.ndim == 2:
        return a.astype(np.int64)
    a = a.astype(np.int64)
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16


def mean_level(a):
    lp = luma(a)
    return int((2 * int(lp.sum()) + lp.size) // (2 * lp.size))


def jitter(a, fb=None, fc=None):
    """the image the resize sees: brightness fb (None: skipped), then contrast fc (None: skipped) around the mean taken after brightness"""
    a = np.asarray(a, np.uint8)
    if fb is not None:
        a = lut(sane(fb), 0)[a]
    if fc is not None:
        a = lut(sane(fc), mean_level(a))[a]
    return a


def pillow_jitter(a, fb=None, fc=None):
    """the same through the installed Pillow (finite factors >= 0 only)"""
    from PIL import Image, ImageEnhance
    img = Image.fromarray(np.asarray(a, np.uint8))
    if fb is not None:
        img = ImageEnhance.Brightness(img).enhance(float(np.float32(fb)))
    if fc is not None:
        img = ImageEnhance.Contrast(img).enhance(float(np.float32(fc)))
    return np.asarray(img)


# ---------------------------------------------------------------------------------------------------------------- the GPU case table
# the kernel cuts a ROI into the 16-byte units of its absolute address, 4 units per thread, 256 threads: 16384 bytes per block
CHUNK = 16384
FACTORS = [0.0, 1.0, 0.37, 1.63, 2.0]                  # 0 and 2: both clip sides; 1: identity
NAN, INF = float('nan'), float('inf')


def _case(name, shapes, cin=1, fb='cycle', fc='cycle'):
    n = len(shapes)
    cyc = lambda k: [FACTORS[(i + k) % len(FACTORS)] for i in range(n)]
    return dict(name=name, shapes=shapes, cin=cin, fb=cyc(2) if fb == 'cycle' else fb, fc=cyc(3) if fc == 'cycle' else fc)


CASES = [
    _case('1x1', [(1, 1)] * 5),
    _case('1x17 head meets tail', [(1, 17)] * 5),                                      # with 32 guard bytes in front: no aligned body at most offsets
    _case('odd starts', [(3, 5), (7, 9), (3, 5), (7, 9), (2, 8), (1, 16), (4, 4), (1, 15), (5, 7), (1, 33)]),
    _case('several chunks', [(300, 220), (3, 5), (129, 127), (128, 128), (1, 16385)]),   # 66000 bytes: 5 blocks; 16384: exactly one chunk
    _case('max far beyond the smallest', [(1, 1), (400, 350), (2, 3), (1, 1), (20, 20)]),
    _case('rgb', [(5, 7), (41, 67), (1, 1), (100, 70), (3, 5)], cin=3),                  # 100 x 70 x 3 = 21000 bytes: a pixel straddles the chunks
    _case('not finite or negative', [(9, 11), (30, 40), (5, 5), (17, 3), (8, 8), (6, 6)], fb=[NAN, 1.5, -INF, -0.5, INF, 0.5],
          fc=[0.5, NAN, INF, 1.7, -1.0, -INF]),
    _case('rgb not finite', [(6, 5), (12, 9), (4, 4)], cin=3, fb=[NAN, 0.4, 1.9], fc=[1.8, INF, -2.0]),
]
MODES = ('brightness', 'contrast', 'both')
GUARD = 32


def pixels(case):
    """random u8 ROIs; the last all 255, the one before it half 0"""
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    shp = (lambda h, w: (h, w)) if case['cin'] == 1 else (lambda h, w: (h, w, 3))
    rois = [rng.integers(0, 256, shp(h, w), dtype=np.uint8) for h, w in case['shapes']]
    if len(rois) > 4:
        rois[-1][:] = 255
        rois[-2][:rois[-2].shape[0] // 2 + 1] = 0
    return rois


def factors(case, mode):
    """(fb list or None, fc list or None) of the mode"""
    return (case['fb'] if mode != 'contrast' else None), (case['fc'] if mode != 'brightness' else None)


def expected(case, rois, mode):
    fb, fc = factors(case, mode)
    return [jitter(r, None if fb is None else fb[i], None if fc is None else fc[i]) for i, r in enumerate(rois)]


def layout(rois, guard=GUARD, poison=0xA5, lead=0):
    """(blob, offs): ``lead`` + ``guard`` poison bytes in front of the first ROI, ``guard`` between ROIs and behind the last"""
    offs, pos = [], lead + guard
    for r in rois:
        offs.append(pos)
        pos += r.size + guard
    blob = np.full(pos, poison, np.uint8)
    for o, r in zip(offs, rois):
        blob[o:o + r.size] = r.reshape(-1)
    return blob, offs
