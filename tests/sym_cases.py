"""RUN --tta: a numpy model of ifcbk_batch_sym (csrc/batch_sym.hip) and the case table of its tests.  A plain helper module.

A batch is [N, S, S] (the u8 plane) or [N, S, S, 8] (the dense tensor; a pixel is the trailing axis and moves whole):
    HFLIP      x'[n][r][c] = x[n][r][S-1-c]
    VFLIP      x'[n][r][c] = x[n][S-1-r][c]
    TRANSPOSE  x'[n][r][c] = x[n][c][r]
The kernel permutes bytes, so every comparison is exact and the dense tensors are handled as their raw bits (int16 for bf16, int32 for
fp32): no NaN can spoil an equality.

WALKS are the op sequences of Engine.TTA_WALKS: every step reaches a view not seen before, and RESTORE names the one further op that
brings the batch back.  With T the transpose and H the horizontal flip, H after T is a quarter turn, an element of order 4, so the
alternating walk T, H, T, H, T, H, T passes through all eight symmetries of the square.

SIZES: 1 (no-op), 2, 3 (the smallest with a fixed middle), and the edges -1 / 0 / +1 of both tiles of the kernels -- 16 pixels for the
dense transpose, 64 for the u8 rectangles --, 129 (three rectangles a side, the last one pixel wide), and the two network inputs 224
and 299 (odd; S * S = 89,401 is a multiple of nothing)."""
import numpy as np

HFLIP, VFLIP, TRANSPOSE = 1, 2, 4
OPS = {'hflip': HFLIP, 'vflip': VFLIP, 'transpose': TRANSPOSE}
WALKS = {'flips': (HFLIP, VFLIP, HFLIP), 'all': (TRANSPOSE, HFLIP) * 3 + (TRANSPOSE,)}
RESTORE = {'flips': VFLIP, 'all': HFLIP}

SIZES = (1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 224, 299)
NS = (1, 3)
# kind -> (the library's kind code, numpy type of the raw bits, trailing shape of a pixel)
KINDS = {'u8': (2, np.uint8, ()), 'bf16': (0, np.int16, (8,)), 'f32': (1, np.int32, (8,))}


def apply(x, op):
    """one op on a batch [N, S, S, ...]; a view of x, not a copy"""
    if op == HFLIP:
        return x[:, :, ::-1]
    if op == VFLIP:
        return x[:, ::-1]
    if op == TRANSPOSE:
        return x.swapaxes(1, 2)
    raise ValueError('op %r is not exactly one of HFLIP, VFLIP, TRANSPOSE' % (op,))


def views(x, mode):
    """the batch as loaded and after every step of the walk: V = len(WALKS[mode]) + 1 contiguous arrays"""
    out = [np.ascontiguousarray(x)]
    for op in WALKS[mode]:
        out.append(np.ascontiguousarray(apply(out[-1], op)))
    return out


def batch(kind, N, S, seed=0):
    """random raw bits of a batch of the kind"""
    _, dt, tail = KINDS[kind]
    rng = np.random.default_rng(1000 * seed + 10 * S + N)
    info = np.iinfo(dt)
    return rng.integers(info.min, int(info.max) + 1, (N, S, S) + tail, dtype=dt)


def symmetrised(x):
    """a batch every symmetry of the square leaves alone: pixel by pixel the maximum over the eight views"""
    out = x
    for v in views(x, 'all')[1:]:
        out = np.maximum(out, v)
    return np.ascontiguousarray(out)
