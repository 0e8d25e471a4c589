"""TRAIN --resident: the numpy model of ifcbk_roi_gather, the case table of tests/test_gpu_roi_gather.py, and the tiny PNG trees the CPU,
model and command-line tests train on."""
import os

import numpy as np

MAX_N, CHUNK = 4096, 16384            # IFCBK_ROI_GATHER_MAX_N / IFCBK_ROI_GATHER_CHUNK (test_resident_cpu.py holds them to the header)


def gather(blob, offs, hs, ws, idx, ch):
    """what ifcbk_roi_gather leaves: (pixels, offs[n + 1], hs[n], ws[n]) of the batch ``idx`` cut from a ragged u8 set"""
    idx = np.asarray(idx, np.int64)
    h, w = hs[idx].astype(np.int32), ws[idx].astype(np.int32)
    size = np.where((h > 0) & (w > 0), h.astype(np.int64) * w * ch, 0)
    d = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(size, out=d[1:])
    parts = [blob[int(offs[i]):int(offs[i]) + int(s)] for i, s in zip(idx, size)]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), d, h, w


def layout(shapes, ch=1, leads=None, seed=0, poison=0xEE):
    """a source set: ROIs of ``shapes`` with random bytes, ROI i behind ``leads[i]`` pad bytes (default: i % 5) -> blob, offs, hs, ws"""
    rng = np.random.default_rng(seed)
    parts, offs, pos = [], [], 0
    for i, (h, w) in enumerate(shapes):
        lead = (i % 5) if leads is None else int(leads[i])
        parts.append(np.full(lead, poison, np.uint8))
        pos += lead
        offs.append(pos)
        n = max(h, 0) * max(w, 0) * ch
        parts.append(rng.integers(0, 256, n, dtype=np.uint8))
        pos += n
    parts.append(np.full(19, poison, np.uint8))
    return (np.concatenate(parts), np.array(offs, np.int64), np.array([s[0] for s in shapes], np.int32),
            np.array([s[1] for s in shapes], np.int32))


def _case(name, shapes, idx, ch=1, extra=0, leads=None):
    return dict(name=name, shapes=list(shapes), idx=list(idx), ch=ch, extra=extra, leads=leads)


def _tiny(n, seed):
    """n indices, with repeats, into 37 ROIs of one to six bytes"""
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(1, 3)), int(rng.integers(1, 4))) for _ in range(37)]
    return shapes, [int(v) for v in rng.integers(0, 37, n)]


MIXED = [(1, 1), (3, 5), (1000, 1200), (1, 1), (3, 5), (7, 1)]
EDGES = [(1, CHUNK - 1), (1, CHUNK), (1, CHUNK + 1), (1, 3), (2, CHUNK // 2), (1, 2 * CHUNK + 1)]
CASES = [
    _case('n 1', [(5, 7), (9, 4)], [1]),
    _case('one 1x1 ROI', [(1, 1)], [0]),
    _case('the same index three times', [(5, 7), (9, 4), (2, 31)], [2, 0, 2, 1, 2]),
    _case('an empty entry between two', [(5, 7), (0, 4), (3, 3), (4, -1)], [0, 1, 2, 3, 1, 0]),
    _case('chunk - 1, chunk, chunk + 1', EDGES, [0, 1, 2, 3, 4, 5]),
    _case('chunk edges, another order', EDGES, [3, 2, 1, 0, 3, 5, 4, 1]),
    _case('one large ROI among tiny ones', MIXED, [0, 1, 2, 3, 4, 5, 0]),
    _case('large first and last', MIXED, [2, 1, 0, 2]),
    _case('three channels', [(5, 7), (1, 1), (33, 17), (2, 2731), (80, 90)], [4, 1, 0, 3, 2, 1, 3], ch=3),
    _case('capacity beyond the total', MIXED, [1, 2, 0, 4], extra=3 * CHUNK + 5),
    _case('capacity beyond the total, tiny batch', [(1, 1), (2, 3)], [1, 0], extra=2 * CHUNK),
] + [_case('scan n %d' % n, *_tiny(n, n)) for n in (64, 65, 256, 257, 1025, MAX_N)]


def alignment_case(d):
    """ROIs of h = 1, w = 1..33, one at every source offset mod 16 (528 of them, behind fillers of 1..16 bytes), each put at destination
    offset d mod 16 by the filler in front of it: over d = 0..15 every (source mod 16, destination mod 16, w) occurs once"""
    shapes, leads = [(1, f) for f in range(1, 17)], [0] * 16
    pos = sum(range(1, 17))
    for s in range(16):
        for w in range(1, 34):
            lead = (s - pos) % 16
            leads.append(lead)
            shapes.append((1, w))
            pos += lead + w
    idx, cur = [], 0
    for k in range(16, len(shapes)):
        f = (d - cur) % 16 or 16
        idx += [f - 1, k]
        cur += f + shapes[k][1]
    return _case('alignment sweep, destination mod 16 = %d' % d, shapes, idx, leads=leads)


# ------------------------------------------------------------------------------------------------------------------------ PNG trees
SIZES = [(1, 1), (1, 37), (41, 1), (17, 33), (64, 64), (5, 129), (97, 3), (31, 47)]


def write_tree(root, kind='grey', classes=('ant', 'bee', 'cat'), per_class=8, seed=5):
    """``per_class`` Pillow-written PNGs of deliberately odd sizes in each class folder.  kind: 'grey' (mode L), 'rgb', or 'mixed' (every
    third file RGB).  8 files per class split 80:20 into 6 + 2, so three classes train on 18 and validate on 6."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    k = 0
    for c, cls in enumerate(classes):
        os.makedirs(os.path.join(root, cls), exist_ok=True)
        for i in range(per_class):
            h, w = SIZES[(i + 3 * c) % len(SIZES)]
            rgb = kind == 'rgb' or (kind == 'mixed' and k % 3 == 0)
            a = np.clip(rng.normal(80 + 50 * c, 40, (h, w, 3) if rgb else (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'RGB' if rgb else 'L').save(os.path.join(root, cls, 'roi_%s_%02d.png' % (cls, i)))
            k += 1
    return root
