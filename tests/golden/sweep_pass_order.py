"""Where does the installed Pillow leave the horizontal-first order of the two resize passes?  (run in the build container; PIL is measured)

  python tests/golden/sweep_pass_order.py

For every grid point (S, h, w) a random u8 'L' image is resized by Pillow and by both pass orders of the numpy restatement
(oracle/pil_resize.py, order='hv' and order='vh'); the 8-bit intermediate makes the order visible (differences of one level).
Grid, for S in 224, 299: w = 1..33 against h = 1, 17, 33, .. 4S, every multiple of S/2 up to 4S +-2, S-3..S+3 and 100w-6..100w+6
(the boundary of the rule below), 100w+50, 200w+1, 4S, 3400; and the transposes (h, w swapped) of the first family.

Outcome (pass_order_sweep.json): for every w the smallest h at which Pillow's result is the vertical-first one, the counts, and the
rule that fits EVERY point: vertical pass first  <=>  h > 100 * w  and  h > S  (the image is more than 100 times as tall as wide and
shrinks in height) -- a branch of Image.resize itself in the installed version; nowhere did Pillow differ from both orders.
tests/test_roi_paths_cpu.py re-checks the committed boundary against oracle.pil_resize.vertical_first and against Pillow."""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np
from PIL import Image
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.pil_resize import resize_bilinear_u8  # noqa: E402


def one(t):
    S, h, w = t
    a = np.random.default_rng(h * 4099 + w * 7 + S).integers(0, 256, (h, w), dtype=np.uint8)
    p = np.asarray(Image.fromarray(a, 'L').resize((S, S), Image.BILINEAR))
    eh = bool((p == resize_bilinear_u8(a, S, S, 'hv')).all())
    ev = bool((p == resize_bilinear_u8(a, S, S, 'vh')).all())
    return S, h, w, 'B' if eh and ev else 'H' if eh else 'V' if ev else 'N'


def grid():
    pts = set()
    for S in (224, 299):
        hs = set(range(1, 4 * S + 1, 16)) | {k * S // 2 + d for k in range(1, 9) for d in (-2, -1, 0, 1, 2)}
        for w in range(1, 34):
            for h in hs:
                pts.add((S, h, w))
                pts.add((S, w, h))
            for h in set(range(100 * w - 6, 100 * w + 7)) | set(range(S - 3, S + 4)) | {4 * S, 3400, 100 * w + 50, 200 * w + 1}:
                pts.add((S, h, w))
    return sorted(pts)


def main():
    pts = grid()
    with Pool(min(8, os.cpu_count())) as p:
        res = p.map(one, pts, chunksize=64)
    counts = {k: sum(r[3] == k for r in res) for k in 'HVBN'}
    rule_ok = all(r[3] == 'B' or (r[3] == 'V') == (r[1] > 100 * r[2] and r[1] > r[0]) for r in res)
    boundary = []
    for S in (224, 299):
        for w in range(1, 34):
            col = sorted((r[1], r[3]) for r in res if r[0] == S and r[2] == w)
            v = [h for h, c in col if c == 'V']
            if v:
                below = max(h for h, c in col if h < min(v))
                assert all(c != 'H' for h, c in col if h > min(v)), (S, w)
                boundary.append(dict(S=S, w=w, last_horizontal_first=below, first_vertical_first=min(v)))
    out = dict(pillow=PIL.__version__, points=len(res), counts=counts, rule='h > 100 * w and h > S', rule_fits_every_point=rule_ok,
               boundary=boundary)
    json.dump(out, open(os.path.join(HERE, 'pass_order_sweep.json'), 'w'), indent=1)
    print(len(res), counts, 'rule fits every point:', rule_ok)


if __name__ == '__main__':
    main()
