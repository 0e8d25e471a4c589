"""The per-item random draws of TRAIN's augmentations as both feeds hand them to the engine (no GPU needed).

  python tests/golden/make_roi_draws.py          # rewrites roi_draws.json

roi_draws.json : setting name -> {'draw_items': [...], 'collate': [...]}, three consecutive batches (N = 5, 5, 3) each.

'draw_items' is what ``neuston_data.draw_items`` returns (the TRAIN --resident feed); 'collate' holds the same entries of the batches
``collate_rois`` builds from ``NeustonDataset.__getitem__`` on a 13-image dataset of tiny grey arrays (the loader feed).  Each feed starts
from ``random.seed(7)`` and a fresh ``RoiTransform(..., seed=7, rank=0)``.  Per batch: ``flips`` as a list, ``turn`` when present, and
``brightness`` / ``contrast`` / ``blur`` when present as lists of ``float.hex()`` strings; an entry a batch does not carry is absent.
Regenerate only for a change that is meant to alter a random stream or a batch's entries, and say so in its description.
"""
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, 'roi_draws.json')

BATCHES = (5, 5, 3)

# name -> RoiTransform keyword arguments (None: no transform at all)
SETTINGS = {
    'none': None,
    'flip xy': dict(vflip=True, hflip=True),
    'rot90': dict(rot90=True),
    'flip xy rot90': dict(vflip=True, hflip=True, rot90=True),
    'jitter 0.4': dict(jitter='0.4'),
    'jitter 0,0.3': dict(jitter='0,0.3'),
    'jitter 0.4,0.3': dict(jitter='0.4,0.3'),
    'blur 2.0 prob 0.5': dict(blur=2.0, blur_prob=0.5),
    'blur 2.0 prob 0': dict(blur=2.0, blur_prob=0.0),
    'flip xy rot90 jitter 0.4,0.3 blur 2.0 prob 0.5': dict(vflip=True, hflip=True, rot90=True, jitter='0.4,0.3', blur=2.0, blur_prob=0.5),
}


def _transform(kw):
    from ifcb_classifier_amd.neuston_data import RoiTransform
    return None if kw is None else RoiTransform(224, seed=7, rank=0, **kw)


def _entries(batch):
    out = dict(flips=batch['flips'].tolist())
    if 'turn' in batch:
        out['turn'] = batch['turn']
    for k in ('brightness', 'contrast', 'blur'):
        if k in batch:
            out[k] = [float(v).hex() for v in batch[k].tolist()]
    return out


def write_images(folder):
    """13 tiny grey PNGs in one class folder"""
    import numpy as np
    from PIL import Image
    os.makedirs(os.path.join(folder, 'a'))
    for i in range(sum(BATCHES)):
        Image.fromarray(np.full((3 + i % 4, 5 + i % 3), 7 * i, np.uint8)).save(os.path.join(folder, 'a', '%02d.png' % i))


def record(name, folder):
    """both feeds of one setting; ``folder``: where ``write_images`` put the dataset"""
    from ifcb_classifier_amd.neuston_data import NeustonDataset, collate_rois, draw_items
    kw = SETTINGS[name]
    random.seed(7)
    t = _transform(kw)
    drawn = [_entries(draw_items(t, n)) for n in BATCHES]
    random.seed(7)
    ds = NeustonDataset(folder, transforms=_transform(kw))
    collated, i = [], 0
    for n in BATCHES:
        collated.append(_entries(collate_rois([ds[k] for k in range(i, i + n)])[0]))
        i += n
    return dict(draw_items=drawn, collate=collated)


def record_all():
    with tempfile.TemporaryDirectory() as tmp:
        write_images(tmp)
        return {name: record(name, tmp) for name in SETTINGS}


if __name__ == '__main__':
    out = record_all()
    with open(GOLDEN, 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('\n'.join('%s %s' % (k, json.dumps(v['draw_items'][2])) for k, v in out.items()))
