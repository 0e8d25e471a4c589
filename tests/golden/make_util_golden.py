"""Generates tests/golden/util_golden.json by running the REFERENCE's own neuston_util.py (make_dataset_config,
make_class_config, main -> calc_img_norm) in this container, with stub modules for its missing third-party imports
(torchvision, ifcb) and the real torch DataLoader.  Only inputs and outputs are stored; the image tree is rebuilt from a
seed by ``make_image_tree`` (the tests call it too), so no image is committed.

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_util_golden.py

Nothing outside this repository is touched at import time: the reference is imported inside main() only.
"""
import argparse
import contextlib
import io
import json
import math
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = '/root/reference'

# class -> image count: --class-min 2 drops Ceratium; the total (203 kept) gives > 100 batches at batch size 2
TREE = {'Akashiwo': 40, 'Ceratium': 1, 'Ditylum': 3, 'detritus': 160}
TREE_SEED = 20261016


def make_image_tree(root):
    """the CALC_IMG_NORM tree: PNGs of 9..400 px on each axis (below and above 224 / 299), about 10 % RGB, the rest grey"""
    from PIL import Image
    rng = np.random.default_rng(TREE_SEED)
    for cls, n in TREE.items():
        os.makedirs(os.path.join(root, cls))
        for i in range(n):
            h, w = (int(v) for v in rng.integers(9, 401, 2))
            rgb = rng.random() < 0.1
            base = rng.integers(0, 256)
            img = rng.integers(0, 256, (h, w, 3) if rgb else (h, w)).astype(np.int64)
            img = ((img + base) // 2).astype(np.uint8)          # per-image brightness offset: batches differ
            Image.fromarray(img, 'RGB' if rgb else 'L').save(os.path.join(root, cls, 'IFCB_%s_%03d.png' % (cls[:3], i)))
        open(os.path.join(root, cls, 'notes.txt'), 'w').close()        # non-image file must be ignored


# --class-config csv of case C: merges Ditylum into Akashiwo, skips Ceratium, names a class the tree lacks
CLASS_CONFIG = 'class,cfg\nAkashiwo,1\nCeratium,0\nDitylum,Akashiwo\ndetritus,1\nmissing_cls,1\n'

# CALC_IMG_NORM cases: (name, resize, batch size, class-min, class-max, class-config, python random seed before the call)
CASES = [
    ('A', 299, 64, 2, None, False, 1),
    ('B', 224, 108, 2, 30, False, 2),
    ('C', 299, 108, 2, None, True, 3),
    ('D', 299, 2, 2, None, False, 4),
]

# MAKE_* trees (empty class folders + a stray file; a comma in one name: csv quoting) and calls, run from the tree root with relative paths
MAKE_TREE = {'dsA': ['Akashiwo', 'Ceratium', 'detritus'], 'dsB': ['Ceratium', 'Ditylum', 'Euglena'], 'dsC': ['Akashiwo', 'zoo, misc']}
MAKE_CSV = 'classes.csv'
MAKE_CSV_TEXT = ',2:dsA,dsB\nAkashiwo,1,0\nCeratium,0,0\nDitylum,0,1\nEuglena,0,0\ndetritus,1,1\n'
MAKE_CALLS = [
    ['MAKE_DATASET_CONFIG', '2:dsA', 'dsB', '--', '-1:dsC'],            # ('--': argparse would read -1:dsC as an option)
    ['MAKE_DATASET_CONFIG', 'dsA', 'dsB'],
    ['MAKE_CLASS_CONFIG', 'dsB'],
    ['MAKE_CLASS_CONFIG', MAKE_CSV],
]


def make_config_tree(root):
    for ds, classes in MAKE_TREE.items():
        for cls in classes:
            os.makedirs(os.path.join(root, ds, cls))
        open(os.path.join(root, ds, 'readme.txt'), 'w').close()
    with open(os.path.join(root, MAKE_CSV), 'w') as f:
        f.write(MAKE_CSV_TEXT)


def case_args(case, root):
    name, resize, batch, cmin, cmax, use_csv, _ = case
    return argparse.Namespace(cmd='CALC_IMG_NORM', SRC=root, resize=resize, batch_size=batch, class_min=cmin, class_max=cmax,
                              class_config=[os.path.join(root, 'cfg.csv'), 'cfg'] if use_csv else None)


def exact_stats(u8):
    """fp64 mean / population std on the ToTensor scale of a u8 batch [N, 3, H, W], from exact integer sums"""
    v = u8.astype(np.int64)
    n = v.shape[0] * v.shape[2] * v.shape[3]
    s = v.sum(axis=(0, 2, 3))
    s2 = (v * v).sum(axis=(0, 2, 3))
    mean = [int(a) / (255 * n) for a in s]
    std = [math.sqrt(n * int(b) - int(a) * int(a)) / (255 * n) for a, b in zip(s, s2)]
    return mean, std


def stub_modules():
    import torch
    from PIL import Image
    tv = types.ModuleType('torchvision')
    tr = types.ModuleType('torchvision.transforms')
    ds = types.ModuleType('torchvision.datasets')
    fo = types.ModuleType('torchvision.datasets.folder')
    fo.IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')

    def default_loader(path):
        with open(path, 'rb') as f:
            return Image.open(f).convert('RGB')
    fo.default_loader = default_loader
    ds.folder = fo

    class ImageFolder:
        pass
    ds.ImageFolder = ImageFolder

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    class Resize:                                   # torchvision 0.8 F.resize on a PIL image, size [S, S]
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            return img.resize((self.size[1], self.size[0]), Image.BILINEAR)

    class ToTensor:
        def __call__(self, img):
            return torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1).float().div(255)
    tr.Compose, tr.Resize, tr.ToTensor = Compose, Resize, ToTensor
    tv.transforms, tv.datasets = tr, ds
    ifcb = types.ModuleType('ifcb')
    data = types.ModuleType('ifcb.data')
    adc = types.ModuleType('ifcb.data.adc')
    adc.SCHEMA_VERSION_1 = 'v1'
    st = types.ModuleType('ifcb.data.stitching')
    st.InfilledImages = object
    for name, m in (('torchvision', tv), ('torchvision.transforms', tr), ('torchvision.datasets', ds),
                    ('torchvision.datasets.folder', fo), ('ifcb', ifcb), ('ifcb.data', data), ('ifcb.data.adc', adc),
                    ('ifcb.data.stitching', st)):
        sys.modules[name] = m


class _RecordingNumpy:
    """numpy for the reference module, recording each batch's np.mean / np.std over axis (0, 2, 3) and its exact statistics"""

    def __init__(self):
        self.batches = []
        self.result = None

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, axis=None, **kw):
        r = np.mean(a, axis=axis, **kw)
        if axis == (0, 2, 3):
            u8 = np.rint(np.asarray(a, np.float64) * 255).astype(np.uint8)
            assert np.array_equal(u8.astype(np.float32) / np.float32(255), a)
            em, es = exact_stats(u8)
            self.batches.append(dict(n=int(a.shape[0]), pop_mean=[float(v) for v in r], exact_mean=em, exact_std=es))
        return r

    def std(self, a, axis=None, **kw):
        r = np.std(a, axis=axis, **kw)
        if axis == (0, 2, 3):
            self.batches[-1]['pop_std0'] = [float(v) for v in r]
        return r


def main():
    stub_modules()
    sys.path.insert(0, REFERENCE)
    import neuston_util as nu                                           # the reference itself
    calc_img_norm = nu.calc_img_norm

    def recording_calc_img_norm(args):
        nu.np.result = calc_img_norm(args)
        return nu.np.result
    nu.calc_img_norm = recording_calc_img_norm
    out = {'tree': TREE, 'tree_seed': TREE_SEED, 'class_config': CLASS_CONFIG, 'cases': [], 'make': [],
           'make_tree': MAKE_TREE, 'make_csv': MAKE_CSV_TEXT}
    worst = 0.0
    with tempfile.TemporaryDirectory() as root:
        make_image_tree(root)
        with open(os.path.join(root, 'cfg.csv'), 'w') as f:
            f.write(CLASS_CONFIG)
        for case in CASES:
            args = case_args(case, root)
            rec = _RecordingNumpy()
            nu.np = rec
            random.seed(case[6])
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                nu.main(args)
            nu.np = np
            final_mean, final_std = rec.result
            for b in rec.batches:
                for got, exact in (('pop_mean', 'exact_mean'), ('pop_std0', 'exact_std')):
                    worst = max([worst] + [abs(x - y) for x, y in zip(b[got], b[exact])])
            out['cases'].append(dict(name=case[0], resize=case[1], batch_size=case[2], class_min=case[3], class_max=case[4],
                                     class_config=case[5], random_seed=case[6], batches=rec.batches,
                                     mean=[float(v) for v in final_mean], std=[float(v) for v in final_std],
                                     stdout=buf.getvalue().replace(root, '{ROOT}')))
            print('case %s: %d batches, MEAN=%s STD=%s' % (case[0], len(rec.batches), final_mean, final_std))
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as root:
        make_config_tree(root)
        os.chdir(root)
        try:
            for call in MAKE_CALLS:
                for outfile in (None, 'out.csv'):
                    paths = [a for a in call[1:] if a != '--']
                    args = argparse.Namespace(cmd=call[0], dataset=paths if call[0] == 'MAKE_DATASET_CONFIG' else paths[0],
                                              outfile=outfile)
                    nu.args = args                              # the reference's write_csv reads the global args.outfile
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        nu.main(args)
                    text = open(outfile, newline='').read() if outfile else buf.getvalue()
                    out['make'].append(dict(argv=call[:1] + (['-o', outfile] if outfile else []) + call[1:], outfile=outfile, output=text))
                    if outfile:
                        os.remove(outfile)
        finally:
            os.chdir(here)
    out['max_f32_gap'] = worst
    json.dump(out, open(os.path.join(HERE, 'util_golden.json'), 'w'), indent=1, sort_keys=True)
    print('written %d CALC_IMG_NORM cases, %d MAKE outputs; largest |reference float32 - exact| per-batch gap: %.3e'
          % (len(out['cases']), len(out['make']), worst))


if __name__ == '__main__':
    main()
