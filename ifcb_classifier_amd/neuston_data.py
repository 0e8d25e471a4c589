"""Host-side twin of ``/root/reference/neuston_data.py``: dataset selection / splitting and the per-item
input contract, re-cut for the MI355X path.

What changes versus the reference: items are NOT resized/normalised on the CPU.  ``__getitem__`` returns the
decoded u8 image (HxW for grayscale ROIs, HxWx3 otherwise) plus a per-item flip code; ``collate_rois`` packs a
batch into one ragged u8 blob + offset table (pinned), and the resize / ToTensor / Normalize chain of
``get_trainval_transforms`` (:342-371) runs on the GPU in ``ifcbk_roi_preprocess`` (bit-exact to PIL).
What does not change: class-folder scanning, class-min/max, class-config CSV, dataset-config CSV,
``split`` (incl. its re-seeding quirk), ``parse_imgnorm``, resize = 299 iff MODEL == 'inception_v3'.
"""
import os
import random

import numpy as np
import torch
from torch.utils.data import get_worker_info
from torch.utils.data.dataset import Dataset

# torchvision.datasets.folder.IMG_EXTENSIONS (the reference filters files with it, neuston_data.py:69)
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


def default_loader(path):
    """[TV] datasets.folder.default_loader = PIL open -> convert('RGB').  A grayscale file stays 2-D here
    (L -> RGB only replicates the channel; the GPU kernel replicates instead) -- same pixels, 1/3 the bytes."""
    from PIL import Image
    with open(path, 'rb') as f:
        img = Image.open(f)
        if img.mode == 'L':
            return np.asarray(img).copy()
        return np.asarray(img.convert('RGB')).copy()


class RoiTransform:
    """What ``transforms.Compose([flips] + [Resize, ToTensor, Normalize?])`` means on the GPU path."""

    def __init__(self, resize, img_norm=None, vflip=False, hflip=False, rot90=False, pad=None, jitter=None, mix=None, blur=None, blur_prob=None,
                 seed=0, rank=0):
        self.resize = resize
        # --blur / --blur-prob: None, or SIGMA_MAX of the Gaussian defocus and the probability that an image is blurred at all
        self.blur, self.blur_prob = parse_blur(blur), parse_blur_prob(blur_prob)
        self._blur_seed, self._blur_rng, self._blur_worker = (int(seed or 0) & 0xffffffffffffffff, int(rank)), None, None
        self.mix = mix                    # --mixup / --cutmix: None, or the BatchMix that draws per batch (the training transform only)
        self.jitter = parse_jitter(jitter)   # --jitter: None, or [B, C] = the brightness / contrast ranges of ColorJitter (not both 0)
        self.pad = parse_pad(pad)         # --pad: None = squash to resize x resize, 'border' / 0..255 = keep the aspect ratio, fill the rest
        self.img_norm = img_norm          # (mean[3], std[3]) or None
        self.vflip, self.hflip = vflip, hflip
        self.rot90 = bool(rot90)          # --rot90: k counter-clockwise quarter turns after the flips, k uniform in {0, 1, 2, 3}

    def flip_code(self):
        """bit0 = vertical flip ('x'), bit1 = horizontal flip ('y'); each with p = 0.5 (RandomVertical/HorizontalFlip).
        With rot90 the k quarter turns that follow the flips are folded in: bit2 = transpose (``fold_turns``).  The third random
        number is drawn only with rot90 set, so the random stream of a run without it is unchanged."""
        code = 0
        if self.vflip and random.random() < 0.5:
            code |= 1
        if self.hflip and random.random() < 0.5:
            code |= 2
        if self.rot90:
            code = fold_turns(code & 1, code >> 1, random.randrange(4))
        return code

    def jitter_factors(self):
        """(fb, fc) of ``ColorJitter(brightness=B, contrast=C)``: each uniform in [max(0, 1 - range), 1 + range], rounded to float32;
        None for a zero range, which draws nothing.  Called after ``flip_code``: brightness first, then contrast.  The order of the
        two enhancements is always brightness, contrast (torchvision permutes them at random)."""
        if self.jitter is None:
            return None, None
        return tuple(float(np.float32(random.uniform(max(0.0, 1.0 - r), 1.0 + r))) if r > 0 else None for r in self.jitter)

    def blur_sigma(self):
        """the sigma of this item's Gaussian blur, a float32 value: uniform in [0.1, SIGMA_MAX] (torchvision's ``GaussianBlur(k,
        sigma=(0.1, SIGMA_MAX))``) with probability ``blur_prob``, else 0.0 = not blurred.  Two numbers per item -- blurred at all, then
        sigma -- whatever the first says, from a generator of this object's own, seeded from (seed, rank): neither ``random`` nor the
        global numpy / torch streams are touched, so no flip, turn or jitter draw moves.  In a DataLoader worker the generator is seeded
        from the worker's seed as well, once per worker: the forked copies of one state would repeat each other's draws."""
        if self.blur is None:
            return 0.0
        info = get_worker_info()
        if self._blur_rng is None or (info is not None and self._blur_worker != (info.id, info.seed)):
            key = [0x626c7572, self._blur_seed[0], self._blur_seed[1]]
            if info is not None:
                key.append(int(info.seed) & 0xffffffffffffffff)
                self._blur_worker = (info.id, info.seed)
            self._blur_rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(key)))
        u, v = self._blur_rng.random(2)
        if not u < self.blur_prob:
            return 0.0
        return float(np.float32(BLUR_SIGMA_MIN + v * (self.blur - BLUR_SIGMA_MIN)))

    def draw_item(self):
        """one item's random draws, in the order every feed makes them -- ``flip_code()``, then ``jitter_factors()`` with jitter set, then
        ``blur_sigma()`` with blur set -- as the tail of its tuple behind the image: (flip[, turn[, fb, fc[, sigma]]]).  turn: this
        transform turns, whatever the draw was; fb, fc: the brightness and contrast factors, None without jitter or for a zero range;
        sigma: 0.0 = not blurred.  A later field brings the earlier ones along; ``collate_draws`` reads them."""
        tail = (self.flip_code(), self.rot90)
        if self.blur is not None:
            return tail + self.jitter_factors() + (self.blur_sigma(),)      # (without jitter the factors are (None, None), nothing drawn)
        if self.jitter is not None:
            return tail + self.jitter_factors()
        return tail if self.rot90 else tail[:1]


BLUR_SIGMA_MIN = 0.1          # torchvision's default low end of GaussianBlur's sigma range
BLUR_SIGMA_LIMIT = 4.0        # the largest SIGMA_MAX: radius ceil(3 * 4) = 12, the kernel's largest window


def _floats(values, expected, ok=None, wrong=None):
    """the body the option parsers share: refuse a bool (ValueError ``expected``), ``float()`` every value, then hold each one to
    ``ok`` (ValueError ``wrong``) -> the list of floats"""
    if any(isinstance(v, bool) for v in values):
        raise ValueError(expected)
    out = [float(v) for v in values]                                    # (float('a') raises ValueError too)
    if ok is not None and not all(ok(v) for v in out):                  # (nan fails every comparison)
        raise ValueError(wrong)
    return out


def _arg_type(parse, message):
    """argparse ``type=`` of an option (neuston_net TRAIN, neuston_util CALC_IMG_NORM): ``parse``, its ValueError reworded as ``message``"""
    def arg(text):
        import argparse
        try:
            return parse(text)
        except ValueError:
            raise argparse.ArgumentTypeError(message % text)
    return arg


def _unit(v):
    return 0.0 <= v <= 1.0


def _finite(v):
    return 0.0 <= v < float('inf')


def parse_blur(value):
    """``--blur SIGMA_MAX`` / a checkpoint's ``blur``: None (unset) or a finite float in (0.1, 4]"""
    if value is None:
        return None
    return _floats([value], 'blur: SIGMA_MAX expected, got %r' % (value,), lambda v: BLUR_SIGMA_MIN < v <= BLUR_SIGMA_LIMIT,
                   'blur: SIGMA_MAX must be a float in (0.1, 4], got %r' % (value,))[0]


def parse_blur_prob(value):
    """``--blur-prob P`` / a checkpoint's ``blur_prob``: None -> 0.5, else a float in [0, 1]"""
    if value is None:
        return 0.5
    return _floats([value], 'blur-prob: P expected, got %r' % (value,), _unit, 'blur-prob: P must be in [0, 1], got %r' % (value,))[0]


def blur_radius(sigma_max):
    """the window of a run with ``--blur SIGMA_MAX``: radius r = ceil(3 SIGMA_MAX) (kernel_size 2 r + 1), 1..12; None -> None"""
    import math
    sigma_max = parse_blur(sigma_max)
    return None if sigma_max is None else int(math.ceil(3.0 * sigma_max))


def parse_jitter(value):
    """``--jitter B[,C]`` / a checkpoint's ``jitter``: None, a 'B' / 'B,C' string or a (B, C) pair -> None (unset, also for 0 and 0,0) or
    [B, C], finite floats >= 0 (C defaults to 0)"""
    if value is None:
        return None
    if isinstance(value, str):
        parts = value.split(',')
    elif isinstance(value, (list, tuple)):
        parts = list(value)
    else:
        parts = [value]
    expected = 'jitter: B[,C] expected, got %r' % (value,)
    if not 1 <= len(parts) <= 2:
        raise ValueError(expected)
    bc = _floats(parts, expected, _finite, 'jitter: B and C must be finite and not negative, got %r' % (value,)) + [0.0] * (2 - len(parts))
    return bc if any(bc) else None


def parse_mix_alpha(value, name='mixup'):
    """``--mixup ALPHA`` / ``--cutmix ALPHA`` / a checkpoint's value: None, a number or its string -> 0.0 (off, also for None and 0) or a
    finite float > 0, the parameter of the Beta(ALPHA, ALPHA) draw"""
    if value is None:
        return 0.0
    return _floats([value], '%s: ALPHA expected, got %r' % (name, value), _finite,
                   '%s: ALPHA must be a finite float >= 0 (0 = off), got %r' % (name, value))[0]


def parse_mix_prob(value):
    """``--mix-prob P`` / a checkpoint's ``mix_prob``: None -> 1.0, else a float in [0, 1]"""
    if value is None:
        return 1.0
    return _floats([value], 'mix-prob: P expected, got %r' % (value,), _unit, 'mix-prob: P must be in [0, 1], got %r' % (value,))[0]


def cut_box(lam0, cy, cx, S):
    """timm's ``rand_bbox`` with no margin, the centre given: (y0, y1, x0, x1) of the box cut for a Beta draw ``lam0``"""
    cut_h = cut_w = int(S * np.sqrt(1.0 - lam0))
    y0, y1 = int(np.clip(cy - cut_h // 2, 0, S)), int(np.clip(cy + cut_h // 2, 0, S))
    x0, x1 = int(np.clip(cx - cut_w // 2, 0, S)), int(np.clip(cx + cut_w // 2, 0, S))
    return y0, y1, x0, x1


def box_lam(box, S):
    """timm's ``correct_lam``: the share of the image outside the box"""
    y0, y1, x0, x1 = box
    return 1.0 - (y1 - y0) * (x1 - x0) / float(S * S)


class BatchMix:
    """The per-batch draw of TRAIN --mixup / --cutmix, after timm's ``Mixup`` in batch mode: one ``lam`` (and, for CutMix, one box) per
    batch; the partner of image n is image N - 1 - n.  ``mixup`` / ``cutmix``: the Beta parameters, 0 = off (not both); ``prob``: the
    probability that a batch is mixed at all.  The draws come from a generator of this object's own, seeded from (seed, rank): neither
    ``random`` nor the global numpy / torch streams are touched, so a run without the flags keeps its streams bit for bit."""

    def __init__(self, mixup=0.0, cutmix=0.0, prob=1.0, seed=0, rank=0):
        self.mixup, self.cutmix, self.prob = parse_mix_alpha(mixup, 'mixup'), parse_mix_alpha(cutmix, 'cutmix'), parse_mix_prob(prob)
        if not (self.mixup > 0 or self.cutmix > 0):
            raise ValueError('BatchMix: one of mixup and cutmix must be > 0')
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([0x6d6978, int(seed or 0) & 0xffffffffffffffff, int(rank)])))

    def draw(self, S):
        """-> (lam, box): lam a python float in [0, 1], box None (Mixup, or an unmixed batch: lam == 1) or (y0, y1, x0, x1) (CutMix, with
        lam corrected to the share of the image outside the box).  Order of the draws: mixed at all (only with prob < 1), which of the
        two (only with both set: CutMix with probability 0.5, timm's switch_prob), the Beta value, the box centre cy then cx."""
        if self.prob < 1.0 and not self.rng.random() < self.prob:
            return 1.0, None
        cut = self.cutmix > 0 and (not self.mixup > 0 or self.rng.random() < 0.5)
        if not cut:
            return float(self.rng.beta(self.mixup, self.mixup)), None
        lam0 = float(self.rng.beta(self.cutmix, self.cutmix))
        cy, cx = int(self.rng.integers(0, S)), int(self.rng.integers(0, S))
        box = cut_box(lam0, cy, cx, S)
        return box_lam(box, S), box


def parse_affine(rotate=None, translate=None, scale=None):
    """the ranges of a random affine (``RandomAffine(degrees=DEG, translate=(T, T), scale=(LO, HI))``) -> None (nothing set: also for
    0, 0 and 1:1) or (DEG, T, LO, HI).  Host arithmetic only so far: no kernel applies the draw yet, and TRAIN has no flag for it.  DEG finite and >= 0, 0 <= T <= 1, 0.25 <= LO <= HI <= 4: with these every matrix a draw can give stays inside
    the range of Pillow's 16.16 fixed-point routine.  scale: None, a 'LO:HI' string, one number (LO = HI) or a (LO, HI) pair."""
    def num(v, what, ok=None, wrong=None):
        return _floats([v], '%s: a number expected, got %r' % (what, v), ok, wrong)[0]
    deg = 0.0 if rotate is None else num(rotate, 'rotate', _finite, 'rotate: DEG must be finite and not negative, got %r' % (rotate,))
    t = 0.0 if translate is None else num(translate, 'translate', _unit, 'translate: FRAC must be in [0, 1], got %r' % (translate,))
    if scale is None:
        lo = hi = 1.0
    else:
        if isinstance(scale, str):
            parts = scale.split(':')
        elif isinstance(scale, (list, tuple)):
            parts = list(scale)
        else:
            parts = [scale]
        if not 1 <= len(parts) <= 2:
            raise ValueError('scale: LO:HI expected, got %r' % (scale,))
        lo, hi = (num(v, 'scale') for v in (parts[0], parts[-1]))
        if not 0.25 <= lo <= hi <= 4.0:
            raise ValueError('scale: 0.25 <= LO <= HI <= 4 expected, got %r' % (scale,))
    if deg == 0.0 and t == 0.0 and lo == 1.0 and hi == 1.0:
        return None
    return deg, t, lo, hi


def affine_matrix(S, angle, translate, scale):
    """torchvision's ``_get_inverse_affine_matrix`` about the centre (S * 0.5, S * 0.5) with no shear: the six floats that
    ``RandomAffine`` hands to ``Image.transform((S, S), AFFINE, m, NEAREST)``; angle in degrees, translate = (tx, ty) in pixels"""
    import math
    rot = math.radians(angle)
    cx = cy = S * 0.5
    tx, ty = translate
    cs, sn = math.cos(rot), math.sin(rot)
    m = [v / scale for v in (cs, sn, 0.0, -sn, cs, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def affine_coefs(S, angle, translate, scale):
    """the six 16.16 fixed-point integers of Pillow's nearest-neighbour affine for one image: Pillow's ``FIX(v) = floor(v * 65536.0 + 0.5)`` of
    ``affine_matrix``, the half-pixel centre folded into the two offsets.  ValueError when one does not fit an int32."""
    import math
    m = affine_matrix(S, angle, translate, scale)
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    c = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    if not all(-2 ** 31 <= v < 2 ** 31 for v in c):
        raise ValueError('affine_coefs: S %d, angle %r, translate %r, scale %r do not fit 16.16 fixed point' % (S, angle, translate, scale))
    return c


AFFINE_IDENTITY = (65536, 0, 32768, 0, 65536, 32768)


class AffineDraw:
    """The per-image draw of a random affine, after torchvision's ``RandomAffine.get_params``: angle ~ U(-DEG, DEG),
    tx, ty = round(U(-T, T) * S), scale ~ U(LO, HI).  ``fill``: 'border' or a level 0..255 for what the warp uncovers.  The draws come from a
    generator of this object's own, seeded from (seed, rank): neither ``random`` nor the global numpy / torch streams are touched."""

    def __init__(self, rotate=0.0, translate=0.0, scale=None, fill='border', seed=0, rank=0):
        p = parse_affine(rotate, translate, scale)
        if p is None:
            raise ValueError('AffineDraw: one of rotate, translate and scale must be set')
        self.deg, self.t, self.lo, self.hi = p
        self.fill = parse_pad(fill)
        if self.fill is None:
            raise ValueError("AffineDraw: fill is 'border' or an integer 0..255")
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([0x616666, int(seed or 0) & 0xffffffffffffffff, int(rank)])))

    def params(self, n, S):
        """-> n tuples (angle, (tx, ty), scale).  Order of the draws: the n angles (only with DEG > 0), the n tx then the n ty (only with
        T > 0), the n scales (only with LO < HI)."""
        ang = self.rng.uniform(-self.deg, self.deg, n) if self.deg > 0 else np.zeros(n)
        if self.t > 0:
            tx = np.rint(self.rng.uniform(-self.t, self.t, n) * S)
            ty = np.rint(self.rng.uniform(-self.t, self.t, n) * S)
        else:
            tx = ty = np.zeros(n)
        sc = self.rng.uniform(self.lo, self.hi, n) if self.lo < self.hi else np.full(n, self.lo)
        return [(float(ang[i]), (int(tx[i]), int(ty[i])), float(sc[i])) for i in range(n)]

    def draw(self, n, S):
        """-> int32 tensor [n, 6] (host): ``affine_coefs`` of the draws for a batch of n images"""
        return torch.tensor([affine_coefs(S, *p) for p in self.params(n, S)], dtype=torch.int32).reshape(n, 6)


def parse_pad(value):
    """``--pad [FILL]`` / a checkpoint's ``pad``: None, 'border' or a grey level 0..255 (an int, or its decimal string)"""
    if value is None or value == 'border':
        return value
    if isinstance(value, bool):
        raise ValueError('pad: %r' % (value,))
    if isinstance(value, (int, np.integer)):
        v = int(value)
    else:
        text = str(value)
        if not (text.isascii() and text.isdigit()):
            raise ValueError("pad: FILL is 'border' or an integer 0..255, got %r" % (value,))
        v = int(text)
    if not 0 <= v <= 255:
        raise ValueError("pad: FILL is 'border' or an integer 0..255, got %r" % (value,))
    return v


blur_arg = _arg_type(parse_blur, 'SIGMA_MAX must be a float in (0.1, 4], got %r')                    # --blur SIGMA_MAX
blur_prob_arg = _arg_type(parse_blur_prob, 'P must be a float in [0, 1], got %r')                      # --blur-prob P
jitter_arg = _arg_type(parse_jitter, 'B[,C] must be one or two finite floats >= 0, got %r')            # --jitter B[,C]
mix_alpha_arg = _arg_type(parse_mix_alpha, 'ALPHA must be a finite float >= 0 (0 = off), got %r')      # --mixup ALPHA, --cutmix ALPHA
mix_prob_arg = _arg_type(parse_mix_prob, 'P must be a float in [0, 1], got %r')                        # --mix-prob P
pad_arg = _arg_type(parse_pad, 'FILL must be "border" or an integer 0..255, got %r')                   # --pad [FILL]


def fold_turns(vflip, hflip, k):
    """(vflip, hflip, then k counter-clockwise quarter turns) as the kernel's code byte: the image is
    hflip^bit1( vflip^bit0( transpose^bit2( src ) ) ).  One turn is vflip(transpose(X)), and a transpose moved inside the flips
    swaps them: (t, v, h) -> (t ^ 1, h ^ 1, v).  Each of the 16 inputs has exactly one such form."""
    t, v, h = 0, int(bool(vflip)), int(bool(hflip))
    for _ in range(k % 4):
        t, v, h = t ^ 1, h ^ 1, v
    return v | (h << 1) | (t << 2)


class NeustonDataset(Dataset):
    """neuston_data.py:21-270.  Folders of ``src`` are the classes."""

    def __init__(self, src, minimum_images_per_class=1, maximum_images_per_class=None, transforms=None,
                 images_perclass=None):
        self.src = src
        if not images_perclass:
            images_perclass = self.fetch_images_perclass(src)
        self.minimum_images_per_class = max(1, minimum_images_per_class)
        kept = {c: imgs for c, imgs in images_perclass.items() if len(imgs) >= self.minimum_images_per_class}
        dropped = sorted(set(images_perclass) - set(kept))
        self.classes_ignored_from_too_few_samples = [(c, len(images_perclass[c])) for c in dropped]
        self.classes = sorted(kept)
        self.maximum_images_per_class = maximum_images_per_class
        if maximum_images_per_class:
            assert maximum_images_per_class > self.minimum_images_per_class
            limited = {}
            for c, imgs in kept.items():
                limited[c] = sorted(random.sample(imgs, maximum_images_per_class)) \
                    if maximum_images_per_class < len(imgs) else imgs
            self.classes_limited_from_too_many_samples = [c for c in self.classes if len(limited[c]) < len(kept[c])]
            kept = limited
        else:
            self.classes_limited_from_too_many_samples = None
        kept = {c: sorted(imgs) for c, imgs in kept.items()}
        pairs = [(self.classes.index(c), i) for c in kept for i in kept[c]]
        self.targets, self.images = zip(*pairs)
        self.transforms = transforms

    @classmethod
    def fetch_images_perclass(cls, src, include_exclude_rename=None):
        if os.path.isdir(src) and include_exclude_rename is None:
            classes = sorted(d.name for d in os.scandir(src) if d.is_dir())
            out = {}
            for sub in classes:
                files = sorted(f for f in os.listdir(os.path.join(src, sub)) if os.path.splitext(f)[1] in IMG_EXTENSIONS)
                out[sub] = [os.path.join(src, sub, f) for f in files]
            return out
        if os.path.isdir(src):
            out = cls.fetch_images_perclass(src)
            for key, mode in include_exclude_rename:
                if mode == 1 or mode == '1':
                    continue
                if (mode == 0 or mode == '0') and key in out:
                    del out[key]
                else:                                   # rename / merge
                    if key not in out:
                        continue
                    if mode in out:
                        out[mode].extend(out[key])
                    else:
                        out[mode] = out[key]
                    del out[key]
            return out
        # dataset-configuration csv: columns "[priority:]dataset_dir", rows = classes  (neuston_data.py:91-140)
        import pandas as pd
        df = pd.read_csv(src, header=0, index_col=0)
        entries = []
        for col in df.columns.to_list():
            parts = col.split(':', 1)
            priority, dataset = (int(parts[0]), parts[1]) if len(parts) == 2 else (0, parts[0])
            ipc = cls.fetch_images_perclass(dataset, include_exclude_rename=zip(df.index, df[col].to_list()))
            entries.append((priority, dataset, ipc))
        prios = [p for p, _, _ in entries]
        prios = set(max(prios) + 1 if p == 0 else p for p in prios)
        entries = [((max(prios) if p == 0 else p), d, i) for p, d, i in entries]

        def extend(d1, d2):
            for k in d2:
                if k in d1:
                    d1[k].extend(d2[k])
                else:
                    d1[k] = d2[k]
        out = {}
        for level in sorted(prios):
            merged = {}
            for p, _, ipc in entries:
                if p == level:
                    extend(merged, ipc)
            for k in merged:
                random.shuffle(merged[k])
            extend(out, merged)
        return out

    @property
    def images_perclass(self):
        ipc = {c: [] for c in self.classes}
        for img, trg in zip(self.images, self.targets):
            ipc[self.classes[trg]].append(img)
        return ipc

    @property
    def count_perclass(self):
        cpc = [0] * len(self.classes)
        for t in self.targets:
            cpc[t] += 1
        return cpc

    def split(self, ratio1, ratio2, seed=None, minimum_images_per_class='scale'):
        assert ratio1 + ratio2 == 100, 'ratio1:ratio2 must sum to 100, instead got {}:{} (total: {})'.format(
            ratio1, ratio2, ratio1 + ratio2)
        d1, d2 = {}, {}
        for label, images in self.images_perclass.items():
            n1 = int(ratio1 * len(images) / 100 + 0.5)
            if n1 == len(images) and self.minimum_images_per_class > 1:
                n1 -= 1                                   # keep one for the second set
            if seed:
                random.seed(seed)                          # re-seeded for every class, as upstream (:169-171)
            pick = random.sample(images, n1)
            rest = sorted(set(images) - set(pick))
            assert len(pick) + len(rest) == len(images)
            d1[label], d2[label] = pick, rest
        ds1 = NeustonDataset(src=self.src, images_perclass=d1, transforms=self.transforms)
        ds2 = NeustonDataset(src=self.src, images_perclass=d2, transforms=self.transforms)
        assert ds1.classes == ds2.classes, 'd1-d2_classes:{}, d2-d1_classes:{}'.format(
            set(ds1.classes) - set(ds2.classes), set(ds2.classes) - set(ds1.classes))
        assert len(ds1) + len(ds2) == len(self), 'd1_len:{}, d2_len:{}'.format(len(ds1), len(ds2))
        return ds1, ds2

    @classmethod
    def from_csv(cls, src, csv_file, column_to_run, transforms=None, minimum_images_per_class=1,
                 maximum_images_per_class=None):
        import pandas as pd
        df = pd.read_csv(csv_file, header=0)
        base_list = df.iloc[:, 0].tolist()
        mod_list = df[column_to_run].tolist()
        found = cls.fetch_images_perclass(src)
        missing_src = [c for c in found if c not in base_list]
        new, missing_csv, skipped, grouped = {}, [], [], {}
        for base, mod in zip(base_list, mod_list):
            if base not in found:
                missing_csv.append(base)
                continue
            if str(mod) == '0':
                skipped.append(base)
                continue
            if str(mod) == '1':
                label = base
            else:
                label = mod
                grouped.setdefault(mod, []).append(base)
            if label not in new:
                new[label] = found[base]
            else:
                new[label].extend(found[base])
        name = os.path.basename(csv_file)
        if missing_src:
            print('\n    '.join(['\n{} of {} classes from src dir {} were NOT FOUND in {}'.format(
                len(missing_src), len(found), src, name)] + missing_src))
        if missing_csv:
            print('\n    '.join(['\n{} of {} classes from {} were NOT FOUND in src dir {}'.format(
                len(missing_csv), len(base_list), name, src)] + missing_csv))
        if grouped:
            print('\n{} GROUPED classes were created, as per {}'.format(len(grouped), name))
            for mod, bases in grouped.items():
                print('  {}'.format(mod))
                print('\n'.join('     <-- {}'.format(c) for c in bases))
        if skipped:
            print('\n    '.join(['\n{} classes were SKIPPED, as per {}'.format(len(skipped), name)] + skipped))
        return cls(src=src, images_perclass=new, transforms=transforms,
                   minimum_images_per_class=minimum_images_per_class,
                   maximum_images_per_class=maximum_images_per_class)

    def __getitem__(self, index):
        path = self.images[index]
        data = default_loader(path)
        tail = self.transforms.draw_item() if self.transforms is not None else (0,)
        return (data,) + tail, self.targets[index], path

    def __len__(self):
        return len(self.images)

    @property
    def imgs(self):
        return self.images


def get_trainval_datasets(args):
    """neuston_data.py:292-329"""
    print('Initializing Data...')
    if not args.class_config:
        nd = NeustonDataset(src=args.SRC, minimum_images_per_class=args.class_min,
                            maximum_images_per_class=args.class_max)
    else:
        nd = NeustonDataset.from_csv(src=args.SRC, csv_file=args.class_config[0], column_to_run=args.class_config[1],
                                     minimum_images_per_class=args.class_min, maximum_images_per_class=args.class_max)
    r1, r2 = map(int, args.split.split(':'))
    pair = nd.split(r1, r2, seed=args.seed)
    training, validation = pair if not args.swap else pair[::-1]
    ci_nd = nd.classes_ignored_from_too_few_samples
    ci_train = training.classes_ignored_from_too_few_samples
    ci_eval = validation.classes_ignored_from_too_few_samples
    assert ci_eval == ci_train
    if ci_nd:
        msg = '\n{} out of {} classes ignored from --class-minimum {}, PRE-SPLIT'.format(
            len(ci_nd), len(nd.classes + ci_nd), args.class_min)
        print('\n    '.join([msg] + ['({:2}) {}'.format(l, c) for c, l in ci_nd]))
    if ci_eval:
        msg = '\n{} out of {} classes ignored from --class-minimum {}, POST-SPLIT'.format(
            len(ci_eval), len(validation.classes + ci_eval), args.class_min)
        print('\n    '.join([msg] + ['({:2}) {}'.format(l, c) for c, l in ci_eval]))
    training.transforms, validation.transforms = get_trainval_transforms(args)
    return training, validation


def parse_imgnorm(img_norm_arg):
    """neuston_data.py:331-339: "m" / "m1,m2,m3" strings -> two 3-lists of floats."""
    mean = [float(m) for m in img_norm_arg[0].split(',')]
    if len(mean) == 1:
        mean = 3 * mean
    std = [float(s) for s in img_norm_arg[1].split(',')]
    if len(std) == 1:
        std = 3 * std
    assert len(mean) == len(std) == 3, '--img-norm invalid: {}'.format(img_norm_arg)
    return mean, std


def get_trainval_transforms(args):
    """neuston_data.py:342-371; sets args.resize (299 only for the exact name 'inception_v3')."""
    args.resize = 299 if args.MODEL == 'inception_v3' else 224
    norm = parse_imgnorm(args.img_norm) if args.img_norm else None
    flip = args.flip or ''
    vflip, hflip = 'x' in flip, 'y' in flip                # 'x' = vertical, 'y' = horizontal (sic)
    # the options a caller's args may lack (None = unset).  rot90: 'T' (training set) | '+V' (validation set as well); pad: geometry,
    # not augmentation, so both sets alike; jitter, blur and batch mixing: the training set only
    opt = {k: getattr(args, k, None) for k in ('rot90', 'pad', 'jitter', 'mixup', 'cutmix', 'mix_prob', 'blur', 'blur_prob', 'seed')}
    own = dict(seed=opt['seed'] or 0, rank=int(os.environ.get('RANK', 0)))      # what the blur and mix generators are seeded from
    # absent or 0: no BatchMix object, no draw
    mixup, cutmix = parse_mix_alpha(opt['mixup'], 'mixup'), parse_mix_alpha(opt['cutmix'], 'cutmix')
    mix = BatchMix(mixup, cutmix, parse_mix_prob(opt['mix_prob']), **own) if mixup > 0 or cutmix > 0 else None
    train = RoiTransform(args.resize, norm, vflip, hflip, rot90=bool(opt['rot90']), pad=opt['pad'], jitter=opt['jitter'], mix=mix,
                         blur=opt['blur'], blur_prob=opt['blur_prob'], **own)
    val = RoiTransform(args.resize, norm, vflip and '+V' in flip, hflip and '+V' in flip, rot90=opt['rot90'] == '+V', pad=opt['pad'])
    return train, val


class ImageDataset(Dataset):
    """neuston_data.py:376-406 (RUN --type img).  No Normalize, as upstream (quirk: img_norm is ignored here)."""

    def __init__(self, image_paths, resize=244, input_src=None, pad=None):
        self.input_src = input_src
        self.image_paths = [img for img in image_paths if img.endswith(IMG_EXTENSIONS)]
        self.transform = RoiTransform(resize, pad=pad)
        if len(self.image_paths) < len(image_paths):
            print('{} non-image files were ommited'.format(len(image_paths) - len(self.image_paths)))
        if len(self.image_paths) == 0:
            raise RuntimeError('No images Loaded!!')

    def __getitem__(self, index):
        path = self.image_paths[index]
        return (default_loader(path), 0), path

    def __len__(self):
        return len(self.image_paths)


class IfcbBinDataset(Dataset):
    """neuston_data.py:433-467.  ``bin`` is any object with ``.pid`` (``with_target(n)``), ``.schema`` and
    ``.images`` ({target_number: 2-D u8 array}); schema-v1 bins must already be stitched/infilled (pyifcb's
    ``InfilledImages`` is not available here: parity unpinned for that step)."""

    def __init__(self, bin, resize, img_norm=None, pad=None):
        self.bin = bin
        self.images, self.pids = [], []
        self.img_norm = parse_imgnorm(img_norm) if img_norm else None
        self.resize = resize[0] if isinstance(resize, (tuple, list)) else resize
        self.transform = RoiTransform(self.resize, self.img_norm, pad=pad)
        if getattr(bin, 'schema', None) == 'v1' and not getattr(bin, 'stitched', False) \
                and os.environ.get('IFCBK_ALLOW_UNSTITCHED_V1', '0') == '0':
            # upstream reads old-style bins through pyifcb's InfilledImages (stitched ROI pairs, :446-449); that algorithm is
            # not available here, and classifying the raw halves would silently change the ROI set of the bin
            raise NotImplementedError('{}: schema-v1 (old-style) bin -- ROI stitching / infilling is not implemented on this path; '
                                      'set IFCBK_ALLOW_UNSTITCHED_V1=1 to classify its raw ROIs knowingly'.format(bin.pid))
        for target_number, img in bin.images.items():
            self.images.append(np.ascontiguousarray(img, dtype=np.uint8))
            self.pids.append(bin.pid.with_target(target_number))

    def __getitem__(self, item):
        return (self.images[item], 0), self.pids[item]

    def __len__(self):
        return len(self.pids)


# ------------------------------------------------------------------------------------------ batching
def collate_draws(tails):
    """the items' draws ``(flip[, turn[, fb, fc[, sigma]]])`` (``RoiTransform.draw_item``; a plain item has ``(flip,)``) as a batch's
    entries: ``flips``, uint8 codes; ``turn`` = True when some item is flagged (its transform has rot90 set), which marks the batch for
    the quarter-turn kernels whatever codes were drawn; float32 ``brightness`` / ``contrast``, each present only when some item carries
    that factor (an item without it counts as 1); float32 ``blur``, present only when some item's sigma is not 0."""
    out = dict(flips=torch.tensor([t[0] for t in tails], dtype=torch.uint8))
    if any(len(t) > 1 and t[1] for t in tails):
        out['turn'] = True
    for key, k in (('brightness', 2), ('contrast', 3)):
        if any(len(t) > k and t[k] is not None for t in tails):
            out[key] = torch.tensor([t[k] if len(t) > k and t[k] is not None else 1.0 for t in tails], dtype=torch.float32)
    if any(len(t) > 4 and t[4] for t in tails):
        out['blur'] = torch.tensor([t[4] if len(t) > 4 else 0.0 for t in tails], dtype=torch.float32)
    return out


def collate_rois(items):
    """DataLoader collate_fn: [( (img_u8, flip[, turn[, fb, fc[, sigma]]]), *rest )] -> (roi_batch dict, *rest lists).  One ragged u8 blob,
    an int64 offset table and int32 dims; tensors are pinned by the loader (pin_memory=True).  What follows the image becomes the
    ``flips`` / ``turn`` / ``brightness`` / ``contrast`` / ``blur`` entries of ``collate_draws``."""
    imgs = [it[0][0] for it in items]
    ch = 3 if any(im.ndim == 3 for im in imgs) else 1
    if ch == 3:
        imgs = [im if im.ndim == 3 else np.repeat(im[:, :, None], 3, 2) for im in imgs]
    hs = torch.tensor([im.shape[0] for im in imgs], dtype=torch.int32)
    ws = torch.tensor([im.shape[1] for im in imgs], dtype=torch.int32)
    sizes = hs.long() * ws.long() * ch
    offs = torch.zeros(len(imgs), dtype=torch.int64)
    if len(imgs) > 1:
        offs[1:] = torch.cumsum(sizes, 0)[:-1]
    blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in imgs]))
    batch = dict(pixels=blob, offs=offs, hs=hs, ws=ws, max_h=int(hs.max()), max_w=int(ws.max()), in_channels=ch)
    batch.update(collate_draws([it[0][1:] for it in items]))
    rest = list(zip(*[it[1:] for it in items]))
    out = [batch]
    for r in rest:
        r = list(r)
        out.append(torch.tensor(r, dtype=torch.int64) if isinstance(r[0], (int, np.integer)) else r)
    return tuple(out)


def rois_to_device(batch, device, transform=None):
    """upload a collated ROI batch (u8 blob + tables) and attach Normalize parameters, the transform's ``pad`` (when set) and the
    batch's jitter factors (when it carries any): ``jitter=(brightness, contrast)``, device tensors or None; likewise ``blur``, the
    device tensor of the batch's sigmas."""
    kw = dict(pixels=batch['pixels'].to(device, non_blocking=True), offs=batch['offs'].to(device, non_blocking=True),
              hs=batch['hs'].to(device, non_blocking=True), ws=batch['ws'].to(device, non_blocking=True),
              max_h=batch['max_h'], max_w=batch['max_w'], in_channels=batch['in_channels'])
    return attach_draws(kw, batch, device, transform)


def attach_settings(kw, transform):
    """the transform's Normalize / pad settings, added to the ``load_rois`` arguments ``kw`` (``transform`` None: nothing)"""
    if transform is not None and transform.img_norm is not None:
        kw['mean'], kw['std'] = transform.img_norm
    if transform is not None and getattr(transform, 'pad', None) is not None:
        kw['pad'] = transform.pad
    return kw


def attach_draws(kw, batch, device, transform=None):
    """the second half of ``rois_to_device``: the batch's flip codes, jitter factors and sigmas (``batch``: a collated batch, or
    ``draw_items``' result) and ``attach_settings``, added to the ``load_rois`` arguments ``kw`` of ROIs already on the device"""
    if batch.get('turn') or (transform is not None and getattr(transform, 'rot90', False)):
        # the codes may hold a transpose bit: always handed over, so the kernels a run launches do not depend on the draw
        kw['flips'] = batch['flips'].to(device, non_blocking=True)
        kw['turn'] = True
    elif batch['flips'].any():
        kw['flips'] = batch['flips'].to(device, non_blocking=True)
    if 'brightness' in batch or 'contrast' in batch:
        kw['jitter'] = tuple(batch[k].to(device, non_blocking=True) if k in batch else None for k in ('brightness', 'contrast'))
    if 'blur' in batch:
        kw['blur'] = batch['blur'].to(device, non_blocking=True)
    return attach_settings(kw, transform)


# ------------------------------------------------------------------------------------------ TRAIN --resident
class _DecodeOnly(Dataset):
    """what ``ResidentSet.build`` iterates: ``default_loader`` of each path and nothing else -- no transform, no random draw"""

    def __init__(self, paths):
        self.paths = list(paths)

    def __getitem__(self, index):
        return default_loader(self.paths[index])

    def __len__(self):
        return len(self.paths)


def _as_list(items):
    return list(items)


class ResidentSet:
    """A dataset decoded ONCE and held as ragged u8 ROIs (TRAIN --resident): one blob in ``dataset.images`` order, an int64 offset table
    of n + 1 entries (the last one the blob's size), int32 heights and widths, int64 targets and the path list.  ``in_channels`` is 1
    when every image is 2-D (grey), else 3 with the grey images replicated here, once; ``collate_rois`` decides that per BATCH, so the
    two feeds agree for all-grey and all-RGB datasets only.  ``to_device`` uploads blob and tables once; every batch of every epoch is
    then cut on the device by ``cut`` (ifcbk_roi_gather), which leaves the resident blob untouched -- ifcbk_roi_jitter maps the blob it
    is given in place, so the resize kernels never get the resident one.  Data parallel: every rank holds the full set (the epoch
    permutation is global); sharded residency is not implemented."""

    def __init__(self, blob, offs, hs, ws, targets, paths, in_channels):
        self.blob, self.offs, self.hs, self.ws, self.targets = blob, offs, hs, ws, targets
        self.paths, self.in_channels = list(paths), int(in_channels)
        self.dev = None                   # to_device: dict(pixels, offs, hs, ws, targets) of device tensors
        self.ready = None                 # ... and the event recorded behind their upload
        self.stream = None                # ... on this stream

    @classmethod
    def build(cls, dataset, loaders=0):
        """one pass over ``dataset.images`` in their order, through a DataLoader of ``loaders`` workers over ``default_loader`` alone.
        Touches neither ``dataset.transforms`` nor any random stream: ``__getitem__`` would call ``flip_code()``, and a DataLoader
        draws its workers' base seed from torch's global generator unless it is handed one of its own."""
        from torch.utils.data import DataLoader
        paths = list(dataset.images)
        loader = DataLoader(_DecodeOnly(paths), batch_size=64, shuffle=False, num_workers=int(loaders), collate_fn=_as_list,
                            generator=torch.Generator())
        imgs = [im for chunk in loader for im in chunk]
        ch = 3 if any(im.ndim == 3 for im in imgs) else 1
        if ch == 3:
            imgs = [im if im.ndim == 3 else np.repeat(im[:, :, None], 3, 2) for im in imgs]
        hs = np.array([im.shape[0] for im in imgs], np.int32)
        ws = np.array([im.shape[1] for im in imgs], np.int32)
        offs = np.zeros(len(imgs) + 1, np.int64)
        np.cumsum(hs.astype(np.int64) * ws * ch, out=offs[1:])
        blob = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in imgs]) if imgs else np.zeros(0, np.uint8)
        return cls(blob, offs, hs, ws, np.array(dataset.targets, np.int64), paths, ch)

    def __len__(self):
        return len(self.hs)

    @property
    def nbytes(self):
        """what ``to_device`` puts on the GPU"""
        return int(self.blob.nbytes + self.offs.nbytes + self.hs.nbytes + self.ws.nbytes + self.targets.nbytes)

    def to_device(self, device, stream):
        """one pinned upload of the blob and the tables on ``stream``, and the ``ready`` event behind it (as ``upload_bin``)"""
        with torch.cuda.stream(stream):
            host = {k: torch.from_numpy(getattr(self, a)).pin_memory() for k, a in
                    (('pixels', 'blob'), ('offs', 'offs'), ('hs', 'hs'), ('ws', 'ws'), ('targets', 'targets'))}
            self._pinned = host           # (lives as long as the set: the copies below are asynchronous)
            self.dev = {k: v.to(device, non_blocking=True) for k, v in host.items()}
            self.ready = torch.cuda.Event()
            self.ready.record(stream)
        self.stream = stream
        return self

    def check_indices(self, idx_host):
        """the range check ifcbk_roi_gather cannot make: on the HOST copy of the indices, before anything is launched"""
        idx = np.asarray(idx_host, np.int64).reshape(-1)
        if idx.size < 1 or int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError('ResidentSet: %d indices in [%s, %s] for a set of %d ROIs' % (
                idx.size, idx.min() if idx.size else '-', idx.max() if idx.size else '-', len(self)))
        return idx

    def cut(self, ctx, idx_dev, idx_host, stream):
        """the compact batch of ROIs ``idx`` (``idx_dev``: int64 device tensor, ``idx_host``: its host copy) on ``stream`` through the
        library context ``ctx``: fresh ``pixels`` / ``offs`` / ``hs`` / ``ws`` tensors, allocated through torch under the current
        stream as an upload's are, plus the batch's own ``max_h`` / ``max_w`` and ``in_channels`` -- the first seven entries of
        ``rois_to_device``'s result.  No host sync: sizes and maxima come from the host table."""
        from . import _lib
        idx = self.check_indices(idx_host)
        n = idx.size
        if not (torch.is_tensor(idx_dev) and idx_dev.dtype == torch.int64 and idx_dev.is_cuda and idx_dev.numel() == n and idx_dev.is_contiguous()):
            raise ValueError('ResidentSet.cut: idx_dev is a contiguous int64 device tensor of the %d indices' % n)
        if n > _lib.ROI_GATHER_MAX_N:
            raise ValueError('ResidentSet.cut: %d ROIs in one batch, ifcbk_roi_gather takes %d' % (n, _lib.ROI_GATHER_MAX_N))
        total = int((self.offs[idx + 1] - self.offs[idx]).sum())
        d, dev = self.dev, self.dev['pixels'].device
        pixels = torch.empty(total, dtype=torch.uint8, device=dev)
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        hs = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(n, dtype=torch.int32, device=dev)
        ctx.call('ifcbk_roi_gather', _lib.ptr(d['pixels']), _lib.ptr(d['offs']), _lib.ptr(d['hs']), _lib.ptr(d['ws']), _lib.ptr(idx_dev), n,
                 self.in_channels, _lib.ptr(pixels), total, _lib.ptr(offs), _lib.ptr(hs), _lib.ptr(ws), _lib._vp(stream.cuda_stream))
        return dict(pixels=pixels, offs=offs[:n], hs=hs, ws=ws, max_h=int(self.hs[idx].max()), max_w=int(self.ws[idx].max()),
                    in_channels=self.in_channels)


def draw_items(transform, n):
    """the per-item draws of n items in batch order, by the very call ``NeustonDataset.__getitem__`` makes (``RoiTransform.draw_item``),
    as the entries ``collate_rois`` builds from such items (``collate_draws``): a ``--resident`` run and a ``--loaders 0`` run of the
    same command consume identical random streams."""
    return collate_draws([transform.draw_item() if transform is not None else (0,) for _ in range(n)])
