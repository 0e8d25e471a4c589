"""Twin of the reference's ``neuston_util.py``: the auxiliary commands run before TRAIN.

``MAKE_DATASET_CONFIG`` and ``MAKE_CLASS_CONFIG`` are host code with the reference's output, byte for byte.
``CALC_IMG_NORM`` runs on the GPU: the Pillow-exact resize of ``ifcbk_roi_preprocess`` writes the u8 plane, and
``ifcbk_u8_channel_moments`` sums v and v*v per image and channel.  Since ToTensor only divides those bytes by 255, a
batch's mean and population std follow exactly from the two sums; they are rounded once to float32 (the reference
accumulates in float32).  From there on the reference's own numpy steps aggregate the batches.

    python -m ifcb_classifier_amd.neuston_util CMD ...
"""
import argparse
import csv
import math
import os
from fractions import Fraction

import numpy as np

from .neuston_data import pad_arg


# ------------------------------------------------------------------------------------------ CALC_IMG_NORM
def _round_f32(cmp, guess):
    """the float32 nearest to a positive real t (ties to even), given cmp(f) = sign(t - f) for a rational f and a close guess"""
    x = np.float32(guess)
    while True:
        up = np.nextafter(x, np.float32(np.inf))
        dn = np.nextafter(x, np.float32(0))
        hi = (Fraction(float(x)) + Fraction(float(up))) / 2
        lo = (Fraction(float(x)) + Fraction(float(dn))) / 2
        c_hi, c_lo = cmp(hi), cmp(lo)
        if c_hi > 0 or (c_hi == 0 and int(up.view(np.uint32)) % 2 == 0):
            x = up
        elif c_lo < 0 or (c_lo == 0 and x > 0 and int(dn.view(np.uint32)) % 2 == 0):
            x = dn
        else:
            return x


def _sign(a, b):
    return (a > b) - (a < b)


def batch_stats(sum_v, sum_v2, count):
    """Mean and population std (ddof = 0) of ``count`` bytes per channel on the ToTensor scale (v / 255), from their exact sums
    ``sum_v`` and ``sum_v2`` (one entry per channel).  Python integers throughout -- ``count * sum_v2 - sum_v**2`` overflows int64
    from about 130 all-255 planes of 299^2 -- and each value is rounded once to float32.  One channel (a batch of grey ROIs) is
    reported for all three, as the reference converts to RGB first.  Returns two float32 arrays of shape (3,)."""
    n = int(count)
    mean, std = [], []
    for s, s2 in zip(sum_v, sum_v2):
        s, s2 = int(s), int(s2)
        den = 255 * n                                       # mean = s / den
        if s == 0:
            mean.append(np.float32(0))
        else:
            mean.append(_round_f32(lambda f: _sign(s * f.denominator, f.numerator * den), s / den))
        num = n * s2 - s * s                                # std = sqrt(num) / den
        if num == 0:
            std.append(np.float32(0))
        else:
            std.append(_round_f32(lambda f: _sign(num * f.denominator ** 2, f.numerator ** 2 * den * den), math.sqrt(num) / den))
    if len(mean) == 1:
        mean, std = mean * 3, std * 3
    return np.array(mean, np.float32), np.array(std, np.float32)


def reduce_batches(moments, num_batches):
    """neuston_util.py:26-54 on per-batch moments: ``moments`` yields (sum_v, sum_v2, count) per batch; prints the reference's
    progress ('.' per batch, a status line every 100th) and returns the unweighted mean of the per-batch means and stds."""
    pop_mean = []
    pop_std0 = []
    for i, (sum_v, sum_v2, count) in enumerate(moments, 1):
        batch_mean, batch_std0 = batch_stats(sum_v, sum_v2, count)
        pop_mean.append(batch_mean)
        pop_std0.append(batch_std0)
        if i % 100 == 0:
            line = '\n{:.1f}% ({} of {}) MEAN={} STD={}'
            line = line.format(100 * i / num_batches, i, num_batches,
                               np.array(pop_mean).mean(axis=0)[0],
                               np.array(pop_std0).mean(axis=0)[0])
            print(line)
        else:
            print('.', end='', flush=True)
    mean = np.array(pop_mean).mean(axis=0)
    std0 = np.array(pop_std0).mean(axis=0)
    return mean, std0


def gpu_moments(loader, resize, device=0, pad=None):
    """per batch of ``loader`` (``collate_rois`` batches): resize on the GPU to the u8 plane, then its channel moments; yields
    (sum_v, sum_v2, count) as Python integers, one entry per channel of the plane (1 for grey batches, 3 otherwise).
    pad: as ``Engine.load_rois`` (the statistics of a padded dataset include the padding)"""
    import ctypes as C
    import torch
    from . import _lib
    from .neuston_data import rois_to_device
    if not torch.cuda.is_available():
        raise RuntimeError('CALC_IMG_NORM runs on the GPU (ifcbk_roi_preprocess + ifcbk_u8_channel_moments) and found none; '
                           'there is no CPU fallback')
    dev = torch.device('cuda', device)
    torch.cuda.set_device(dev)
    ctx = _lib.Context(device)
    try:
        for batch in loader:
            kw = rois_to_device(batch[0], dev)
            n, ch = int(kw['hs'].numel()), int(kw['in_channels'])
            d, fn, fill = _lib.roi_resize(n, resize, ch, _lib.BF16, pad=pad)
            need = getattr(ctx.lib, fn + '_workspace')(C.byref(d), kw['max_h'], kw['max_w'])
            if need > ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h):
                ctx.reserve(need)
            plane = torch.empty((n, resize, resize, ch), dtype=torch.uint8, device=dev)
            mom = torch.empty((n, ch, 2), dtype=torch.int64, device=dev)        # uint64 bits; every sum is < 2^63
            stream = _lib.cur_stream()
            ctx.call(fn, C.byref(d), _lib.ptr(kw['pixels']), _lib.ptr(kw['offs']), _lib.ptr(kw['hs']),
                     _lib.ptr(kw['ws']), None, kw['max_h'], kw['max_w'], *fill, None, _lib.ptr(plane), stream)
            ctx.call('ifcbk_u8_channel_moments', _lib.ptr(plane), n, resize * resize, ch, _lib.ptr(mom), stream)
            m = mom.cpu().numpy().view(np.uint64).astype(object).sum(axis=0)      # [ch][2], Python integers
            yield [int(v) for v in m[:, 0]], [int(v) for v in m[:, 1]], n * resize * resize
    finally:
        torch.cuda.synchronize(dev)
        ctx.close()


def calc_img_norm(args):
    """neuston_util.py:13-54: per-channel MEAN and STD (two float32 arrays of shape (3,)) of the dataset at args.resize^2"""
    from torch.utils.data import DataLoader
    from .neuston_data import NeustonDataset, collate_rois
    if not args.class_config:
        nd = NeustonDataset(src=args.SRC, minimum_images_per_class=args.class_min, maximum_images_per_class=args.class_max)
    else:
        nd = NeustonDataset.from_csv(src=args.SRC, csv_file=args.class_config[0], column_to_run=args.class_config[1],
                                     minimum_images_per_class=args.class_min, maximum_images_per_class=args.class_max)
    loaders = getattr(args, 'loaders', 4)
    dataloader = DataLoader(nd, batch_size=args.batch_size, shuffle=False, num_workers=loaders, collate_fn=collate_rois,
                            pin_memory=True)
    pad = getattr(args, 'pad', None)
    # (without --pad the call is the two-argument one it always was: callers that swap gpu_moments for a host twin keep working)
    moments = gpu_moments(dataloader, args.resize) if pad is None else gpu_moments(dataloader, args.resize, pad=pad)
    return reduce_batches(moments, len(dataloader))


# ------------------------------------------------------------------------------------------ config makers
def write_csv(outfile, rows):
    """neuston_util.py:56-63 (the reference reads the global args.outfile here; the value is passed instead)"""
    if outfile:
        with open(outfile, 'w') as f:
            writer = csv.writer(f)
            writer.writerows(rows)
    else:
        for row in rows:
            print(','.join(row))


def make_dataset_config(args):
    """neuston_util.py:66-97"""
    datasets = []
    priorities = []
    for src in args.dataset:
        src = src.split(':', 1)
        if len(src) == 2:
            datasets.append(src[1])
            priorities.append(int(src[0]))
        else:
            datasets.append(src[0])
            priorities.append(0)
    priorities = [p if p > 0 else max(priorities) + 1 for p in priorities]

    classes = set()
    dataset_subdirs = []
    for dataset in datasets:
        subdirs = [subdir for subdir in os.listdir(dataset) if os.path.isdir(os.path.join(dataset, subdir))]
        dataset_subdirs.append(subdirs)
        classes.update(subdirs)
    classes = sorted(classes)

    header = [''] + ['{}:{}'.format(p, d) for p, d in zip(priorities, datasets)]
    rows = []
    for cls in classes:
        defaults = ['1' if cls in dssd else '0' for dssd in dataset_subdirs]
        rows.append([cls] + defaults)
    write_csv(args.outfile, [header] + rows)


def make_class_config(args):
    """neuston_util.py:101-121"""
    if os.path.isdir(args.dataset):
        classes = [subdir for subdir in os.listdir(args.dataset) if os.path.isdir(os.path.join(args.dataset, subdir))]
    elif os.path.isfile(args.dataset) and args.dataset.endswith('.csv'):
        with open(args.dataset) as f:
            reader = csv.reader(f)
            next(reader)
            rows = list(reader)
        classes = [row[0] for row in rows if any([val != '0' for val in row[1:]])]
    else:
        raise ValueError(f'Dataset is invalid: "{args.dataset}"')
    classes.sort()

    header = [args.dataset, 'CONFIG1']
    rows = []
    for cls in classes:
        rows.append([cls, '1'])
    write_csv(args.outfile, [header] + rows)


def main(args):
    if args.cmd == 'MAKE_DATASET_CONFIG':
        make_dataset_config(args)
    elif args.cmd == 'MAKE_CLASS_CONFIG':
        make_class_config(args)
    elif args.cmd == 'CALC_IMG_NORM':
        print('Calculating Image Normalization MEAN and STD...')
        mean, std = calc_img_norm(args)
        print('MEAN={}, STD={}'.format(mean, std))


def argparse_init():
    """neuston_util.py:135-162 (plus --batch-size type=int and --loaders)"""
    parser = argparse.ArgumentParser()
    subparsers = parser.add_subparsers(dest='cmd', help='These sub-commands are mutually exclusive.')

    # DATASET CONFIG CSV #
    dataset_config = subparsers.add_parser('MAKE_DATASET_CONFIG', help='Creates a default dataset-combining configuration file.')
    dataset_config.add_argument('dataset', metavar='PATH', nargs='+',
                                help='List of dataset paths. Space deliminated. '
                                     'You may optionally prefix the paths with "n:" where n is an integer priority value. Lower values are higher priority.'
                                     'Multiple Datasets may have the same priority level. '
                                     'If only some datasets have priority values, datasets without priority values are designated with the lowers priority level.')
    dataset_config.add_argument('-o', '--outfile', help='Specify an output file. If unset, outputs to stdout.')

    # CLASS-CONFIG CSV #
    class_config = subparsers.add_parser('MAKE_CLASS_CONFIG', help='Creates a default class-config csv file.')
    class_config.add_argument('dataset', metavar='PATH', help='path to a dataset directory or dataset configuration csv file.')
    class_config.add_argument('-o', '--outfile', help='Specify an output file. If unset, outputs to stdout.')

    # IMAGE NORMALIZATION
    imgnorm = subparsers.add_parser('CALC_IMG_NORM', help='Calculate the MEAN and STD of dataset for image normalizing')
    imgnorm.add_argument('SRC')
    imgnorm.add_argument('--resize', metavar='N', default=299, type=int, choices=[224, 299], help='Default is 299 (for inception_v3)')
    imgnorm.add_argument('--class-config', metavar=('CSV', 'COL'), nargs=2, help='Skip and combine classes as defined by column COL of a special CSV configuration file')
    imgnorm.add_argument('--class-min', metavar='MIN', default=2, type=int, help='Exclude classes with fewer than MIN instances. Default is 2')
    imgnorm.add_argument('--class-max', metavar='MAX', default=None, type=int, help='Limit classes to a MAX number of instances. '
                         'If multiple datasets are specified with a dataset-configuration csv, classes from lower-priority datasets are truncated first.')
    imgnorm.add_argument('--pad', metavar='FILL', nargs='?', const='border', type=pad_arg, default=None, help='(MI355X path, additive) Statistics of the dataset as "neuston_net TRAIN --pad [FILL]" sees it: aspect ratio kept, the rest of the square filled with FILL ("border", the bare flag, or a grey level 0..255); the padding counts. Put the bare flag behind SRC')
    imgnorm.add_argument('--batch-size', metavar='B', default=108, type=int, help='Number of images per minibatch')
    imgnorm.add_argument('--loaders', metavar='N', default=4, type=int, help='Number of data-loading worker processes. Default is 4')
    return parser


if __name__ == '__main__':
    main(argparse_init().parse_args())
