#!/usr/bin/env python
"""What TRAIN delivers end to end from a directory of PNGs, with and without --resident (inception_v3, bf16, batch 256, one GPU).

The dataset is synthetic: FILES grey PNGs (default 3072) in 4 class folders, written to a temporary directory.  Height and width are
drawn independently from a log-normal distribution, exp(N(ln 64, 0.7)), clipped to [8, 640] (seed 0): a median ROI of 64 x 64, a tail
of a few hundred pixels a side, a mean near 7 kB -- the shape of an IFCB sample, where most ROIs are small and a few are large.

Timed, steady state (the first epoch of each loop is run and thrown away):
  (a) bare ``train_step`` on one loaded batch, three times over: this box's run-to-run spread
  (b) the train loop of ``Trainer.fit`` (stage, use_staged, stage the next, fit_current) through ``ShardedLoader`` with --loaders 4
  (c) the same loop through ``ResidentLoader``
and, by HIP events on the prefetch stream with nothing else running, ifcbk_roi_gather alone (``ResidentSet.cut``) and the whole
``stage_resident_batch`` (cut + resize + targets).  Prints one JSON line.

    python scripts/resident_bench.py [--files 3072] [--epochs 3] [--steps 30] [--loaders 4]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_tree(root, files, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    dims = np.clip(np.exp(rng.normal(np.log(64.0), 0.7, (files, 2))), 8, 640).astype(int)
    for c in range(4):
        os.makedirs(os.path.join(root, 'class%d' % c))
    for i, (h, w) in enumerate(dims):
        a = np.clip(rng.normal(110 + 20 * (i % 4), 35, (h, w)), 0, 255).astype(np.uint8)
        Image.fromarray(a, 'L').save(os.path.join(root, 'class%d' % (i % 4), 'roi_%05d.png' % i))
    return dims


def train_epoch(trainer_cls, model, loader, tf):
    """the train loop of Trainer.fit; -> images staged"""
    n_next, images = None, 0
    for (rois, targets, paths), nxt in trainer_cls._lookahead(loader):
        n = trainer_cls._stage(model, rois, tf, targets, train=True) if n_next is None else n_next
        model.use_staged()
        n_next = trainer_cls._stage(model, nxt[0], tf, nxt[1], train=True) if nxt is not None else None
        model.fit_current(n)
        images += n
    return images


def timed_epochs(trainer_cls, model, loader, tf, epochs):
    rates = []
    for e in range(epochs + 1):
        loader.set_epoch(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        images = train_epoch(trainer_cls, model, loader, tf)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if e:
            rates.append(images / dt)
    return rates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=3072)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--loaders', type=int, default=4)
    ap.add_argument('--batch', type=int, default=256)
    a = ap.parse_args()
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import NeustonDataset, ResidentSet, RoiTransform
    from ifcb_classifier_amd.neuston_models import NeustonModel
    out = dict(model='inception_v3', precision='bf16', batch=a.batch, files=a.files, loaders=a.loaders, device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as root:
        dims = write_tree(root, a.files)
        out['roi_bytes_mean'] = float((dims[:, 0] * dims[:, 1]).mean())
        ds = NeustonDataset(root)
        tf = RoiTransform(299, None, True, True)
        ds.transforms = tf
        hp = argparse.Namespace(MODEL='inception_v3', classes=ds.classes, pretrained=False, batch_size=a.batch, precision='bf16', model_id='bench',
                                resize=299, img_norm=None, seed=0)
        torch.manual_seed(0)
        model = NeustonModel(hp, max_batch=a.batch)
        eng = model.model.engine
        t0 = time.perf_counter()
        res = ResidentSet.build(ds, a.loaders)
        out['build_s'] = round(time.perf_counter() - t0, 3)
        res.to_device(eng.dev, eng.prefetch_stream())
        out['resident_bytes'] = res.nbytes
        files = nn_.ShardedLoader(ds, a.batch, True, a.loaders, 0, 1, 0)
        resident = nn_.ResidentLoader(ds, res, a.batch, True, 0, 1, 0)
        # (a) bare step on one loaded batch
        idx, bounds = resident.host_batches()
        first = next(iter(resident))
        n = nn_.Trainer._stage(model, first[0], tf, first[1], train=True)
        model.use_staged()
        model.model.train()
        bare = []
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                eng.train_step(n)
            torch.cuda.synchronize()
            if rep:                                                  # (the first repeat warms up: plans, graphs, clocks)
                bare.append(n * a.steps / (time.perf_counter() - t0))
        out['a_bare_step_img_s'] = [round(v, 1) for v in bare]
        # (b) and (c), interleaved order c, b, c: the resident loop on both sides of the file loop
        c1 = timed_epochs(nn_.Trainer, model, resident, tf, a.epochs)
        b = timed_epochs(nn_.Trainer, model, files, tf, a.epochs)
        c2 = timed_epochs(nn_.Trainer, model, resident, tf, a.epochs)
        out['b_files_img_s'] = [round(v, 1) for v in b]
        out['c_resident_img_s'] = [round(v, 1) for v in c1 + c2]
        out['c_over_b'] = round(statistics.median(c1 + c2) / statistics.median(b), 2)
        out['c_over_a'] = round(statistics.median(c1 + c2) / statistics.median(bare), 3)
        # staging alone, by events on the prefetch stream
        side = eng.prefetch_stream()
        torch.cuda.synchronize()
        gather_ms, stage_ms = [], []
        for k in range(24):
            i0, i1 = bounds[k % (len(bounds) - 1)]
            part = idx[i0:i1]
            with torch.cuda.stream(side):
                idx_dev = torch.from_numpy(part).to(eng.dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                kw = res.cut(eng.pre_ctx, idx_dev, part, side)
                e1.record(side)
            side.synchronize()
            gather_ms.append(e0.elapsed_time(e1))
            out['batch_bytes'] = int(kw['pixels'].numel())
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record(side)
            model.stage_resident_batch(res, idx_dev, part, tf, train=True)
            s1.record(side)
            side.synchronize()
            model.use_staged()
            stage_ms.append(s0.elapsed_time(s1))
        out['gather_ms'] = dict(median=round(statistics.median(gather_ms[4:]), 4), min=round(min(gather_ms[4:]), 4), max=round(max(gather_ms[4:]), 4))
        out['stage_resident_ms'] = dict(median=round(statistics.median(stage_ms[4:]), 4), min=round(min(stage_ms[4:]), 4), max=round(max(stage_ms[4:]), 4))
        out['step_ms'] = round(1000.0 * n / statistics.median(bare), 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
