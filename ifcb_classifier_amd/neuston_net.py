#!/usr/bin/env python
"""``neuston_net.py TRAIN|RUN`` on the MI355X path -- same command line as ``/root/reference/neuston_net.py``
(:311-413: global ``--batch/--loaders`` before the sub-command, every TRAIN / RUN flag with its default), same
outputs ({model_id}.ptl, epochs.csv, args.yml, training/validation image lists, results files, per-bin class
files), with Lightning's Trainer replaced by the small explicit loop below (fit: :101-115, test: :192-308).

Data parallel: launch one process per GPU with ``python -m torch.distributed.run --nproc-per-node N -m
ifcb_classifier_amd.neuston_net ... TRAIN ...``; ``--batch`` stays per GPU (as under the reference's
ddp_spawn), gradients are averaged over RCCL, BatchNorm statistics stay per rank, rank 0 writes the files.
"""
import argparse
import contextlib
import csv
import datetime as dt
import os
import random
from shutil import copyfile

import numpy as np
import torch
from torch.utils.data import DataLoader

from .neuston_callbacks import SaveValidationResults, SaveTestResults
from .neuston_data import (get_trainval_datasets, IfcbBinDataset, ImageDataset, IMG_EXTENSIONS, collate_rois,
                           blur_arg, blur_prob_arg, jitter_arg, mix_alpha_arg, mix_prob_arg, pad_arg, rois_to_device)
from .neuston_models import NeustonModel, check_teacher_classes, load_checkpoint_file, load_pretrained_weights


def seed_everything(seed=None):
    """[PL] seed_everything: None -> draw a seed, record it (neuston_net.py:62)."""
    if seed is None:
        seed = random.SystemRandom().randint(0, 2 ** 32 - 1)
    seed = int(seed)
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)
    os.environ['PL_GLOBAL_SEED'] = str(seed)
    return seed


def class_norm_weights(counts, power):
    """``--class-norm POWER``: per-class loss weights w_c = Z * n_c ** -POWER from the per-class counts n_c of the training split, with
    Z = sum n_c / sum n_c ** (1 - POWER), so that sum_c n_c * w_c == sum_c n_c: the mean weight over the training samples is 1.
    POWER = 1 is the "balanced" weighting N / (C * n_c), POWER = 0 all ones.  Computed in float64, rounded once to float32; returned
    as a list of python floats holding exactly those float32 values.  A class without a training sample gets weight 0 (it cannot
    occur as a training target) and stays out of both sums."""
    power = float(power)
    if power < 0:
        raise ValueError('class-norm POWER must be >= 0')
    n = [float(c) for c in counts]
    if not any(c > 0 for c in n):
        raise ValueError('class-norm: the training split is empty')
    z = sum(n) / sum(c ** (1.0 - power) for c in n if c > 0)
    w64 = [z * c ** -power if c > 0 else 0.0 for c in n]
    return [float(v) for v in np.asarray(w64, dtype=np.float64).astype(np.float32)]


def _class_norm_power(text):
    v = float(text)
    if not v >= 0:
        raise argparse.ArgumentTypeError('POWER must be >= 0, got %r' % text)
    return v


def _label_smoothing(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:                    # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('EPS must be in [0, 1], got %r' % text)
    return v


def _focal_gamma(text):
    v = float(text)
    if not 0.0 <= v < float('inf'):            # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('GAMMA must be finite and not negative, got %r' % text)
    return v


def _distill_alpha(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:                    # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('A must be in [0, 1], got %r' % text)
    return v


def _distill_temperature(text):
    v = float(text)
    if not 0.0 < v < float('inf'):             # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('T must be finite and > 0, got %r' % text)
    return v


def _ema_decay(text):
    v = float(text)
    if not 0.0 < v < 1.0:                      # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('DECAY must be in (0, 1), got %r' % text)
    return v


def _clip_grad(text):
    v = float(text)
    if not 0.0 < v < float('inf'):             # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('NORM must be finite and > 0, got %r' % text)
    return v


def _lr_nonneg(text):
    v = float(text)
    if not 0.0 <= v < float('inf'):            # (nan fails both comparisons)
        raise argparse.ArgumentTypeError('must be finite and not negative, got %r' % text)
    return v


def _accumulate(text):
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError('K must be an integer >= 1, got %r' % text) from None
    if v < 1:
        raise argparse.ArgumentTypeError('K must be an integer >= 1, got %r' % text)
    return v


def check_accumulate(k, batches_per_epoch):
    """TRAIN --accumulate K beyond the training batches of an epoch (per GPU) is a usage error: no window would ever fill"""
    if k > batches_per_epoch:
        argparse_nn().error('TRAIN --accumulate {} is more than the {} training batch(es) of an epoch: use a K <= {} or a smaller '
                            '--batch'.format(k, batches_per_epoch, batches_per_epoch))


def check_lr_flags(args):
    """the combinations of --lr-schedule / --warmup / --lr-min / --learning-rate / --emax that TRAIN refuses, each with its message"""
    kind, warmup, lr_min = args.lr_schedule, args.warmup, args.lr_min
    if lr_min > args.learning_rate:
        raise SystemExit('TRAIN --lr-min {:g} is above --learning-rate {:g}: the rate decays from the latter to the former'.format(
            lr_min, args.learning_rate))
    if warmup and warmup >= args.emax:
        raise SystemExit('TRAIN --warmup {:g} must be less than --emax {}: the warm-up would take the whole run'.format(warmup, args.emax))
    if kind == 'constant' and lr_min:
        raise SystemExit('TRAIN --lr-min {:g} needs a decaying --lr-schedule (cosine or linear): a constant rate never gets there '
                         '(--warmup alone into a constant rate is fine)'.format(lr_min))


class _ExclusiveLossScalar(argparse.Action):
    """stores --label-smoothing / --focal-gamma (and --mixup / --cutmix / --distill); the second of the two to arrive non-zero is an
    argparse error naming both, as is --focal-gamma, --mixup or --cutmix beside --distill"""
    FLAGS = {'label_smoothing': '--label-smoothing', 'focal_gamma': '--focal-gamma'}

    def __call__(self, parser, namespace, value, option_string=None):
        setattr(namespace, self.dest, value)
        if all(getattr(namespace, d, 0.0) for d in self.FLAGS):
            parser.error('%s and %s do not combine: give one of them' % tuple(sorted(self.FLAGS.values(), reverse=True)))
        # batch mixing (--mixup / --cutmix) has a two-target loss of its own, which has no focal form
        if getattr(namespace, 'focal_gamma', 0.0):
            for d, flag in (('mixup', '--mixup'), ('cutmix', '--cutmix')):
                if getattr(namespace, d, 0.0):
                    parser.error('%s and --focal-gamma do not combine: give one of them' % flag)
        # distillation (--distill, stored through this action as well) has a loss kernel of its own, without a focal or a two-target form
        if getattr(namespace, 'distill', None):
            for d, flag in (('focal_gamma', '--focal-gamma'), ('mixup', '--mixup'), ('cutmix', '--cutmix')):
                if getattr(namespace, d, 0.0):
                    parser.error('%s and --distill do not combine: give one of them' % flag)


def _dist():
    import torch.distributed as dist
    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        if not dist.is_initialized():
            local = int(os.environ.get('LOCAL_RANK', 0))
            if torch.cuda.is_available():
                torch.cuda.set_device(local)
                dist.init_process_group('nccl', device_id=torch.device('cuda', local))
            else:
                dist.init_process_group('gloo')
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


class ShardedLoader:
    """per-rank view of a dataset order (what [PL]'s auto DistributedSampler does): a seeded permutation per epoch
    (train) or the natural order (val), padded by wrap-around to a multiple of world, strided by rank."""

    def __init__(self, dataset, batch_size, shuffle, num_workers, rank, world, seed):
        self.dataset, self.bs, self.shuffle, self.nw = dataset, batch_size, shuffle, num_workers
        self.rank, self.world, self.seed, self.epoch = rank, world, seed, 0

    def set_epoch(self, e):
        self.epoch = e

    def indices(self):
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        if self.world > 1:
            total = (n + self.world - 1) // self.world * self.world
            idx = (idx + idx[:total - n])[self.rank:total:self.world]
        return idx

    def __iter__(self):
        sub = torch.utils.data.Subset(self.dataset, self.indices())
        return iter(DataLoader(sub, batch_size=self.bs, shuffle=False, pin_memory=True, num_workers=self.nw,
                               collate_fn=collate_rois))

    def __len__(self):
        return (len(self.indices()) + self.bs - 1) // self.bs


class ResidentBatch:
    """what a ``ResidentLoader`` yields in the place of a collated ROI batch: the set and the batch's indices, on the device and on the host"""

    def __init__(self, res, idx_dev, idx_host):
        self.res, self.idx_dev, self.idx_host = res, idx_dev, idx_host


class ResidentLoader(ShardedLoader):
    """TRAIN --resident: the same order as ``ShardedLoader`` (``indices()`` is inherited: seed, epoch, rank, world and wrap-around), but
    nothing is decoded, collated or uploaded per batch.  ``res`` is the dataset's ``neuston_data.ResidentSet``, on the device; the
    epoch's index vector goes up once per epoch, on the set's stream, and the batches are slices of it.  Yields
    (ResidentBatch, targets, paths) where ``ShardedLoader`` yields (rois, targets, paths); the short last batch is the same."""

    def __init__(self, dataset, res, batch_size, shuffle, rank, world, seed):
        super().__init__(dataset, batch_size, shuffle, 0, rank, world, seed)
        if len(res) != len(dataset):
            raise ValueError('ResidentLoader: the resident set holds %d ROIs, the dataset %d' % (len(res), len(dataset)))
        self.res = res

    def host_batches(self):
        """-> (the epoch's index vector, int64; the (start, stop) bounds of its batches)"""
        idx = self.res.check_indices(self.indices())
        return idx, [(i, min(i + self.bs, len(idx))) for i in range(0, len(idx), self.bs)]

    def __iter__(self):
        res = self.res
        idx, bounds = self.host_batches()
        with torch.cuda.stream(res.stream):
            idx_dev = torch.from_numpy(idx).pin_memory().to(res.dev['pixels'].device, non_blocking=True)
        for i0, i1 in bounds:
            part = idx[i0:i1]
            yield (ResidentBatch(res, idx_dev[i0:i1], part), torch.from_numpy(res.targets[part]), [res.paths[j] for j in part])


class Trainer:
    """fit/test loops with [PL] 1.3.8's observable semantics for this driver: num_sanity_val_steps=0; per epoch
    train -> validate -> callbacks; ModelCheckpoint(monitor=val_loss, top-1); EarlyStopping(val_loss, patience)
    honoured only after min_epochs; CSV log of scalar metrics."""

    def __init__(self, max_epochs, min_epochs, estop, outdir, callbacks=()):
        self.max_epochs, self.min_epochs, self.estop = max_epochs, min_epochs, estop
        self.outdir, self.callbacks = outdir, list(callbacks)
        self.metrics = []
        self.best_model_path = None
        self.dist, self.rank, self.world = _dist()
        self.tta = None                   # RUN --tta: 'flips' / 'all' -- the test loops average each batch's scores over symmetry views

    def _scores(self, model, n):
        """the class scores of the current batch of the test loops: plain, or (RUN --tta) the mean over the views"""
        if self.tta is None:
            return model.eval_current(n)[0]
        return model.eval_current_tta(n, self.tta)

    @staticmethod
    def _lookahead(loader):
        """(batch, next batch or None) pairs: the next batch is staged on the GPU's side stream while the current one runs"""
        it = iter(loader)
        cur = next(it, None)
        while cur is not None:
            nxt = next(it, None)
            yield cur, nxt
            cur = nxt

    @staticmethod
    def _stage(model, rois, transform, targets, train=False):
        """stage one batch of ``fit``'s loaders: a collated batch is uploaded, a ``ResidentBatch`` (TRAIN --resident) is cut on the device"""
        if isinstance(rois, ResidentBatch):
            return model.stage_resident_batch(rois.res, rois.idx_dev, rois.idx_host, transform, train=train)
        if train:
            return model.stage_batch(rois, transform, targets, train=True)
        return model.stage_batch(rois, transform, targets)

    def _allreduce(self, t):
        # the bucket exchange: one all_reduce, or reduce-scatter + all-gather (IFCBK_DP_EXCHANGE=allreduce|rsag, dp.make_exchange)
        if getattr(self, '_exchange', None) is None:
            from .dp import make_exchange
            self._exchange, self.exchange_mode = make_exchange(self.dist)
        return self._exchange(t)

    def fit(self, model, train_loader, val_loader):
        dev = model.model.engine.dev
        eng = model.model.engine
        if self.world > 1:
            self.dist.broadcast(eng.P, 0)
            self.dist.broadcast(eng.RB, 0)
            eng.params_changed()
        chk = os.path.join(self.outdir, 'chkpts')
        best, wait, global_step = np.inf, 0, 0
        for epoch in range(self.max_epochs):
            model.current_epoch = epoch
            train_loader.set_epoch(epoch)
            ttf, vtf = train_loader.dataset.transforms, val_loader.dataset.transforms
            # one batch of look-ahead: upload + on-GPU preprocessing of batch k+1 run on a side stream beside step k
            n_next = None
            epoch_steps = 0
            for (rois, targets, paths), nxt in self._lookahead(train_loader):
                n = self._stage(model, rois, ttf, targets, train=True) if n_next is None else n_next
                model.use_staged()
                n_next = self._stage(model, nxt[0], ttf, nxt[1], train=True) if nxt is not None else None
                done = eng.step_count
                model.fit_current(n, self.world, self._allreduce if self.world > 1 else None)
                # (TRAIN --accumulate K: the engine steps once per K batches; global_step and the clip report count optimizer steps)
                global_step += eng.step_count - done
                epoch_steps += eng.step_count - done
            if model.fit_flush(self.world, self._allreduce if self.world > 1 else None):       # an epoch's short last window
                global_step += 1
                epoch_steps += 1
            model.agg_train_loss = model.epoch_train_loss()
            # TRAIN --clip-grad: the epoch's report, read where the loss sum is read (the epoch's one wait on the device) and restarted.
            # Data parallel: every rank clips the same averaged gradient by the same norm, so rank 0 speaks for all
            clip = model.epoch_clip_stats()
            if clip is not None and self.rank == 0:
                print('Epoch {}: largest gradient norm before clipping {:.4g} (--clip-grad {:g}): clipped {} of {} steps'.format(
                    epoch, clip[0], model.clip_grad, clip[1], epoch_steps))
            # TRAIN --ema: the averaged model stands in P / RB from here to the checkpoint -- val_loss, F1 and the results files, early
            # stopping, the choice of the best epoch and the state_dict saved for it are the averaged model's; training goes on from the
            # raw weights.  Data parallel: every rank holds the same P after the exchange, so the same average; it is never communicated
            with (eng.ema_weights() if getattr(eng, 'ema_decay', None) is not None else contextlib.nullcontext()):
                steps = []
                n_next = None
                for (rois, targets, paths), nxt in self._lookahead(val_loader):
                    n = self._stage(model, rois, vtf, targets) if n_next is None else n_next
                    model.use_staged()
                    n_next = self._stage(model, nxt[0], vtf, nxt[1]) if nxt is not None else None
                    probs, loss = model.eval_current(n, with_loss=True)
                    tg = targets.to(dev, non_blocking=True)
                    steps.append(dict(val_batch_loss=loss, val_outputs=probs, val_input_classes=tg, val_input_srcs=list(paths)))
                steps = self._gather_val(steps, len(val_loader.dataset))
                stop = False
                if self.rank == 0:
                    model.validation_epoch_end(steps)
                    log = model.logged
                    self.metrics.append({k: (float(v) if not isinstance(v, bool) else v) for k, v in log.items()
                                         if k not in ('input_classes', 'output_classes', 'input_srcs', 'outputs')})
                    for cb in self.callbacks:
                        cb.on_validation_end(log, model, train_loader.dataset, val_loader.dataset)
                    if log['val_loss'] < best:
                        best, wait = log['val_loss'], 0
                        if self.world > 1:
                            pass                                  # rank-0 BN buffers win (DDP broadcast_buffers)
                        os.makedirs(chk, exist_ok=True)
                        path = os.path.join(chk, 'epoch={}-step={}.ckpt'.format(epoch, global_step - 1))
                        torch.save(model.checkpoint_dict(epoch, global_step), path)
                        if self.best_model_path and os.path.exists(self.best_model_path) and self.best_model_path != path:
                            os.remove(self.best_model_path)
                        self.best_model_path = path
                    else:
                        wait += 1
                    stop = bool(self.estop and wait >= self.estop and epoch + 1 >= self.min_epochs)
            if self.world > 1:
                flag = torch.tensor([1 if stop else 0], device=dev)
                self.dist.broadcast(flag, 0)
                stop = bool(flag.item())
            if stop:
                break

    def _gather_val(self, steps, n_total):
        """rank 0 receives every rank's validation outputs (the reference's epoch-end aggregation sees only the
        local shard under ddp: SURVEY.md §5); wrap-around padding is dropped."""
        if self.world == 1:
            return steps
        payload = [dict(val_batch_loss=s['val_batch_loss'].item(), val_outputs=s['val_outputs'].cpu(),
                        val_input_classes=s['val_input_classes'].cpu(), val_input_srcs=s['val_input_srcs']) for s in steps]
        gathered = [None] * self.world if self.rank == 0 else None
        self.dist.gather_object(payload, gathered, dst=0)
        if self.rank != 0:
            return []
        out, seen = [], set()
        for part in gathered:
            for s in part:
                keep = [i for i, p in enumerate(s['val_input_srcs']) if p not in seen]
                seen.update(s['val_input_srcs'])
                if not keep:
                    continue
                out.append(dict(val_batch_loss=torch.tensor(s['val_batch_loss']), val_outputs=s['val_outputs'][keep],
                                val_input_classes=s['val_input_classes'][keep],
                                val_input_srcs=[s['val_input_srcs'][i] for i in keep]))
        return out

    def test(self, model, loader, input_obj, transform, callbacks):
        dev = model.model.engine.dev
        steps = []
        n_next = None
        for (rois, ids), nxt in self._lookahead(loader):
            n = model.stage_batch(rois, transform) if n_next is None else n_next
            model.use_staged()
            n_next = model.stage_batch(nxt[0], transform) if nxt is not None else None
            probs = self._scores(model, n)
            steps.append(dict(test_outputs=probs, test_srcs=list(ids)))
        rr = model.test_epoch_end(steps, input_obj)
        rr.type = 'Bin' if hasattr(input_obj, 'yearday') else 'ImgDir'
        written = []
        for cb in callbacks:
            written += cb.on_test_end(rr, model)
        return rr, written

    def test_resident(self, model, bin_fileset, ds, input_obj, callbacks, batch_size):
        """RUN on one raw bin the way SURVEY 8 f-3 means it (reference data path: neuston_data.py:433-467, one PIL image per
        ROI through DataLoader workers): the .adc was read ONCE into an offset / size table, the .roi blob is uploaded ONCE, and
        every batch of the bin is preprocessed on the GPU straight from that resident blob (ifcbk_roi_preprocess takes absolute
        byte offsets) -- no per-ROI slicing, no per-batch concatenation or upload.  Same scores as ``test`` over a DataLoader of
        the bin, bit for bit."""
        t = bin_fileset.table
        res = model.upload_bin(bin_fileset.blob, t['offs'], t['hs'], t['ws'])
        n_total = len(t['targets'])
        bounds = [(i, min(i + batch_size, n_total)) for i in range(0, n_total, batch_size)]
        steps, n_next = [], None
        for k, (i0, i1) in enumerate(bounds):
            n = model.stage_resident(res, i0, i1, ds.transform) if n_next is None else n_next
            model.use_staged()
            n_next = model.stage_resident(res, bounds[k + 1][0], bounds[k + 1][1], ds.transform) if k + 1 < len(bounds) else None
            probs = self._scores(model, n)
            steps.append(dict(test_outputs=probs, test_srcs=list(ds.pids[i0:i1])))
        rr = model.test_epoch_end(steps, input_obj)
        rr.type = 'Bin'
        written = []
        for cb in callbacks:
            written += cb.on_test_end(rr, model)
        return rr, written

    def test_many(self, model, bins, batch_size, num_workers, callbacks):
        """--gobig: classify the ROIs of all ``bins`` [(pid, IfcbBinDataset)] as one stream of full batches, then write one
        result set per bin (the per-bin files are the same as without --gobig: an image's scores do not depend on its batch)."""
        dev = model.model.engine.dev
        cat = torch.utils.data.ConcatDataset([ds for _, ds in bins])
        loader = DataLoader(cat, batch_size=batch_size, pin_memory=True, num_workers=num_workers, collate_fn=collate_rois)
        probs, ids = [], []
        tf, n_next = bins[0][1].transform, None
        for (rois, pids), nxt in self._lookahead(loader):
            n = model.stage_batch(rois, tf) if n_next is None else n_next
            model.use_staged()
            n_next = model.stage_batch(nxt[0], tf) if nxt is not None else None
            p = self._scores(model, n)
            probs.append(p)
            ids.extend(pids)
        probs = torch.cat(probs, 0).detach().cpu().numpy()
        written, lo = [], 0
        for bin_obj, ds in bins:
            hi = lo + len(ds)
            rr = model.RunResults(inputs=ids[lo:hi], outputs=probs[lo:hi], input_obj=bin_obj)
            rr.type = 'Bin'
            model.logged = dict(RunResults=[rr])
            for cb in callbacks:
                written += cb.on_test_end(rr, model)
            lo = hi
        return written

    def write_metrics_csv(self, path):
        keys = []
        for m in self.metrics:
            for k in m:
                if k not in keys:
                    keys.append(k)
        with open(path, 'w', newline='') as f:
            w = csv.DictWriter(f, fieldnames=keys)
            w.writeheader()
            w.writerows(self.metrics)


def main(args):
    if args.cmd_mode == 'TRAIN':
        do_training(args)
    else:
        do_run(args)
    print('\nDONE!')


def do_training(args):
    date_str = args.cmd_timestamp.split('T')[0]
    args.model_id = args.model_id.format(TRAIN_DATE=date_str, TRAIN_ID=args.TRAIN_ID)
    os.makedirs(args.outdir, exist_ok=True)
    if not args.result_files:
        args.result_files = ['results.mat training_image_basenames training_classes image_basenames input_classes '
                             'output_scores confusion_matrix counts_perclass f1_perclass f1_weighted f1_macro'.split()]
    callbacks = [SaveValidationResults(outdir=args.outdir, outfile=rf[0], series=rf[1:]) for rf in args.result_files]
    check_lr_flags(args)
    args.seed = seed_everything(args.seed or None)
    if getattr(args, 'blur', None) is None:
        # unset: the model file and args.yml carry no blur entry at all
        for k in ('blur', 'blur_prob'):
            if hasattr(args, k):
                delattr(args, k)
    elif getattr(args, 'distill', None):
        raise SystemExit('TRAIN --blur and --distill do not combine: the teacher resizes the ROIs itself, at its own input side, and '
                         'would see sharp images where the student sees blurred ones; blurring the teacher\'s batch alike is not implemented')

    training_dataset, validation_dataset = get_trainval_datasets(args)
    assert training_dataset.classes == validation_dataset.classes
    args.classes = training_dataset.classes
    args.class_weights = None
    if args.class_norm is not None:
        # counts of the whole training split (before any data-parallel sharding: every rank holds the same weights), args.classes order
        args.class_weights = class_norm_weights(training_dataset.count_perclass, args.class_norm)
        lo = min(range(len(args.classes)), key=lambda c: args.class_weights[c])
        hi = max(range(len(args.classes)), key=lambda c: args.class_weights[c])
        print('Class-norm POWER {:g}: loss weights from {:.4g} ({}) to {:.4g} ({})'.format(
            args.class_norm, args.class_weights[lo], args.classes[lo], args.class_weights[hi], args.classes[hi]))
    if args.distill:
        # the teacher's class list is checked from its file's hyper-parameters alone, before anything is built or trained
        thp = load_checkpoint_file(args.distill)['hyper_parameters']
        try:
            check_teacher_classes(args.classes, thp['classes'])
        except ValueError as e:
            raise SystemExit('TRAIN {}'.format(e))
        args.distill_teacher_id = thp.get('model_id')
    else:
        # unset: the model file and args.yml carry no distillation entry at all
        del args.distill, args.distill_alpha, args.distill_temperature
    resident = resident_flag(args)
    dist, rank, world = _dist()
    if rank == 0:
        with open(os.path.join(args.outdir, 'training_images.list'), 'w') as f:
            f.write('\n'.join(sorted(training_dataset.images)))
        with open(os.path.join(args.outdir, 'validation_images.list'), 'w') as f:
            f.write('\n'.join(sorted(validation_dataset.images)))
    print('Loading Training Dataloader...')
    training_loader = ShardedLoader(training_dataset, args.batch_size, True, args.loaders, rank, world, args.seed)
    print('Loading Validation Dataloader...')
    validation_loader = ShardedLoader(validation_dataset, args.batch_size, False, args.loaders, rank, world, args.seed)
    check_accumulate(args.accumulate, len(training_loader))

    if args.pretrained and not getattr(args, 'weights', None):
        # upstream: pretrained=True downloads torchvision's ImageNet weights (neuston_models.py:23-42).  Training from random
        # initialisation instead would silently change the experiment, so refuse.
        raise SystemExit('TRAIN without --untrain fine-tunes ImageNet weights upstream (torchvision download); this path has no '
                         'network and no torchvision: pass --weights <torchvision state_dict .pth> (or set '
                         'IFCBK_PRETRAINED_WEIGHTS), or add --untrain to train from random initialisation')
    trainer = Trainer(args.emax, args.emin, args.estop, args.outdir, callbacks)
    hp = argparse.Namespace(**{k: v for k, v in vars(args).items()})
    classifier = NeustonModel(hp, device=int(os.environ.get('LOCAL_RANK', 0)), max_batch=args.batch_size)
    if args.pretrained:
        loaded, skipped = load_pretrained_weights(classifier.model, args.weights)
        print('Loaded {} pretrained tensors from {}; freshly initialised: {}'.format(
            len(loaded), args.weights, [k for k in skipped if not k.endswith('num_batches_tracked')]))
    if getattr(args, 'distill', None):
        # loaded as RUN loads a model: activations for a training batch, gradient-side buffers for one image
        teacher = NeustonModel.load_from_checkpoint(args.distill, device=int(os.environ.get('LOCAL_RANK', 0)),
                                                    max_batch=args.batch_size, inference=True)
        if teacher.model.engine.max_batch < args.batch_size:
            raise SystemExit('TRAIN --distill: the teacher ({}) holds {} images per program, --batch is {}'.format(
                teacher.hparams.MODEL, teacher.model.engine.max_batch, args.batch_size))
        classifier.attach_teacher(teacher)
        print('Distilling from {} ({}, {} classes): alpha {:g}, temperature {:g}'.format(
            args.distill, teacher.hparams.MODEL, len(teacher.hparams.classes), args.distill_alpha, args.distill_temperature))
    if resident:
        training_loader, validation_loader = resident_loaders(classifier, training_loader, validation_loader, args.loaders)
    eng = classifier.model.engine
    if eng.window_batch < args.batch_size:
        # --batch is per GPU as upstream (neuston_net.py:102); BatchNorm statistics are per step, so a step cannot be chunked
        raise ValueError('--batch %d: one launch addresses each tensor through a 2 GiB buffer descriptor, which holds %d images '
                         'of %s; use --batch <= %d per GPU (and more GPUs for a larger global batch), or --accumulate K for an '
                         'effective batch of K times --batch on the same GPUs'
                         % (args.batch_size, eng.window_batch, args.MODEL, eng.window_batch))
    # --accumulate K: one optimizer step per K training batches, and one more for an epoch's short last window
    steps_per_epoch = classifier.optimizer_steps(len(training_loader))
    if args.accumulate > 1:
        print('Accumulating gradients over {} batches: effective batch {} ({} x {} x {} GPU(s)), {} optimizer steps per epoch'.format(
            args.accumulate, args.batch_size * args.accumulate * world, args.batch_size, args.accumulate, world, steps_per_epoch))
    # --lr-schedule / --warmup: the optimizer steps of an epoch -- the per-rank length of the training loader (--resident: the same
    # length), over --accumulate -- times --emax is the run
    sched = classifier.set_lr_schedule(steps_per_epoch)
    if sched is not None:
        print('Learning rate: {} schedule over {} steps, {} of them warm-up, from {:g} to {:g}'.format(
            sched.kind, sched.total_steps, sched.warmup_steps, sched.base, sched.base if sched.kind == 'constant' else sched.lr_min))
    trainer.fit(classifier, training_loader, validation_loader)
    if rank != 0:
        return
    output_path = os.path.join(args.outdir, args.model_id + '.ptl')
    copyfile(trainer.best_model_path, output_path)
    if args.epochs_log:
        trainer.write_metrics_csv(os.path.join(args.outdir, args.epochs_log))
    if args.args_log:
        import yaml
        with open(os.path.join(args.outdir, args.args_log), 'w') as f:
            yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v))
                            for k, v in vars(args).items()}, f)
    if args.onnx:
        # upstream exports its in-memory classifier as fit left it (not the best checkpoint); at the 224 pixels these backbones
        # train at, where upstream's dummy input says 244
        from . import onnx_export
        output_path_onnx = os.path.join(args.outdir, args.model_id + '.onnx')
        # (TRAIN --ema: the averaged model, as the checkpoint holds)
        sd = classifier.model.state_dict(ema=True) if classifier.ema is not None else classifier.model.state_dict()
        onnx_export.export(sd, args.MODEL, args.classes, args.pretrained, output_path_onnx, pad=args.pad)
        print('EXPORTED:', output_path_onnx)
        onnx_export.write_classes(output_path_onnx + '.classes', args.classes)
        print('EXPORTED:', output_path_onnx + '.classes')


def resident_flag(args):
    """TRAIN --resident as ``do_training`` reads it: set, it stays in ``args`` (so in args.yml and the model file's hyper_parameters);
    unset, the entry is removed and neither file carries one -- their bytes are those of a run before the flag existed"""
    on = bool(getattr(args, 'resident', False))
    if not on and hasattr(args, 'resident'):
        del args.resident
    return on


def resident_loaders(classifier, training_loader, validation_loader, loaders):
    """TRAIN --resident: decode both sets once, check that they fit the memory the GPU has left now that the engine (and a teacher) is
    built, upload them on the engine's prefetch stream and return the two loaders that cut their batches there.  No fallback: sets
    that do not fit end TRAIN.  Data parallel: every rank does all of this for the whole sets."""
    from .neuston_data import ResidentSet
    eng = classifier.model.engine
    print('Decoding the Training and Validation images once (--resident)...')
    sets = [ResidentSet.build(ld.dataset, loaders) for ld in (training_loader, validation_loader)]
    free, _ = torch.cuda.mem_get_info(eng.dev)
    need = sum(s.nbytes for s in sets)
    if need > free:
        raise SystemExit('TRAIN --resident: the training set ({:,} bytes of ROIs and tables) and the validation set ({:,} bytes) need '
                         '{:,} bytes on the GPU, which has {:,} bytes free beside the model: train without --resident'.format(
                             sets[0].nbytes, sets[1].nbytes, need, free))
    stream = eng.prefetch_stream()
    out = []
    for s, ld in zip(sets, (training_loader, validation_loader)):
        s.to_device(eng.dev, stream)
        out.append(ResidentLoader(ld.dataset, s, ld.bs, ld.shuffle, ld.rank, ld.world, ld.seed))
    print('Resident: {} + {} ROIs, {:,} bytes, {} channel(s)'.format(len(sets[0]), len(sets[1]), need, sets[0].in_channels))
    return out


class _ImgSource:
    def __init__(self, src):
        self.src = src


def do_run(args):
    if args.filter:
        if args.filter[0] not in ['IN', 'OUT']:
            raise argparse.ArgumentTypeError('IN|OUT must be either "IN" or "OUT"')
        if len(args.filter) < 2:
            raise argparse.ArgumentTypeError('Must be at least one KEYWORD')
    classifier = NeustonModel.load_from_checkpoint(args.MODEL, device=int(os.environ.get('LOCAL_RANK', 0)),
                                                   max_batch=args.batch_size, inference=True)
    if args.batch_size > classifier.model.engine.max_batch:
        args.batch_size = classifier.model.engine.max_batch          # per-image results: a smaller program batch changes nothing
    seed_everything(classifier.hparams.seed)
    run_pad = getattr(classifier.hparams, 'pad', None)       # the geometry the model was trained on; absent in older files: squash
    # (a RUN batch beyond the 2 GiB buffer-descriptor window needs nothing here: results are per image, and the library cuts the
    #  convolutions of such a batch into launches over image groups)
    if os.path.isdir(args.SRC) and not args.SRC.endswith(os.sep):
        args.SRC = args.SRC + os.sep
    if not args.outfile:
        args.outfile = ['D{BIN_YEAR}/D{BIN_DATE}/{BIN_ID}_class.h5'] if args.src_type == 'bin' else ['img_results.json']
    if any(o.endswith('.h5') for o in args.outfile):
        try:
            import h5py  # noqa: F401
        except ImportError:
            raise SystemExit('RUN: outfile(s) {} need h5py, which is not installed in this environment (the default class file is '
                             '.h5, neuston_net.py:181): install h5py or pass --outfile with a .mat / .json name'.format(
                                 [o for o in args.outfile if o.endswith('.h5')]))
    callbacks = [SaveTestResults(outdir=args.outdir, outfile=o, timestamp=args.cmd_timestamp) for o in args.outfile]
    trainer = Trainer(0, 0, 0, args.outdir)
    trainer.tta = getattr(args, 'tta', None)
    filter_mode, filter_keywords = None, []
    if args.filter:
        filter_mode = args.filter[0]
        for kw in args.filter[1:]:
            if os.path.isfile(kw):
                with open(kw) as f:
                    filter_keywords.extend(f.read().splitlines())
            else:
                filter_keywords.append(kw)

    if args.src_type == 'bin':
        from .ifcb_bins import DataDirectory
        if os.path.isdir(args.SRC):
            dd = DataDirectory(args.SRC, whitelist=filter_keywords if filter_mode == 'IN' else None,
                               blacklist=filter_keywords if filter_mode == 'OUT' else None)
        elif os.path.isfile(args.SRC) and args.SRC.endswith('.txt'):
            with open(args.SRC) as f:
                bins = f.read().splitlines()
            dd = DataDirectory(os.path.commonpath(bins), whitelist=bins)
        else:
            dd = DataDirectory(os.path.dirname(args.SRC), whitelist=[os.path.basename(args.SRC)])
        error_bins = []
        big = []          # --gobig: (bin pid, dataset) of every bin, classified together afterwards
        n_bins = 0
        dist, rank, world = _dist()
        if args.gobig:
            print('Loading Bins', end=' ')
        for i, bin_fileset in enumerate(dd):
            if world > 1 and i % world != rank:        # RUN shards bins over ranks; no collective (replicas only)
                continue
            bin_fileset.pid.namespace = os.path.dirname(bin_fileset.basepath.replace(args.SRC, '')) + os.sep
            bin_obj = bin_fileset.pid
            if args.filter:
                if filter_mode == 'IN' and not any(k in str(bin_obj) for k in filter_keywords):
                    continue
                if filter_mode == 'OUT' and any(k in str(bin_obj) for k in filter_keywords):
                    continue
            if not args.clobber:
                fmt = dict(BIN_ID=bin_obj.pid, BIN_YEAR=bin_obj.year, BIN_DATE=bin_obj.yearday, INPUT_SUBDIRS=bin_obj.namespace)
                outs = [os.path.join(args.outdir, o).format(**fmt).replace(2 * os.sep, os.sep) for o in args.outfile]
                if all(os.path.isfile(o) for o in outs):
                    print('{} result-file(s) already exist - skipping this bin'.format(bin_obj))
                    continue
            n_bins += 1
            try:
                ds = IfcbBinDataset(bin_fileset, classifier.hparams.resize, classifier.hparams.img_norm, pad=run_pad)
                if len(ds) == 0:
                    error_bins.append((bin_obj, AssertionError('Bin is Empty')))
                    continue
                if args.gobig:
                    print('.', end='', flush=True)
                    big.append((bin_obj, ds))
                    continue
                if hasattr(bin_fileset, 'table') and hasattr(bin_fileset, 'blob') and os.environ.get('IFCBK_BIN_RESIDENT', '1') != '0':
                    # one upload per bin, batches cut on the device (f-3); IFCBK_BIN_RESIDENT=0: the per-ROI DataLoader path below
                    trainer.test_resident(classifier, bin_fileset, ds, bin_obj, callbacks, args.batch_size)
                    continue
                loader = DataLoader(ds, batch_size=args.batch_size, pin_memory=True, num_workers=args.loaders,
                                    collate_fn=collate_rois)
                trainer.test(classifier, loader, bin_obj, ds.transform, callbacks)
            except Exception as e:                     # noqa: per-bin isolation as upstream (:266-268)
                error_bins.append((bin_obj, e))
        if args.gobig and big:
            # upstream hands Lightning the list of all bin loaders at once (:261-263,271).  Here "big" means what it buys on the
            # GPU: ONE stream of full fixed-size batches across bin boundaries (a bin's tail no longer runs a short batch, the
            # captured hipGraph of the batch size is replayed throughout); the scores are cut back per bin before the writers
            print()
            try:
                trainer.test_many(classifier, big, args.batch_size, args.loaders, callbacks)
            except Exception as e:                     # noqa
                error_bins.extend((b, e) for b, _ in big)
        print('RUN IS DONE')
        if error_bins:
            print('The following bins failed; they were not processed:')
            for bin_obj, err in error_bins:
                print(bin_obj, type(err), err)
            if n_bins and len(error_bins) >= n_bins:
                raise SystemExit('RUN: every one of the {} bins failed'.format(n_bins))
    else:
        img_paths = []
        if os.path.isdir(args.SRC):
            for pardir, _, imgs in os.walk(args.SRC):
                img_paths.extend(os.path.join(pardir, im) for im in imgs if im.endswith(IMG_EXTENSIONS))
        elif os.path.isfile(args.SRC) and args.SRC.endswith('.txt'):
            with open(args.SRC) as f:
                img_paths = [ln.strip() for ln in f.read().splitlines()]
            img_paths = [p for p in img_paths if p.endswith(IMG_EXTENSIONS)]
        elif args.SRC.endswith(IMG_EXTENSIONS):
            img_paths.append(args.SRC)
        if args.filter:
            for img in img_paths[:]:
                if filter_mode == 'IN' and not any(k in img for k in filter_keywords):
                    img_paths.remove(img)
                elif filter_mode == 'OUT' and any(k in img for k in filter_keywords):
                    img_paths.remove(img)
        assert len(img_paths) > 0, 'No images to process'
        ds = ImageDataset(img_paths, resize=classifier.hparams.resize, input_src=args.SRC, pad=run_pad)
        loader = DataLoader(ds, batch_size=args.batch_size, pin_memory=True, num_workers=args.loaders,
                            collate_fn=collate_rois)
        trainer.test(classifier, loader, args.SRC, ds.transform, callbacks)


def argparse_nn(parser=None):
    if parser is None:
        parser = argparse.ArgumentParser(description='Train, Run, and perform other tasks related to ifcb and general image classification!')
    subparsers = parser.add_subparsers(dest='cmd_mode', help='These sub-commands are mutually exclusive. Note: optional arguments (below) must be specified before "TRAIN" or "RUN"')
    train = subparsers.add_parser('TRAIN', help='Train a new model')
    run = subparsers.add_parser('RUN', help='Run a previously trained model')
    common = parser.add_argument_group(title='NN Common Args', description=None)
    common.add_argument('--batch', dest='batch_size', metavar='SIZE', default=108, type=int, help='Number of images per batch. Defaults is 108')
    common.add_argument('--loaders', metavar='N', default=4, type=int, help='Number of data-loading threads. 4 per GPU is typical. Default is 4')
    common.add_argument('--precision', choices=['bf16', 'fp32'], default='bf16', help='(MI355X path, additive) activation storage / MFMA type: bf16 = performance mode (default), fp32 = parity mode matching the reference CPU arithmetic to 1e-3')
    argparse_nn_train(train)
    argparse_nn_run(run)
    return parser


def argparse_nn_train(train_subparser):
    t = train_subparser
    t.add_argument('SRC', help='Directory with class-label subfolders and images. May also be a dataset-configuration csv.')
    t.add_argument('MODEL', help='Select a base model. Eg: "inception_v3"')
    t.add_argument('TRAIN_ID', help='Training ID. This value is the default value used by --outdir and --model-id.')
    model = t.add_argument_group(title='Model Adjustments', description=None)
    model.add_argument('--untrain', dest='pretrained', default=True, action='store_false', help='If set, initializes MODEL ~without~ pretrained neurons. Default (unset) is pretrained')
    model.add_argument('--weights', metavar='PATH', default=os.environ.get('IFCBK_PRETRAINED_WEIGHTS'), help='(MI355X path, additive) torchvision state_dict (.pth) standing in for the ImageNet weights the reference downloads when --untrain is not set; there is no network / torchvision here. Default: $IFCBK_PRETRAINED_WEIGHTS')
    model.add_argument('--pad', metavar='FILL', nargs='?', const='border', type=pad_arg, default=None, help='(MI355X path, additive) Keep each image\'s aspect ratio: resize it to fit the square input (PIL.ImageOps.pad, bilinear, centred) and fill the rest with FILL, instead of stretching it. FILL is "border" (per image, the mean level of its border pixels; the bare flag) or a grey level 0..255. Applies to the training and the validation set; RUN reads it from the model file. Put the bare flag behind the positionals (before them argparse takes SRC for FILL). Default (unset) stretches to the square')
    model.add_argument('--img-norm', nargs=2, metavar=('MEAN', 'STD'), help='Normalize images by MEAN and STD. eg1: "0.667 0.161", eg2: "0.056,0.058,0.051 0.067,0.071,0.057"')
    data = t.add_argument_group(title='Dataset Adjustments', description=None)
    data.add_argument('--seed', default=0, type=int, help='Set a specific seed for deterministic output & dataset-splitting reproducability.')
    data.add_argument('--split', metavar='T:V', default='80:20', help='Ratio of images per-class to split randomly into Training and Validation datasets. Default is "80:20"')
    data.add_argument('--class-config', metavar=('CSV', 'COL'), nargs=2, help='Skip and combine classes as defined by column COL of a special CSV configuration file')
    data.add_argument('--class-min', metavar='MIN', default=2, type=int, help='Exclude classes with fewer than MIN instances. Default is 2')
    data.add_argument('--class-max', metavar='MAX', default=None, type=int, help='Limit classes to a MAX number of instances.')
    data.add_argument('--swap', default=False, action='store_true', help=argparse.SUPPRESS)
    data.add_argument('--resident', default=False, action='store_true', help='(MI355X path, additive) Decode the training and the validation images ONCE (with --loaders workers), hold them on the GPU as ragged u8 ROIs and cut every batch of every epoch there, instead of decoding, collating and uploading each batch of each epoch again. Same order, same augmentation draws and same results as "--loaders 0" for an all-grey or an all-RGB dataset (a mixed one is held as RGB throughout, where the per-batch path decides per batch). Both sets must fit the GPU\'s free memory beside the model, else TRAIN stops and names the sizes; data parallel, every rank holds both whole sets. Default (unset) reads the files every epoch')
    epochs = t.add_argument_group(title='Epoch Parameters', description=None)
    epochs.add_argument('--emax', metavar='MAX', default=60, type=int, help='Maximum number of training epochs. Default is 60')
    epochs.add_argument('--emin', metavar='MIN', default=10, type=int, help='Minimum number of training epochs. Default is 10')
    epochs.add_argument('--estop', metavar='STOP', default=10, type=int, help='Early Stopping: Number of epochs following a best-epoch after-which to stop training. Set STOP=0 to disable. Default is 10')
    augs = t.add_argument_group(title='Augmentation Options')
    augs.add_argument('--flip', choices=['x', 'y', 'xy', 'x+V', 'y+V', 'xy+V'], help='Training images have 50%% chance of being flipped along the designated axis: (x) vertically, (y) horizontally, (xy) either/both. "+V" includes the Validation dataset')
    augs.add_argument('--rot90', nargs='?', const='T', choices=['T', '+V'], default=None, help='(MI355X path, additive) Training images are rotated counter-clockwise by k quarter turns, k uniform in {0,1,2,3}, after any --flip and before the resize. "+V" includes the Validation dataset. With "--flip xy" the eight symmetries of the square are equally likely. Default (unset) is no rotation')
    augs.add_argument('--jitter', metavar='B[,C]', type=jitter_arg, default=None, help='(MI355X path, additive) Brightness / contrast jitter of the training images, as transforms.ColorJitter(brightness=B, contrast=C) in front of the resize: per image a brightness factor uniform in [max(0, 1-B), 1+B] and a contrast factor uniform in [max(0, 1-C), 1+C] (PIL.ImageEnhance arithmetic, on the GPU; always brightness first). B and C are finite floats >= 0, C defaults to 0. Training set only. Default (unset, also "0") is no jitter')
    augs.add_argument('--mixup', metavar='ALPHA', type=mix_alpha_arg, default=0.0, action=_ExclusiveLossScalar, help='(MI355X path, additive) Mixup of the training batches, as timm\'s Mixup in batch mode: per batch lam ~ Beta(ALPHA, ALPHA), every image becomes lam * image + (1 - lam) * partner, the partner being the image at the mirrored place of the batch, and the loss takes both labels with weights lam and 1 - lam. Mixed on the GPU after the resize. A finite float > 0; composes with --class-norm and --label-smoothing, not with --focal-gamma; val_loss stays unmixed. Default is 0 (off)')
    augs.add_argument('--cutmix', metavar='ALPHA', type=mix_alpha_arg, default=0.0, action=_ExclusiveLossScalar, help='(MI355X path, additive) CutMix of the training batches, as timm\'s Mixup(cutmix_alpha=ALPHA) in batch mode: per batch a box covering about 1 - Beta(ALPHA, ALPHA) of the image is filled from the partner image, and lam is the share left outside the box. With --mixup as well, each batch is CutMix with probability 0.5, else Mixup. A finite float > 0; not with --focal-gamma. Default is 0 (off)')
    augs.add_argument('--mix-prob', metavar='P', type=mix_prob_arg, default=1.0, help='(MI355X path, additive) Probability that a training batch is mixed at all by --mixup / --cutmix. A float in [0, 1]. Default is 1')
    augs.add_argument('--blur', metavar='SIGMA_MAX', type=blur_arg, default=None, help='(MI355X path, additive) Gaussian defocus of the training images, as transforms.GaussianBlur(k, sigma=(0.1, SIGMA_MAX)) behind the resize: each image is blurred with probability --blur-prob, with sigma uniform in [0.1, SIGMA_MAX], by a window of radius ceil(3*SIGMA_MAX) (k = 2*radius+1) with reflected borders, on the GPU. SIGMA_MAX is a float in (0.1, 4]. Training set only; not with --distill. Default (unset) is no blur')
    augs.add_argument('--blur-prob', metavar='P', type=blur_prob_arg, default=0.5, help='(MI355X path, additive) Probability that a training image is blurred at all by --blur. A float in [0, 1]. Default is 0.5')
    out = t.add_argument_group(title='Output Options')
    out.add_argument('--outdir', default='training-output/{TRAIN_ID}', help='Default is "training-output/{TRAIN_ID}"')
    out.add_argument('--model-id', default='{TRAIN_ID}', help='Set a specific model id. Patterns {TRAIN_DATE} and {TRAIN_ID} are recognized. Default is "{TRAIN_ID}"')
    out.add_argument('--epochs-log', metavar='ELOG', default='epochs.csv', help='Specify a csv filename. Default is epochs.csv')
    out.add_argument('--args-log', metavar='ALOG', default='args.yml', help='Specify a human-readable yaml filename. Default is args.yml')
    out.add_argument('--onnx', action='store_true', help='Additionally output an onnx version of the model')
    out.add_argument('--results', dest='result_files', metavar=('FNAME', 'SERIES'), nargs='+', action='append', help='FNAME: validation-results filename or pattern ("{epoch}"); .json .h5 .mat.  SERIES: data to include.')
    optim = t.add_argument_group(title='Optimization', description='(MI355X path, additive: upstream keeps these flags commented out, neuston_net.py:385-390; the defaults are its only behaviour, Adam(lr=0.001))')
    optim.add_argument('--optimizer', default='Adam', choices=['Adam', 'SGD', 'AdamW'], help='Select an optimizer. AdamW (MI355X path, additive) is Adam with decoupled weight decay, as torch.optim.AdamW over all parameters: --weight-decay WD then shrinks every parameter by the factor 1 - lr * WD ahead of each step instead of joining the gradient, and follows the --lr-schedule. Default is Adam')
    optim.add_argument('--learning-rate', default=0.001, type=float, help='Set a learning rate. Default is 0.001')
    optim.add_argument('--lr-schedule', choices=['constant', 'cosine', 'linear'], default='constant', help='(MI355X path, additive) How the learning rate moves over the run\'s emax * (batches per epoch) optimizer steps, behind any --warmup: "cosine" decays from --learning-rate to --lr-min along half a cosine (torch\'s CosineAnnealingLR, stepped per batch), "linear" along a straight line; the rate is a launch argument of the fused optimizer step. Early stopping ends the run part-way down the curve. Each epoch then reports the rate of its last step. Default is constant')
    optim.add_argument('--warmup', metavar='EPOCHS', type=_lr_nonneg, default=0.0, help='(MI355X path, additive) Linear warm-up: over the first EPOCHS epochs (a float, e.g. 0.5; rounded to whole steps) the rate rises from --learning-rate / W to --learning-rate, W the number of warm-up steps, as torch\'s LinearLR. Must be less than --emax; combines with every --lr-schedule. Default is 0 (none)')
    optim.add_argument('--lr-min', metavar='LR', type=_lr_nonneg, default=0.0, help='(MI355X path, additive) The rate a cosine or linear --lr-schedule ends at. A float in [0, --learning-rate]. Default is 0')
    optim.add_argument('--momentum', default=0.0, type=float, help='SGD momentum. Default is 0')
    optim.add_argument('--weight-decay', default=0.0, type=float, help='L2 weight decay of every parameter, as torch.optim.Adam/SGD(weight_decay=WD); with "--optimizer AdamW" the decoupled decay of torch.optim.AdamW(weight_decay=WD). Default is 0')
    optim.add_argument('--class-norm', metavar='POWER', nargs='?', const=1.0, type=_class_norm_power, default=None, help='Bias results to emphasize smaller classes: weight the loss of class c by n_c^-POWER (n_c: training images of the class), scaled to a mean weight of 1 per training image. POWER defaults to 1 ("balanced"); 0 weights all classes equally. Default (unset) is the unweighted loss')
    optim.add_argument('--label-smoothing', metavar='EPS', default=0.0, type=_label_smoothing, action=_ExclusiveLossScalar, help='Label smoothing of the loss, as nn.CrossEntropyLoss(label_smoothing=EPS): the target distribution is (1-EPS) one-hot + EPS/C uniform, for noisy annotations. A float in [0, 1]; val_loss follows the smoothed value. Default is 0 (hard labels)')
    optim.add_argument('--focal-gamma', metavar='GAMMA', default=0.0, type=_focal_gamma, action=_ExclusiveLossScalar, help='Focal loss against class imbalance: the loss of an image is scaled by (1 - p)^GAMMA, p the softmax probability of its class, so images the network already classifies confidently count less. A finite float >= 0; composes with --class-norm (its weights are the per-class alpha), not with --label-smoothing; val_loss follows the focal value. Default is 0 (cross-entropy)')
    optim.add_argument('--ema', metavar='DECAY', type=_ema_decay, default=None, help='(MI355X path, additive) Keep an exponential moving average of the weights and of the BatchNorm running statistics, updated inside the fused optimizer step: avg += (1 - d) * (weights - avg) after every step, d = min(DECAY, (1 + t) / (10 + t)) at the t-th step (the warm-up of TensorFlow\'s ExponentialMovingAverage), as torch.optim.swa_utils.get_ema_multi_avg_fn / timm\'s ModelEmaV3. Validation (val_loss, F1, --results files), early stopping, the choice of the best epoch, the saved model and --onnx then use the averaged weights; the training trajectory is unchanged. A float in (0, 1), e.g. 0.999. Default (unset) is no averaging')
    optim.add_argument('--clip-grad', metavar='NORM', type=_clip_grad, default=None, help='(MI355X path, additive) Clip the gradient of every step by its global L2 norm: when the norm over all parameters exceeds NORM the whole gradient is scaled by NORM / (norm + 1e-6), as torch.nn.utils.clip_grad_norm_(parameters, NORM) before every optimizer step / Lightning\'s gradient_clip_val. The norm and the scale are taken on the GPU inside the fused step; weight decay is added to the clipped gradient; with several GPUs the averaged gradient is clipped. Each epoch reports its largest norm and how many steps were clipped. A finite float > 0, e.g. 1.0. Default (unset) is no clipping')
    optim.add_argument('--accumulate', metavar='K', type=_accumulate, default=1, help='(MI355X path, additive) Gradient accumulation, as Lightning\'s accumulate_grad_batches=K: the gradients of K consecutive training batches are summed on the GPU and one optimizer step is taken from the sum times 1/K, for an effective batch of K x --batch x GPUs where one launch or the card\'s memory holds only --batch. BatchNorm statistics stay per batch; the last window of an epoch is applied even when it holds fewer than K batches, still scaled by 1/K; --lr-schedule, --warmup, --ema, --clip-grad and the step count of the model file count optimizer steps. An integer >= 1 and at most the training batches of an epoch; combines with every other flag. Default is 1 (a step per batch)')
    optim.add_argument('--distill', metavar='TEACHER.ptl', default=None, action=_ExclusiveLossScalar, help='(MI355X path, additive) Knowledge distillation: train MODEL to match the class scores of a trained teacher model file as well as the labels, (1 - A) * CrossEntropy + A * T^2 * KL(softmax(teacher / T) || softmax(student / T)). The teacher may be any backbone and input size (e.g. an inception_v3 teacher for a resnet18 student); its class list must equal the training set\'s. It sees every training batch with the same flips, turns and jitter, resized and normalised as it was trained. Composes with --class-norm (hard term only) and --label-smoothing, not with --focal-gamma, --mixup or --cutmix; val_loss stays the hard loss. RUN needs the student file alone. Default (unset) is no teacher')
    optim.add_argument('--distill-alpha', metavar='A', type=_distill_alpha, default=0.5, help='Weight of the teacher term of --distill, a float in [0, 1]. Default is 0.5')
    optim.add_argument('--distill-temperature', metavar='T', type=_distill_temperature, default=4.0, help='Softmax temperature of --distill, a finite float > 0. Default is 4')
    meta = t.add_argument_group(title='Metadata and Annotations')
    meta.add_argument('--dataset-id', help='Associate a dataset id label with this model')
    meta.add_argument('--notes', help='Add any kind of note to the trained model.')


def argparse_nn_run(run_subparser):
    r = run_subparser
    r.add_argument('SRC', help='Resource(s) to be classified. Accepts a bin, an image, a text-file, or a directory. Directories are accessed recursively')
    r.add_argument('MODEL', help='Path to a previously-trained model file')
    r.add_argument('RUN_ID', help='Run ID. Used by --outdir')
    r.add_argument('--type', dest='src_type', default='bin', choices=['bin', 'img'], help='File type to perform classification on. Defaults is "bin"')
    r.add_argument('--outdir', default='run-output/{RUN_ID}/v3/{MODEL_ID}', help='Default is "run-output/{RUN_ID}/v3/{MODEL_ID}"')
    r.add_argument('--outfile', action='append', help='Name/pattern of the output classification file ({BIN_ID}, {BIN_YEAR}, {BIN_DATE}, {INPUT_SUBDIRS}; .json .mat .h5)')
    r.add_argument('--filter', nargs='+', metavar=('IN|OUT', 'KEYWORD'), help='Explicitly include (IN) or exclude (OUT) bins or image-files by KEYWORDs.')
    r.add_argument('--clobber', action='store_true', help='If set, already processed bins in OUTDIR are reprocessed.')
    r.add_argument('--gobig', action='store_true', help=argparse.SUPPRESS)
    r.add_argument('--tta', choices=['flips', 'all'], default=None, help='(MI355X path, additive) Test-time augmentation: the class scores of an image are the mean of the softmax outputs over symmetry views of the resized network input, "flips" = 4 views (identity, both flips, half turn), "all" = the 8 symmetries of the square; for models trained with --flip / --rot90. Costs 4 or 8 forwards per batch; the output files keep their format. Default (unset) is one view')


def argparse_nn_runtimeparams(args):
    args.cmd_timestamp = dt.datetime.now(dt.timezone.utc).isoformat(timespec='seconds')
    try:
        with open('version') as f:
            args.version = f.read().strip()
    except FileNotFoundError:
        args.version = None
    if torch.cuda.is_available():
        vis = os.environ.get('CUDA_VISIBLE_DEVICES') or os.environ.get('HIP_VISIBLE_DEVICES') or \
            os.environ.get('ROCR_VISIBLE_DEVICES')
        args.gpus = [int(g) for g in vis.split(',')] if vis else list(range(torch.cuda.device_count()))
    else:
        args.gpus = None
    proc_outdir(args)


def proc_outdir(args):
    run_date_str, _ = args.cmd_timestamp.split('T')
    if args.cmd_mode == 'TRAIN':
        args.outdir = args.outdir.format(TRAIN_DATE=run_date_str, TRAIN_ID=args.TRAIN_ID)
    elif args.cmd_mode == 'RUN':
        hp = load_checkpoint_file(args.MODEL)['hyper_parameters']   # no model build
        args.outdir = args.outdir.format(RUN_DATE=run_date_str, RUN_ID=args.RUN_ID, MODEL_ID=hp['model_id'])


if __name__ == '__main__':
    parser = argparse_nn()
    input_args = parser.parse_args()
    argparse_nn_runtimeparams(input_args)
    main(input_args)
