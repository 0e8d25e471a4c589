"""TRAIN --optimizer AdamW --weight-decay --lr-schedule cosine --warmup from the command line, on the GPU: three epochs on a tiny image
dataset, the lr column of epochs.csv with the rate of each epoch's last step, the flags in args.yml and the .ptl, RUN of the model; and
the same command line without the new flags, whose log has no lr figure."""
import csv
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def _rows(out):
    with open(os.path.join(out, 'epochs.csv'), newline='') as f:
        return list(csv.DictReader(f))


def test_train_with_adamw_and_a_cosine_schedule_then_run(tmp_path, capsys):
    from PIL import Image
    import yaml
    from ifcb_classifier_amd.lr_schedule import LrSchedule
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 24), ('mid', 130, 8), ('small', 170, 4)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))
    common = ['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18']
    tail = ['--untrain', '--seed', '1', '--emax', '3', '--emin', '3', '--estop', '0']
    out = str(tmp_path / 'training-output' / 'sched')
    _cli(common + ['sched'] + tail + ['--outdir', out, '--optimizer', 'AdamW', '--weight-decay', '0.05', '--lr-schedule', 'cosine', '--warmup', '1'])
    printed = capsys.readouterr().out
    n_train = len(open(os.path.join(out, 'training_images.list')).read().split())
    spe = -(-n_train // 16)                                                   # batches per epoch
    assert spe >= 2
    assert 'Learning rate: cosine schedule over %d steps, %d of them warm-up' % (3 * spe, spe) in printed, printed[-2000:]
    s = LrSchedule('cosine', 0.001, 3 * spe, spe, 0.0)
    want = [C.c_float(s.at((e + 1) * spe - 1)).value for e in range(3)]       # the rate of each epoch's last step, as the op carried it
    rows = _rows(out)
    assert len(rows) == 3 and list(rows[0])[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and 'lr' in rows[0]
    got = [float(r['lr']) for r in rows]
    assert got == want and want[0] == C.c_float(0.001).value > want[1] > want[2] > 0, (got, want)
    assert all(np.isfinite(float(r['train_loss'])) and np.isfinite(float(r['val_loss'])) for r in rows)
    assert printed.count(', lr: ') == 3
    y = yaml.safe_load(open(os.path.join(out, 'args.yml')))
    ck = torch.load(os.path.join(out, 'sched.ptl'), map_location='cpu', weights_only=False)
    for d in (y, ck['hyper_parameters']):
        assert (d['optimizer'], d['weight_decay'], d['lr_schedule'], d['warmup'], d['lr_min']) == ('AdamW', 0.05, 'cosine', 1.0, 0.0)
    grp = ck['optimizer_states'][0]['param_groups'][0]
    assert grp['initial_lr'] == 0.001 and grp['weight_decay'] == 0.05 and grp['lr'] in want
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(out, 'sched.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'sched', 'img_results.json')))
    scores = np.array(rj['output_scores'], dtype=np.float32)
    assert rj['model_id'] == 'sched' and scores.shape == (36, 3) and np.allclose(scores.sum(1), 1, atol=1e-4)
    capsys.readouterr()
    # the same command line without the new flags: no lr figure anywhere
    out2 = str(tmp_path / 'training-output' / 'plain')
    _cli(common + ['plain'] + tail + ['--outdir', out2])
    printed = capsys.readouterr().out
    rows = _rows(out2)
    assert len(rows) == 3 and 'lr' not in rows[0] and list(rows[0])[:4] == ['epoch', 'best', 'train_loss', 'val_loss']
    assert ', lr: ' not in printed and 'Learning rate:' not in printed
    ck2 = torch.load(os.path.join(out2, 'plain.ptl'), map_location='cpu', weights_only=False)
    assert 'initial_lr' not in ck2['optimizer_states'][0]['param_groups'][0]
    assert (ck2['hyper_parameters']['optimizer'], ck2['hyper_parameters']['lr_schedule']) == ('Adam', 'constant')
    # and a refused combination ends TRAIN with its message before anything is built
    with pytest.raises(SystemExit, match='--lr-min 0.01 is above --learning-rate 0.001'):
        _cli(common + ['bad'] + tail + ['--outdir', str(tmp_path / 'bad'), '--lr-schedule', 'cosine', '--lr-min', '0.01'])
