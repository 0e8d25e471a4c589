"""TRAIN --accumulate from the command line: a run of two epochs with an odd number of training batches (so every epoch ends on a short
window) prints its start line, counts optimizer steps in the schedule, the model file and the engine, and RUN reads the result;
``--accumulate 1`` trains the weights of a run without the flag, bit for bit."""
import json
import math
import os
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PER_CLASS = 12          # 2 classes x 12 ROIs: 18..20 training images at the 80:20 split, 5 batches of 4 (the last one short)


def _make_dataset(root):
    from PIL import Image
    rng = np.random.default_rng(11)
    for cls, mean in (('cls_dark', 96), ('cls_bright', 160)):
        os.makedirs(os.path.join(root, cls))
        for i in range(PER_CLASS):
            h, w = rng.integers(32, 97, 2)
            a = np.clip(rng.normal(mean, 32, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(root, cls, 'roi_%s_%03d.png' % (cls, i)))


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def _train(src, outdir, model_id, *flags):
    """-> the NeustonModel the run built (its engine as the last epoch left it)"""
    from ifcb_classifier_amd import neuston_net as nn_
    made = []

    class Spy(nn_.NeustonModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    with mock.patch.object(nn_, 'NeustonModel', Spy):
        _cli(['--batch', '4', '--loaders', '0', '--precision', 'fp32', 'TRAIN', src, 'resnet18', model_id, '--untrain', '--seed', '1',
              '--emax', '2', '--emin', '1', '--estop', '0', '--outdir', outdir, *flags])
    assert len(made) == 1
    return made[0]


def test_train_with_accumulate_then_run(tmp_path, capsys):
    import yaml
    src = str(tmp_path / 'training-data')
    os.makedirs(src)
    _make_dataset(src)
    out = str(tmp_path / 'training-output' / 'acc')
    model = _train(src, out, 'acc', '--accumulate', '2', '--lr-schedule', 'cosine')
    printed = capsys.readouterr().out
    n_train = len(open(os.path.join(out, 'training_images.list')).read().splitlines())
    batches = math.ceil(n_train / 4)
    steps = math.ceil(batches / 2)
    assert batches % 2 == 1 and batches >= 3, (n_train, batches)              # every epoch ends on a window of one batch
    line = [ln for ln in printed.splitlines() if ln.startswith('Accumulating gradients over')]
    assert line == ['Accumulating gradients over 2 batches: effective batch 8 (4 x 2 x 1 GPU(s)), %d optimizer steps per epoch' % steps], printed[-2000:]
    assert 'Learning rate: cosine schedule over %d steps' % (2 * steps) in printed
    rows = open(os.path.join(out, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 3          # 2 rows
    assert all(math.isfinite(float(r.split(',')[2])) for r in rows[1:])
    assert yaml.safe_load(open(os.path.join(out, 'args.yml')))['accumulate'] == 2
    ck = torch.load(os.path.join(out, 'acc.ptl'), map_location='cpu', weights_only=False)
    assert ck['hyper_parameters']['accumulate'] == 2
    eng = model.model.engine
    assert eng.accumulate == 2 and eng.acc_pending == 0                       # the trainer left no window open
    assert eng.step_count == 2 * steps                                        # optimizer steps of the run: 2 epochs x ceil(batches / 2)
    assert bool((eng.nbt == 2 * batches).all())                               # BatchNorm counted batches
    # the file is the best epoch's: its step count is that epoch's
    assert ck['global_step'] == (ck['epoch'] + 1) * steps
    assert int(ck['optimizer_states'][0]['state'][0]['step']) == ck['global_step']
    import ctypes as C
    sched = eng.lr_schedule                                                   # the schedule ran out exactly: the last step's rate is its last
    assert sched.total_steps == 2 * steps and eng.lr_now == C.c_float(sched.at(2 * steps - 1)).value < 0.001

    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '4', '--loaders', '0', 'RUN', src, os.path.join(out, 'acc.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'acc', 'img_results.json')))
    scores = np.array(rj['output_scores'], dtype=np.float32)
    assert rj['model_id'] == 'acc' and scores.shape == (2 * PER_CLASS, 2) and np.allclose(scores.sum(1), 1, atol=1e-4)


def test_accumulate_1_trains_the_weights_of_a_run_without_the_flag(tmp_path, capsys):
    src = str(tmp_path / 'training-data')
    os.makedirs(src)
    _make_dataset(src)
    outs = [str(tmp_path / 'training-output' / name) for name in ('plain', 'one')]
    plain = _train(src, outs[0], 'plain')
    one = _train(src, outs[1], 'one', '--accumulate', '1')
    assert 'Accumulating gradients' not in capsys.readouterr().out            # K = 1 prints nothing new
    assert one.model.engine.A is None and one.model.engine.step_count == plain.model.engine.step_count > 0
    torch.cuda.synchronize()
    for key in ('P', 'M', 'V', 'RB', 'nbt'):
        a, b = getattr(plain.model.engine, key), getattr(one.model.engine, key)
        assert torch.equal(a.cpu().view(torch.int32) if a.dtype == torch.float32 else a.cpu(),
                           b.cpu().view(torch.int32) if b.dtype == torch.float32 else b.cpu()), key
    cks = [torch.load(os.path.join(o, n + '.ptl'), map_location='cpu', weights_only=False) for o, n in zip(outs, ('plain', 'one'))]
    assert cks[0]['global_step'] == cks[1]['global_step'] and cks[0]['epoch'] == cks[1]['epoch']
    assert list(cks[0]['state_dict']) == list(cks[1]['state_dict'])
    for k, v in cks[0]['state_dict'].items():
        assert torch.equal(v, cks[1]['state_dict'][k]), k
    assert cks[1]['hyper_parameters']['accumulate'] == 1
    rows = [[ln.split(',')[:4] for ln in open(os.path.join(o, 'epochs.csv')).read().strip().splitlines()] for o in outs]
    assert rows[0] == rows[1] and len(rows[0]) == 3                           # epoch, best, train_loss, val_loss: the same trajectory
