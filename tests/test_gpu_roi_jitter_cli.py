"""TRAIN --jitter from the command line, on the GPU: one epoch on a tiny image dataset with the ranges in args.yml and the .ptl, RUN of
the model, and `--jitter 0` against no flag at all: the same weights bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CLASSES = ['big', 'mid', 'small']


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def _dataset(src):
    from PIL import Image
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 20), ('mid', 130, 8), ('small', 170, 4)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))


def _train(src, outdir, name, *flags):
    _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', name, '--untrain', '--seed', '1', '--emax', '1', '--emin', '1',
          '--estop', '0', '--outdir', outdir, '--flip', 'xy'] + list(flags))
    return torch.load(os.path.join(outdir, name + '.ptl'), map_location='cpu', weights_only=False)


def test_train_jitter_then_run_and_zero_range_is_no_flag(tmp_path):
    import yaml
    src = str(tmp_path / 'training-data')
    _dataset(src)
    outdir = str(tmp_path / 'training-output' / 'jt')
    ck = _train(src, outdir, 'jt', '--jitter', '0.3,0.3')
    y = yaml.safe_load(open(os.path.join(outdir, 'args.yml')))
    assert y['jitter'] == [0.3, 0.3] and y['classes'] == CLASSES
    assert ck['hyper_parameters']['jitter'] == [0.3, 0.3]
    rows = open(os.path.join(outdir, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 2
    assert all(np.isfinite(float(v)) for v in rows[1].split(',')[2:4])
    # RUN of that checkpoint: the usual shape
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(outdir, 'jt.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'jt', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'jt' and rj['class_labels'] == CLASSES and scores.shape == (32, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()
    # --jitter 0 is "unset": the weights of a run without the flag, bit for bit; the jittered run's differ
    plain = _train(src, str(tmp_path / 'training-output' / 'p0'), 'p0')
    zero = _train(src, str(tmp_path / 'training-output' / 'z0'), 'z0', '--jitter', '0')
    assert zero['hyper_parameters']['jitter'] is None and plain['hyper_parameters']['jitter'] is None
    assert sorted(plain['state_dict']) == sorted(zero['state_dict'])
    for k, v in plain['state_dict'].items():
        assert torch.equal(v, zero['state_dict'][k]), k
    assert any(not torch.equal(v, ck['state_dict'][k]) for k, v in plain['state_dict'].items() if v.is_floating_point())
