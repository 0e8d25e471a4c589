"""TRAIN --mixup / --cutmix from the command line, on the GPU: two epochs with --label-smoothing and --class-norm on a tiny image dataset,
the three values in args.yml and the .ptl, finite losses, RUN of the model, and a second TRAIN with the same seed that reproduces
epochs.csv."""
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


def test_train_mixup_cutmix_then_run_and_reproduce(tmp_path):
    from PIL import Image
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 40), ('mid', 130, 8), ('small', 170, 3)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))
    csvs = []
    for run in ('mx', 'mx2'):
        outdir = str(tmp_path / 'training-output' / run)
        _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', run, '--untrain', '--seed', '1', '--emax', '2', '--emin', '2',
              '--estop', '0', '--outdir', outdir, '--mixup', '0.4', '--cutmix', '1.0', '--label-smoothing', '0.1', '--class-norm'])
        csvs.append(open(os.path.join(outdir, 'epochs.csv')).read())
    assert csvs[0] == csvs[1]                                       # the draws come from the seed: the run repeats bit for bit
    outdir = str(tmp_path / 'training-output' / 'mx')
    import yaml
    y = yaml.safe_load(open(os.path.join(outdir, 'args.yml')))
    assert (y['mixup'], y['cutmix'], y['mix_prob'], y['label_smoothing'], y['class_norm']) == (0.4, 1.0, 1.0, 0.1, 1.0)
    ck = torch.load(os.path.join(outdir, 'mx.ptl'), map_location='cpu', weights_only=False)
    hp = ck['hyper_parameters']
    assert (hp['mixup'], hp['cutmix'], hp['mix_prob']) == (0.4, 1.0, 1.0) and hp['class_weights'] == y['class_weights']
    rows = csvs[0].strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 3
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r.split(',')[2:4])
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(outdir, 'mx.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'mx', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'mx' and rj['class_labels'] == ['big', 'mid', 'small'] and scores.shape == (51, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()
