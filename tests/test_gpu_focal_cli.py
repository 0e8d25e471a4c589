"""TRAIN --focal-gamma from the command line, on the GPU: one epoch with --class-norm on a tiny image dataset, the value in args.yml and
the .ptl, a finite val_loss, and RUN of the model."""
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


def test_train_focal_gamma_class_norm_then_run(tmp_path):
    from PIL import Image
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 40), ('mid', 130, 8), ('small', 170, 3)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))
    outdir = str(tmp_path / 'training-output' / 'fg')
    _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', 'fg', '--untrain', '--seed', '1', '--emax', '1', '--emin', '1',
          '--estop', '0', '--outdir', outdir, '--focal-gamma', '2', '--class-norm'])
    classes = ['big', 'mid', 'small']
    import yaml
    y = yaml.safe_load(open(os.path.join(outdir, 'args.yml')))
    assert y['focal_gamma'] == 2.0 and y['class_norm'] == 1.0 and y['label_smoothing'] == 0.0 and y['classes'] == classes
    ck = torch.load(os.path.join(outdir, 'fg.ptl'), map_location='cpu', weights_only=False)
    hp = ck['hyper_parameters']
    assert hp['focal_gamma'] == 2.0 and hp['class_weights'] == y['class_weights']
    assert ck['state_dict']['criterion.weight'].tolist() == y['class_weights']
    rows = open(os.path.join(outdir, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 2
    assert all(np.isfinite(float(v)) for v in rows[1].split(',')[2:4])
    # RUN of that checkpoint: the usual shape
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(outdir, 'fg.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'fg', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'fg' and rj['class_labels'] == classes and scores.shape == (51, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()
