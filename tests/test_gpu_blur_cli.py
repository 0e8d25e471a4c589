"""TRAIN --blur from the command line, on the GPU: two epochs on a tiny image dataset (ifcbk_batch_blur behind every training batch's
resize), the two values in args.yml and the .ptl, finite losses, RUN of the model; and `--blur 2 --blur-prob 0`, which draws no sigma
and ends with the weights of the run without the flag, bit for bit."""
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


@pytest.fixture(scope='module')
def src(tmp_path_factory):
    from PIL import Image
    root = str(tmp_path_factory.mktemp('blur_cli') / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 24), ('mid', 130, 8), ('small', 170, 4)):
        os.makedirs(os.path.join(root, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(root, cls, 'roi_%s_%03d.png' % (cls, i)))
    return root


def _train(src, outdir, run, *flags):
    _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', run, '--untrain', '--seed', '1', '--emax', '2', '--emin', '2',
          '--estop', '0', '--outdir', outdir, '--flip', 'xy'] + list(flags))
    return torch.load(os.path.join(outdir, run + '.ptl'), map_location='cpu', weights_only=False)


def test_train_blur_then_run(src, tmp_path):
    import yaml
    outdir = str(tmp_path / 'training-output' / 'bl')
    ck = _train(src, outdir, 'bl', '--blur', '2', '--blur-prob', '0.75')
    y = yaml.safe_load(open(os.path.join(outdir, 'args.yml')))
    assert (y['blur'], y['blur_prob']) == (2.0, 0.75)
    hp = ck['hyper_parameters']
    assert (hp['blur'], hp['blur_prob']) == (2.0, 0.75)
    rows = open(os.path.join(outdir, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 3
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r.split(',')[2:4])
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(outdir, 'bl.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'bl', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'bl' and rj['class_labels'] == ['big', 'mid', 'small'] and scores.shape == (36, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()


def test_blur_prob_0_trains_to_the_bits_of_the_run_without_the_flag(src, tmp_path):
    a = _train(src, str(tmp_path / 'out' / 'p0'), 'p0', '--blur', '2', '--blur-prob', '0')
    b = _train(src, str(tmp_path / 'out' / 'no'), 'no')
    assert a['hyper_parameters']['blur'] == 2.0 and 'blur' not in b['hyper_parameters']
    sa, sb = a['state_dict'], b['state_dict']
    assert sorted(sa) == sorted(sb) and len(sa) > 20
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
