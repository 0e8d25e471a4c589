"""TRAIN --resident from the command line, on the GPU: the same TRAIN command with and without the flag, each in a fresh child process
with a time limit, leaves the same epochs.csv byte for byte, the same bits in every state_dict tensor of the model file, and an
args.yml / hyper_parameters that differ by the one key -- with flips, jitter and mixup on a grey tree, and without augmentation on an
RGB tree.  (``--loaders 0``: with worker processes the per-item draws come from the workers' own streams, and nothing is claimed.)"""
import os
import subprocess
import sys

import pytest
import torch

import resident_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train(cwd, src, extra):
    """one TRAIN in a child process, run from ``cwd`` so that the default --outdir (and with it args.yml) is the same text for both"""
    os.makedirs(cwd)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    argv = [sys.executable, '-m', 'ifcb_classifier_amd.neuston_net', '--batch', '8', '--loaders', '0', 'TRAIN', src, 'resnet18', 'id', '--untrain',
            '--emax', '2', '--emin', '2'] + extra
    r = subprocess.run(argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = os.path.join(cwd, 'training-output', 'id')
    import yaml
    ck = torch.load(os.path.join(out, 'id.ptl'), map_location='cpu', weights_only=False)
    return dict(csv=open(os.path.join(out, 'epochs.csv'), 'rb').read(), yml=yaml.safe_load(open(os.path.join(out, 'args.yml'))), ck=ck,
                lists=[open(os.path.join(out, f)).read() for f in ('training_images.list', 'validation_images.list')], log=r.stdout)


def _compare(off, on):
    assert b'nan' not in off['csv'] and len(off['csv'].splitlines()) == 3
    assert off['csv'] == on['csv']
    sd0, sd1 = off['ck']['state_dict'], on['ck']['state_dict']
    assert list(sd0) == list(sd1) and len(sd0) > 50
    for k in sd0:
        assert sd0[k].dtype == sd1[k].dtype and torch.equal(sd0[k], sd1[k]), k
    assert off['lists'] == on['lists']
    for a, b in ((off['yml'], on['yml']), (off['ck']['hyper_parameters'], on['ck']['hyper_parameters'])):
        diff = {k for k in set(a) | set(b) if k != 'cmd_timestamp' and (k not in a or k not in b or a[k] != b[k])}
        assert diff == {'resident'} and 'resident' not in a and b['resident'] is True
    assert 'Resident: 18 + 6 ROIs' in on['log'] and 'Resident' not in off['log']


def test_flips_jitter_and_mixup_on_a_grey_tree_train_to_the_same_bits(tmp_path):
    src = rc.write_tree(str(tmp_path / 'grey'), 'grey')
    extra = ['--flip', 'xy', '--jitter', '0.2,0.2', '--mixup', '0.4', '--seed', '3']
    off = _train(str(tmp_path / 'off'), src, extra)
    on = _train(str(tmp_path / 'on'), src, extra + ['--resident'])
    _compare(off, on)
    assert (on['yml']['flip'], on['yml']['jitter'], on['yml']['mixup'], on['yml']['seed']) == ('xy', [0.2, 0.2], 0.4, 3)


def test_an_rgb_tree_without_augmentation_trains_to_the_same_bits(tmp_path):
    src = rc.write_tree(str(tmp_path / 'rgb'), 'rgb')
    off = _train(str(tmp_path / 'off'), src, ['--seed', '3'])
    on = _train(str(tmp_path / 'on'), src, ['--seed', '3', '--resident'])
    _compare(off, on)
    assert '3 channel(s)' in on['log']
