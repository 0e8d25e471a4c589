"""neuston_util (the reference's auxiliary tool) without a GPU: the two config makers byte for byte against the reference's own
output, the host-side arithmetic of CALC_IMG_NORM on moments computed from Pillow's resize, the argparse surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util_norm_check as unc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = unc.golden()


def _util(argv, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-m', 'ifcb_classifier_amd.neuston_util'] + argv, cwd=cwd, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


@pytest.mark.parametrize('i', range(len(G['make'])), ids=[' '.join(m['argv']) for m in G['make']])
def test_make_commands_match_the_reference_byte_for_byte(tmp_path, i):
    m = G['make'][i]
    unc.mug.make_config_tree(str(tmp_path))
    r = _util(m['argv'], str(tmp_path))
    assert r.returncode == 0, r.stderr
    if m['outfile']:
        assert r.stdout == ''
        with open(tmp_path / m['outfile'], newline='') as f:
            assert f.read() == m['output']
    else:
        assert r.stdout == m['output']


def test_make_class_config_rejects_what_is_neither_a_folder_nor_a_csv(tmp_path):
    from ifcb_classifier_amd import neuston_util as nu
    bad = str(tmp_path / 'nope.txt')
    with pytest.raises(ValueError, match=r'^Dataset is invalid: "%s"$' % bad.replace('.', r'\.')):
        nu.make_class_config(unc.namespace(dataset=bad, outfile=None))


@pytest.mark.parametrize('cmd,flags', [
    ('MAKE_DATASET_CONFIG', ['PATH', '-o', '--outfile']),
    ('MAKE_CLASS_CONFIG', ['PATH', '-o', '--outfile']),
    ('CALC_IMG_NORM', ['SRC', '--resize', '--class-config', 'CSV COL', '--class-min', '--class-max', '--batch-size', '--loaders']),
])
def test_argparse_surface(cmd, flags):
    r = _util([cmd, '--help'], ROOT)
    assert r.returncode == 0, r.stderr
    for f in flags:
        assert f in r.stdout, (f, r.stdout)
    from ifcb_classifier_amd import neuston_util as nu
    a = nu.argparse_init().parse_args(['CALC_IMG_NORM', 'src'])
    assert (a.resize, a.class_config, a.class_min, a.class_max, a.batch_size, a.loaders) == (299, None, 2, None, 108, 4)
    assert nu.argparse_init().parse_args(['CALC_IMG_NORM', 'src', '--batch-size', '16']).batch_size == 16
    assert _util(['CALC_IMG_NORM', 'src', '--resize', '256'], ROOT).returncode == 2          # choices 224 / 299


def test_batch_stats_is_exact_and_rounded_once():
    from fractions import Fraction
    from ifcb_classifier_amd.neuston_util import batch_stats
    # all-255 planes: n * sum_v2 - sum_v^2 is far beyond int64 for 300 planes of 299^2, and the std is exactly 0
    n = 300 * 299 * 299
    m, s = batch_stats([255 * n], [255 * 255 * n], n)
    assert m.tolist() == [1.0] * 3 and s.tolist() == [0.0] * 3
    assert (255 * 255 * n) * n > 2 ** 63
    # half zeros, half 255: mean 1/2 and std 1/2 exactly, per channel
    m, s = batch_stats([255, 0, 255 * 2], [255 * 255, 0, 2 * 255 * 255], 2)
    assert m.tolist() == [0.5, 0.0, 1.0] and s.tolist() == [0.5, 0.0, 0.0]
    rng = np.random.default_rng(5)
    for _ in range(300):
        v = rng.integers(0, 256, int(rng.integers(1, 4000)))
        n, sv, sv2 = v.size, int(v.sum()), int((v * v).sum())
        m, s = batch_stats([sv], [sv2], n)
        # correctly rounded: no float32 is closer to the exact value (compared as exact rationals / squares)
        t = Fraction(sv, 255 * n)
        for cand in (np.nextafter(m[0], np.float32(0)), np.nextafter(m[0], np.float32(2))):
            assert abs(Fraction(float(cand)) - t) >= abs(Fraction(float(m[0])) - t)
        var = Fraction(n * sv2 - sv * sv, (255 * n) ** 2)
        below, above = np.nextafter(s[0], np.float32(0)), np.nextafter(s[0], np.float32(2))
        assert (Fraction(float(below)) + Fraction(float(s[0]))) ** 2 / 4 <= var <= (Fraction(float(above)) + Fraction(float(s[0]))) ** 2 / 4


def _pil_moments(loader, resize):
    """CPU stand-in for the GPU half of CALC_IMG_NORM: Pillow's resize of each image (the reference's transform chain), numpy sums"""
    from PIL import Image
    for batch, _, paths in loader:
        ch = batch['in_channels']
        sv, sv2 = np.zeros(ch, np.int64), np.zeros(ch, np.int64)
        for p in paths:
            with open(p, 'rb') as f:
                img = Image.open(f)
                img = img if (ch == 1 and img.mode == 'L') else img.convert('RGB')
                v = np.asarray(img.resize((resize, resize), Image.BILINEAR)).astype(np.int64).reshape(-1, ch)
            sv += v.sum(0)
            sv2 += (v * v).sum(0)
        yield [int(x) for x in sv], [int(x) for x in sv2], len(paths) * resize * resize


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('util_tree'))
    unc.build_tree(root)
    return root


@pytest.mark.parametrize('name', [c['name'] for c in G['cases']])
def test_calc_img_norm_host_arithmetic_vs_reference(tree, capsys, monkeypatch, name):
    from ifcb_classifier_amd import neuston_util as nu
    case = next(c for c in G['cases'] if c['name'] == name)
    monkeypatch.setattr(nu, 'gpu_moments', _pil_moments)
    seen, out = unc.run_case(nu, case, tree, capsys, loaders=0)
    unc.check_case(case, seen, out, unc.bound(G))
    if name == 'D':                                                        # grey-only batches report one value thrice
        assert any(len(set(m.tolist())) == 1 for m, _ in seen)


def test_calc_img_norm_without_a_gpu_is_an_error(tree, monkeypatch):
    import torch
    from ifcb_classifier_amd import neuston_util as nu
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    args = unc.namespace(SRC=tree, resize=224, batch_size=64, class_min=2, class_max=None, class_config=None, loaders=0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        nu.calc_img_norm(args)


def test_the_module_imports_neither_the_oracle_nor_torchvision():
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'neuston_util.py')).read()
    assert 'oracle' not in src and 'torchvision' not in src
