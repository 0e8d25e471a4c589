"""Shared by test_util_cpu.py and test_gpu_util.py: run CALC_IMG_NORM on the golden tree (tests/golden/make_util_golden.py) and
compare with what the reference's own calc_img_norm produced (tests/golden/util_golden.json)."""
import argparse
import json
import os
import random
import re
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)
import make_util_golden as mug  # noqa: E402

_NUM = re.compile(r'-?\d+\.\d+(?:e[-+]?\d+)?')


def _mask(text):
    """numbers -> '#', and the padding numpy puts between array elements of different lengths squeezed out"""
    return re.sub(r' +', ' ', _NUM.sub('#', text)).replace('[ ', '[').replace(' ]', ']')


def golden():
    with open(os.path.join(GOLD, 'util_golden.json')) as f:
        return json.load(f)


def build_tree(root):
    mug.make_image_tree(root)
    with open(os.path.join(root, 'cfg.csv'), 'w') as f:
        f.write(mug.CLASS_CONFIG)


def bound(g):
    """allowed distance from the reference's float32 statistics: 3x the largest gap the generator saw, at least 2e-6"""
    return max(3 * g['max_f32_gap'], 2e-6)


def run_case(nu, case, root, capsys, loaders):
    """neuston_util.main on one golden case (same Python random state as the generator); returns (per-batch (mean, std), stdout)"""
    seen = []
    batch_stats = nu.batch_stats

    def recording(sum_v, sum_v2, count):
        r = batch_stats(sum_v, sum_v2, count)
        seen.append(r)
        return r
    args = mug.case_args((case['name'], case['resize'], case['batch_size'], case['class_min'], case['class_max'],
                          case['class_config'], case['random_seed']), root)
    args.loaders = loaders
    nu.batch_stats = recording
    try:
        capsys.readouterr()
        random.seed(case['random_seed'])
        nu.main(args)
        out = capsys.readouterr().out
    finally:
        nu.batch_stats = batch_stats
    return seen, out.replace(root, '{ROOT}')


def check_case(case, seen, out, tol):
    assert len(seen) == len(case['batches'])
    for (mean, std), b in zip(seen, case['batches']):
        assert mean.dtype == np.float32 and std.dtype == np.float32 and mean.shape == std.shape == (3,)
        for got, exact, ref in ((mean, b['exact_mean'], b['pop_mean']), (std, b['exact_std'], b['pop_std0'])):
            exact32 = np.array(exact, np.float32)
            assert np.all(np.abs(got.astype(np.float64) - np.array(exact)) <= np.spacing(exact32)), (got, exact)
            assert np.abs(got.astype(np.float64) - np.array(ref)).max() <= tol, (got, ref)
    # the text equals the reference's once the numbers are masked; the numbers agree within the bound
    want = case['stdout']
    assert _mask(out) == _mask(want), (out, want)
    got_n, want_n = [float(v) for v in _NUM.findall(out)], [float(v) for v in _NUM.findall(want)]
    assert np.abs(np.array(got_n) - np.array(want_n)).max() <= tol, (got_n, want_n)


def namespace(**kw):
    return argparse.Namespace(**kw)
