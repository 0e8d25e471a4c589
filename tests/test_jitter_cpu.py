"""TRAIN --jitter without a GPU: the numpy twin of the kernel's rule (tests/jitter_cases.py) against the installed Pillow's ImageEnhance
chain, the command line, the random stream and item tuples with and without the flag, collate / upload, the args.yml and .ptl round
trip, and the header's declarations."""
import argparse
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

import jitter_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAMP = np.arange(256, dtype=np.uint8)
SPREAD = [np.float32(0), np.float32(1), np.float32(2)] + list(np.random.default_rng(5).uniform(0, 2, 13).astype(np.float32))


def _with_mean(m, rgb=False):
    """the 0..255 ramp plus filler pixels of level m, enough of them that the rounded mean level is m"""
    a = np.concatenate([RAMP, np.full(256 * 255, m, np.uint8)]).reshape(-1, 256)
    if rgb:
        a = np.stack([a, a, a], -1)                   # R = G = B = v gives L = v: (19595 + 38470 + 7471) v + 0x8000 >> 16
    assert jc.mean_level(a) == m
    return a


def test_brightness_table_equals_pillow_over_the_ramp():
    for rgb in (False, True):
        a = np.stack([RAMP[None]] * 3, -1) if rgb else RAMP[None]
        for f in SPREAD:
            want = jc.pillow_jitter(a, fb=f)
            assert np.array_equal(jc.jitter(a, fb=f), want), (rgb, f)
            assert np.array_equal(jc.lut(f, 0)[a], want)
    assert np.array_equal(jc.lut(1, 0), RAMP) and not jc.lut(0, 0).any() and jc.lut(2, 0)[128:].min() == 255


def test_contrast_table_equals_pillow_for_every_mean_level():
    """exhaustive: every mean level 0..255 times every input level, factors 0, 1, 2 and a seeded spread in [0, 2]"""
    for m in range(256):
        a = _with_mean(m)
        img = Image.fromarray(a)
        for f in SPREAD:
            from PIL import ImageEnhance
            want = np.asarray(ImageEnhance.Contrast(img).enhance(float(f)))
            assert np.array_equal(jc.lut(f, m)[a], want), (m, f)
        assert np.array_equal(jc.lut(1, m), RAMP) and (jc.lut(0, m) == m).all()
    for m in (0, 1, 77, 128, 254, 255):
        a = _with_mean(m, rgb=True)
        for f in SPREAD[:7]:
            assert np.array_equal(jc.jitter(a, fc=f), jc.pillow_jitter(a, fc=f)), (m, f)


def test_brightness_then_contrast_takes_the_mean_after_brightness():
    rng = np.random.default_rng(11)
    for shape in ((23, 31), (1, 1), (1, 17), (40, 9, 3), (5, 7, 3), (64, 64, 3)):
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        for fb in SPREAD[:8]:
            for fc in SPREAD[:8]:
                got = jc.jitter(a, fb, fc)
                assert np.array_equal(got, jc.pillow_jitter(a, fb, fc)), (shape, fb, fc)
        # the mean is the brightened image's, not the source's
        b = jc.jitter(a, fb=np.float32(0.37))
        if a.size > 1 and jc.mean_level(b) != jc.mean_level(a):
            other = jc.lut(np.float32(1.63), jc.mean_level(a))[b]
            assert np.array_equal(jc.jitter(a, 0.37, 1.63), jc.lut(np.float32(1.63), jc.mean_level(b))[b])
            assert not np.array_equal(jc.jitter(a, 0.37, 1.63), other) or a.size < 4
    # RGB luma with unequal channels
    a = rng.integers(0, 256, (37, 29, 3), dtype=np.uint8)
    assert jc.mean_level(a) == int(np.asarray(Image.fromarray(a).convert('L')).astype(np.int64).sum() * 2 + 37 * 29) // (2 * 37 * 29)
    # a factor that is not finite or negative: identity
    for f in (jc.NAN, jc.INF, -jc.INF, -0.5):
        assert np.array_equal(jc.jitter(a, f, f), a)


def test_jitter_command_line():
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import parse_jitter
    p = nn_.argparse_nn()
    base = ['TRAIN', 'src', 'resnet18', 'id1']
    assert p.parse_args(base).jitter is None
    assert p.parse_args(base + ['--jitter', '0.2']).jitter == [0.2, 0.0]
    assert p.parse_args(base + ['--jitter', '0.2,0.3']).jitter == [0.2, 0.3]
    assert p.parse_args(base + ['--jitter', '0,0.3']).jitter == [0.0, 0.3]
    assert p.parse_args(base + ['--jitter', '0']).jitter is None and p.parse_args(base + ['--jitter', '0,0']).jitter is None
    t = p.parse_args(base + ['--flip', 'xy', '--rot90', '--jitter', '0.5,1.5', '--pad'])
    assert (t.flip, t.rot90, t.jitter, t.pad) == ('xy', 'T', [0.5, 1.5], 'border')
    for bad in ('-0.1', 'nan', 'a', '1,2,3', 'inf', '0.1,-1', '0.1,', ''):
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--jitter=' + bad])
    with pytest.raises(SystemExit):
        p.parse_args(['RUN', 'src', 'm.ptl', 'rid', '--jitter', '0.2'])
    assert parse_jitter([0.2, 0.3]) == [0.2, 0.3] and parse_jitter((0, 0)) is None and parse_jitter(None) is None
    for bad in ([1, 2, 3], [True, 0], [-1, 0], [float('nan'), 0]):
        with pytest.raises(ValueError):
            parse_jitter(bad)


def _parent_flip_code(vflip, hflip, rot90):
    """RoiTransform.flip_code's draw sequence before jitter existed"""
    from ifcb_classifier_amd.neuston_data import fold_turns
    code = 0
    if vflip and random.random() < 0.5:
        code |= 1
    if hflip and random.random() < 0.5:
        code |= 2
    if rot90:
        code = fold_turns(code & 1, code >> 1, random.randrange(4))
    return code


def _dataset(tmp_path, **kw):
    from ifcb_classifier_amd.neuston_data import NeustonDataset, RoiTransform
    if not os.path.isdir(tmp_path / 'a'):
        for cls in ('a', 'b'):
            os.makedirs(tmp_path / cls)
            for i in range(6):
                Image.fromarray(np.full((6, 9), 20 * i + 1, np.uint8)).save(str(tmp_path / cls / ('%s%d.png' % (cls, i))))
    return NeustonDataset(str(tmp_path), transforms=RoiTransform(224, None, True, True, **kw))


def test_codes_and_random_stream_of_a_seeded_dataset(tmp_path):
    """unset: the item tuples and the random stream are those of the draw sequence before the flag.  Set: the codes are still those of
    the flip / turn draws (made first), the factors follow (brightness, then contrast, a zero range draws nothing) and lie in range."""
    for rot in (False, True):
        ds = _dataset(tmp_path, rot90=rot)
        assert ds.transforms.jitter is None
        random.seed(5)
        items = [ds[i % len(ds)] for i in range(60)] + [random.random()]
        random.seed(5)
        want = [_parent_flip_code(True, True, rot) for _ in range(60)] + [random.random()]
        assert [it[0][1] for it in items[:-1]] + items[-1:] == want
        assert all(len(it[0]) == (3 if rot else 2) for it in items[:-1])
        for B, C in ((0.4, 0.0), (0.0, 0.7), (0.3, 1.5)):
            ds = _dataset(tmp_path, rot90=rot, jitter=[B, C])
            random.seed(5)
            items = [ds[i % len(ds)] for i in range(60)]
            tail = random.random()
            random.seed(5)
            codes, fbs, fcs = [], [], []
            for _ in range(60):
                codes.append(_parent_flip_code(True, True, rot))
                fbs.append(float(np.float32(random.uniform(max(0.0, 1 - B), 1 + B))) if B else None)
                fcs.append(float(np.float32(random.uniform(max(0.0, 1 - C), 1 + C))) if C else None)
            assert tail == random.random()
            assert [it[0][1] for it in items] == codes and all(it[0][2] is rot and len(it[0]) == 5 for it in items)
            assert [it[0][3] for it in items] == fbs and [it[0][4] for it in items] == fcs
            for f, r in ((fbs, B), (fcs, C)):
                if r:
                    lo, hi = np.float32(max(0.0, 1 - r)), np.float32(1 + r)
                    assert all(lo <= v <= hi and v == float(np.float32(v)) for v in f) and len(set(f)) > 50


def test_only_the_training_transform_jitters():
    from ifcb_classifier_amd.neuston_data import ImageDataset, RoiTransform, get_trainval_transforms
    a = argparse.Namespace(MODEL='resnet18', img_norm=None, flip='xy+V', rot90='+V', pad='border', jitter=[0.2, 0.3])
    train, val = get_trainval_transforms(a)
    assert train.jitter == [0.2, 0.3] and val.jitter is None and val.rot90 and val.vflip and val.pad == 'border'
    train, val = get_trainval_transforms(argparse.Namespace(MODEL='resnet18', img_norm=None, flip=None))          # an args object without the key
    assert train.jitter is None and val.jitter is None
    assert RoiTransform(224).jitter is None and RoiTransform(224, jitter='0').jitter is None and RoiTransform(224, jitter='0.1').jitter == [0.1, 0.0]
    assert RoiTransform(224).jitter_factors() == (None, None)
    assert ImageDataset(['a.png'], resize=224).transform.jitter is None


def test_collate_and_upload_carry_the_factors_only_when_drawn():
    from ifcb_classifier_amd.neuston_data import RoiTransform, collate_rois, rois_to_device
    imgs = [np.full((5, 3), 7, np.uint8), np.full((2, 4), 9, np.uint8)]
    plain = collate_rois([((imgs[0], 0), 1, 'a'), ((imgs[1], 3), 0, 'b')])[0]
    assert sorted(plain) == ['flips', 'hs', 'in_channels', 'max_h', 'max_w', 'offs', 'pixels', 'ws']                # today's keys
    assert sorted(collate_rois([((imgs[0], 0, True), 1, 'a'), ((imgs[1], 3, True), 0, 'b')])[0]) == sorted(list(plain) + ['turn'])
    assert sorted(rois_to_device(plain, 'cpu', RoiTransform(224, jitter=[0.2, 0.2]))) == \
        ['flips', 'hs', 'in_channels', 'max_h', 'max_w', 'offs', 'pixels', 'ws']                                    # no factors in the batch: none uploaded
    both = collate_rois([((imgs[0], 0, False, 0.75, 1.25), 1, 'a'), ((imgs[1], 3, False, 1.5, 0.5), 0, 'b')])[0]
    assert sorted(both) == sorted(list(plain) + ['brightness', 'contrast']) and 'turn' not in both
    assert both['brightness'].dtype == torch.float32 and both['brightness'].tolist() == [0.75, 1.5] and both['contrast'].tolist() == [1.25, 0.5]
    kw = rois_to_device(both, 'cpu')
    assert kw['jitter'][0].tolist() == [0.75, 1.5] and kw['jitter'][1].tolist() == [1.25, 0.5] and 'turn' not in kw
    b_only = collate_rois([((imgs[0], 0, True, 0.75, None), 1, 'a'), ((imgs[1], 5, True, 1.5, None), 0, 'b')])[0]
    assert 'contrast' not in b_only and b_only['turn'] is True and b_only['flips'].tolist() == [0, 5]
    kw = rois_to_device(b_only, 'cpu')
    assert kw['jitter'][1] is None and kw['jitter'][0].tolist() == [0.75, 1.5] and kw['turn'] is True
    c_only = collate_rois([((imgs[0], 0, False, None, 0.25), 1, 'a')])[0]
    assert 'brightness' not in c_only and rois_to_device(c_only, 'cpu')['jitter'][0] is None


def test_jitter_round_trips_through_args_yml_and_the_ptl(tmp_path):
    import yaml
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import parse_jitter
    from ifcb_classifier_amd.neuston_models import load_checkpoint_file
    p = nn_.argparse_nn()
    for argv, want in ((['--jitter', '0.2'], [0.2, 0.0]), (['--jitter', '0.25,0.5'], [0.25, 0.5]), (['--jitter', '0'], None), ([], None)):
        args = p.parse_args(['TRAIN', 'src', 'resnet18', 'id1'] + argv)
        text = yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v)) for k, v in vars(args).items()})
        back = yaml.safe_load(text)
        assert back['jitter'] == want and type(back['jitter']) is type(want)
        hp = dict(vars(argparse.Namespace(**vars(args))), classes=['a', 'b'])
        path = str(tmp_path / ('m%d.ptl' % len(argv + [str(want)])))
        torch.save(dict(hyper_parameters=hp, state_dict={}), path)
        got = load_checkpoint_file(path)['hyper_parameters']
        assert got['jitter'] == want and parse_jitter(getattr(argparse.Namespace(**got), 'jitter', None)) == want
    path = str(tmp_path / 'old.ptl')                                                                     # a checkpoint without the key
    torch.save(dict(hyper_parameters=dict(MODEL='resnet18', classes=['a', 'b']), state_dict={}), path)
    assert getattr(argparse.Namespace(**load_checkpoint_file(path)['hyper_parameters']), 'jitter', None) is None


def test_header_prototypes_and_makefile_name_the_entry_points():
    from ifcb_classifier_amd import _lib
    hdr = re.sub(r'\s+', ' ', open(os.path.join(ROOT, 'include', 'ifcbk.h')).read())
    assert 'IFCBK_API size_t ifcbk_roi_jitter_workspace(int n_img);' in hdr
    assert re.search(r'IFCBK_API int ifcbk_roi_jitter\(ifcbk_ctx\*, const uint8_t\* pixels, const int64_t\* offs, const int32_t\* hs, '
                     r'const int32_t\* ws, int n_img, int in_channels', hdr)
    assert 'ifcbk_roi_jitter' in _lib.EXPORTS and 'ifcbk_roi_jitter_workspace' in _lib.EXPORTS
    assert len(_lib._PROTOS['ifcbk_roi_jitter'][1]) == 13
    mk = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'Makefile')).read()
    assert 'roi_jitter.hip' in mk and '-ffp-contract=on' in mk
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'roi_jitter.hip')).read()
    assert '__fadd_rn((float)m, __fmul_rn(f, (float)(v - m)))' in src                  # two roundings, whatever the contraction flag says
    assert 'constexpr int JCHUNK = JT * JUNITS * 16;' in src and 'constexpr int JT = 256;' in src and 'constexpr int JUNITS = 4;' in src
    assert jc.CHUNK == 256 * 4 * 16
