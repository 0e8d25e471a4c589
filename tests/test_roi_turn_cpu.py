"""CPU twin of tests/test_gpu_roi_turn.py (TRAIN --rot90): the folding of (vflip, hflip, k quarter turns) into the kernel's code
byte against numpy and Pillow, the oracle against the installed Pillow on every turned shape of the case table, the path predicates
of roi_turn_cases.py against the text of roi_turn.hip, the random stream of RoiTransform.flip_code, the command line, and the
``turn`` flag through collate_rois / rois_to_device."""
import argparse
import os
import random
import re

import numpy as np
import pytest
import torch

import roi_bounds as rb
import roi_turn_cases as tc
from oracle import pil_resize as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Image = pytest.importorskip('PIL.Image')


def _norm(s):
    return re.sub(r'\s+', ' ', s)


def test_folded_code_equals_numpy_rot90_and_the_pillow_chain():
    from ifcb_classifier_amd.neuston_data import fold_turns
    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)              # non-square, distinct values
    codes = {}
    for v in (0, 1):
        for h in (0, 1):
            for k in range(4):
                code = fold_turns(v, h, k)
                assert 0 <= code < 8 and (code >= 4) == (k % 2 == 1)
                f = a[::-1] if v else a
                f = f[:, ::-1] if h else f
                want = np.rot90(f, k)
                assert np.array_equal(tc.seen(a, code), want), (v, h, k, code)
                im = Image.fromarray(a, 'L')
                if v:
                    im = im.transpose(Image.FLIP_TOP_BOTTOM)
                if h:
                    im = im.transpose(Image.FLIP_LEFT_RIGHT)
                for _ in range(k):
                    im = im.transpose(Image.ROTATE_90)
                assert np.array_equal(np.asarray(im), want), (v, h, k)
                codes.setdefault(code, []).append((v, h, k))
    # 16 chains, 8 symmetries, two chains each: --flip xy --rot90 is uniform over the symmetries of the square
    assert sorted(codes) == list(range(8)) and all(len(c) == 2 for c in codes.values())
    # the eight codes are eight different images, and k + 4 is k
    assert len({tc.seen(a, c).tobytes() + bytes(tc.seen(a, c).shape) for c in range(8)}) == 8
    assert fold_turns(1, 0, 6) == fold_turns(1, 0, 2)


def test_oracle_equals_installed_pillow_on_every_turned_case_shape():
    seen = {}
    for c in tc.TURN:
        for (h, w), code in zip(c['rois'], c['flips']):
            seen.setdefault((h, w, code & 4, c['S'], c['cin']), code)
    assert len(seen) > 150
    rng = np.random.default_rng(9)
    for (h, w, _, S, cin), code in sorted(seen.items()):
        a = rng.integers(0, 256, (h, w) if cin == 1 else (h, w, 3), dtype=np.uint8)
        t = tc.seen(a, code)
        assert t.shape[:2] == tc.seen_dims(h, w, code)
        pil = np.asarray(Image.fromarray(t, 'L' if cin == 1 else 'RGB').resize((S, S), Image.BILINEAR))
        assert np.array_equal(PR.resize_bilinear_u8(t, S, S), pil), (h, w, code, S)


def test_turn_path_predicates_quote_the_source_and_every_path_is_reached_turned_and_unturned():
    src = _norm(open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'roi_turn.hip')).read())
    for name, (pred, cond) in tc.PATHS.items():
        assert _norm(cond) in src, '%s: %r is no longer in roi_turn.hip' % (name, cond)
    for q in tc.QUOTED:
        assert _norm(q) in src, q
    shared = _norm(open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'roi_resample.h')).read())
    for q in tc.rb.QUOTED_SHARED:
        assert _norm(q) in shared, q
    assert _norm(tc.BRANCH) in _norm(open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'roi.hip')).read())
    reached = {p: set() for p in tc.PATHS}
    vf = set()
    for c in tc.TURN:
        assert {f & 4 for f in c['flips']} == {0, 4}, c['name']                # every batch mixes turned and unturned images
        for (h, w), code, p, v in zip(c['rois'], c['flips'], tc.paths(c), tc.vfirst(c)):
            if h != w:
                reached[p].add(code)
                reached['roi_turn_coeffs_kernel'].add(code)
            if v:
                vf.add((p, bool(code & 4)))
    for p, codes in reached.items():
        assert codes == set(range(8)), '%s: codes on non-square ROIs %s' % (p, sorted(codes))
    assert vf == {(p, t) for p in ('roi_turn_resize_kernel staged', 'roi_turn_resize_kernel generic') for t in (True, False)}
    by = {c['name']: c for c in tc.TURN}
    # the statements of the case table's comments
    c = by['turn mid299']
    order = {}
    for (h, w), code, v in zip(c['rois'], c['flips'], tc.vfirst(c)):
        order[(h, w, bool(code & 4))] = v
    for hw in ((5, 598), (4, 597), (5, 501)):
        assert order[hw + (True,)] and not order[hw + (False,)]
    assert order[(598, 5, False)] and not order[(598, 5, True)]
    for hw in ((6, 598), (5, 500)):
        assert not order[hw + (True,)] and not order[hw + (False,)]
    assert set(tc.paths(c)) == {'roi_turn_resize_kernel staged'} and rb.kmax(c) == 5
    c = by['turn wide384']
    assert rb.kmax(c) == 5
    pv = {(h, w, bool(code & 4)): (p, v) for (h, w), code, p, v in zip(c['rois'], c['flips'], tc.paths(c), tc.vfirst(c))}
    assert pv[(30, 641, False)][0].endswith('generic') and pv[(30, 641, True)][0].endswith('staged')
    assert pv[(641, 30, True)][0].endswith('generic') and pv[(641, 30, False)][0].endswith('staged')
    assert pv[(6, 641, True)] == ('roi_turn_resize_kernel staged', True) and not pv[(6, 641, False)][1]
    assert pv[(100, 640, True)][0].endswith('staged') and pv[(640, 100, True)][0].endswith('staged')
    c = by['turn wide299']
    assert rb.kmax(c) == 7 and set(tc.paths(c)) == {'roi_turn_resize_kernel generic'}
    assert [v for (h, w), code, v in zip(c['rois'], c['flips'], tc.vfirst(c)) if (h, w) == (6, 641)] == [False, True] and c['flips'][7] & 4
    assert rb.kmax(by['turn big224']) == 11 and rb.kmax(by['turn small384']) == 3
    assert {c['S'] for c in tc.TURN if set(tc.paths(c)) == {'roi_turn_resize3_kernel'}} == {299, 224, 40}
    assert any(c['cout'] == 16 for c in tc.TURN) and any(not c['out'] for c in tc.TURN) and any(not c['u8'] for c in tc.TURN)
    assert {c['dtype'] for c in tc.TURN} == {'bf16', 'fp32'} and any(c['cin'] == 3 for c in tc.TURN)


def test_band_of_a_row_block_fits_the_strip():
    """roi_turn_resize3_kernel stages, per block of BAND_RPB = 8 output rows, rows first .. last of the turned image, at most BAND_ROWS = 12
    of them: for every input size <= S the 8 rows' windows span at most 10 rows"""
    for S in (299, 224, 40, 320):
        for size in range(1, S + 1):
            bounds = PR._coeffs(size, S)[0]
            for y0 in range(0, S, 8):
                y1 = min(y0 + 7, S - 1)
                assert bounds[y1][0] + bounds[y1][1] - bounds[y0][0] <= 10, (S, size, y0)
                assert all(bounds[y][0] >= bounds[y0][0] and bounds[y][0] + bounds[y][1] <= bounds[y1][0] + bounds[y1][1] for y in range(y0, y1 + 1))


def _parent_flip_code(vflip, hflip):
    """the two-draw logic of RoiTransform.flip_code before rot90 existed"""
    code = 0
    if vflip and random.random() < 0.5:
        code |= 1
    if hflip and random.random() < 0.5:
        code |= 2
    return code


def test_flip_code_random_stream_is_unchanged_without_rot90_and_covers_eight_codes_with_it():
    from ifcb_classifier_amd.neuston_data import RoiTransform, get_trainval_transforms
    for v, h in ((False, False), (True, False), (False, True), (True, True)):
        t = RoiTransform(224, None, v, h)
        assert t.rot90 is False
        random.seed(12)
        got = [t.flip_code() for _ in range(200)] + [random.random()]
        random.seed(12)
        want = [_parent_flip_code(v, h) for _ in range(200)] + [random.random()]
        assert got == want
    random.seed(1)
    t = RoiTransform(224, None, True, True, rot90=True)
    draws = [t.flip_code() for _ in range(400)]
    assert set(draws) == set(range(8)) and min(draws.count(c) for c in range(8)) > 25
    t = RoiTransform(224, None, rot90=True)
    assert {t.flip_code() for _ in range(200)} == {0, 3, 5, 6}             # the four rotations: id, 180, and the two quarter turns
    for rot, tr, va in ((None, False, False), ('T', True, False), ('+V', True, True)):
        a = argparse.Namespace(MODEL='resnet18', img_norm=None, flip='x', rot90=rot)
        train, val = get_trainval_transforms(a)
        assert (train.rot90, val.rot90) == (tr, va) and train.vflip and not val.vflip
    train, val = get_trainval_transforms(argparse.Namespace(MODEL='resnet18', img_norm=None, flip=None))      # an args object without the key
    assert not train.rot90 and not val.rot90


def test_rot90_command_line():
    from ifcb_classifier_amd import neuston_net as nn_
    p = nn_.argparse_nn()
    base = ['TRAIN', 'src', 'resnet18', 'id1']
    t = p.parse_args(base)
    assert t.rot90 is None and t.flip is None
    assert (t.optimizer, t.learning_rate, t.momentum, t.precision) == ('Adam', 0.001, 0.0, 'bf16')
    assert p.parse_args(base + ['--rot90']).rot90 == 'T'
    assert p.parse_args(base + ['--rot90', '+V']).rot90 == '+V'
    t = p.parse_args(base + ['--flip', 'xy', '--rot90', '--emax', '3'])
    assert (t.flip, t.rot90, t.emax) == ('xy', 'T', 3)
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--rot90', '45'])
    with pytest.raises(SystemExit):
        p.parse_args(['RUN', 'src', 'm.ptl', 'rid', '--rot90'])


def test_collate_and_upload_carry_the_turn_flag_whatever_the_draw():
    from ifcb_classifier_amd.neuston_data import RoiTransform, collate_rois, rois_to_device
    imgs = [np.full((5, 3), 7, np.uint8), np.full((2, 4), 9, np.uint8)]
    plain = collate_rois([((imgs[0], 0), 1, 'a'), ((imgs[1], 3), 0, 'b')])[0]
    assert 'turn' not in plain and plain['flips'].tolist() == [0, 3]
    kw = rois_to_device(plain, 'cpu')
    assert 'turn' not in kw and kw['flips'].tolist() == [0, 3]
    assert 'flips' not in rois_to_device(collate_rois([((imgs[0], 0), 1, 'a')])[0], 'cpu')        # as before: no codes, none uploaded
    # all codes zero, the transform turns: flagged, and the codes are handed over all the same
    turned = collate_rois([((imgs[0], 0, True), 1, 'a'), ((imgs[1], 0, True), 0, 'b')])[0]
    assert turned['turn'] is True and turned['flips'].tolist() == [0, 0]
    kw = rois_to_device(turned, 'cpu')
    assert kw['turn'] is True and kw['flips'].tolist() == [0, 0]
    assert (kw['max_h'], kw['max_w']) == (5, 4)                                                  # the SOURCE dims
    mixed = collate_rois([((imgs[0], 6, True), 1, 'a'), ((imgs[1], 1, True), 0, 'b')])[0]
    assert rois_to_device(mixed, 'cpu')['flips'].tolist() == [6, 1]
    # a transform with rot90 marks a batch collated elsewhere
    kw = rois_to_device(plain, 'cpu', RoiTransform(224, None, rot90=True))
    assert kw['turn'] is True and kw['flips'].tolist() == [0, 3]


def test_dataset_items_carry_the_flag_only_under_a_turning_transform(tmp_path):
    from ifcb_classifier_amd.neuston_data import NeustonDataset, RoiTransform, collate_rois
    for cls in ('a', 'b'):
        os.makedirs(tmp_path / cls)
        for i in range(2):
            Image.fromarray(np.full((6, 9), 40 * i + 1, np.uint8)).save(str(tmp_path / cls / ('%s%d.png' % (cls, i))))
    ds = NeustonDataset(str(tmp_path), transforms=RoiTransform(224))
    assert len(ds[0][0]) == 2 and 'turn' not in collate_rois([ds[0], ds[1]])[0]
    ds = NeustonDataset(str(tmp_path), transforms=RoiTransform(224, rot90=True))
    random.seed(0)
    items = [ds[i] for i in range(len(ds))]
    assert all(it[0][2] is True and it[0][1] in (0, 3, 5, 6) for it in items)
    assert collate_rois(items)[0]['turn'] is True
