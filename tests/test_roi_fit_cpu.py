"""CPU twin of tests/test_gpu_roi_fit.py (TRAIN --pad): the numpy twin of roi_fit_cases.py against PIL.ImageOps.pad of the installed
Pillow on every case shape and code and on a wider grid, the clamp shapes against a hand-built expectation, border_fill against a
brute-force mask sum, the path predicates against the text of roi_fit.hip, the tap bound, and the ``pad`` setting through the command
lines, RoiTransform / rois_to_device, args.yml, the .ptl and the ONNX metadata."""
import argparse
import os
import random
import re

import numpy as np
import pytest
import torch

import roi_bounds as rb
import roi_fit_cases as fc
from oracle import pil_resize as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')


def _norm(s):
    return re.sub(r'\s+', ' ', s)


def _pil_pad(img, S, fill):
    Image = pytest.importorskip('PIL.Image')            # only the two comparisons with Pillow need it
    ImageOps = pytest.importorskip('PIL.ImageOps')
    mode = 'L' if img.ndim == 2 else 'RGB'
    color = int(fill[0]) if mode == 'L' else tuple(int(f) for f in fill)
    out = ImageOps.pad(Image.fromarray(img, mode), (S, S), Image.BILINEAR, color=color, centering=(0.5, 0.5))
    return np.asarray(out).reshape(S, S, -1)


def test_fit_dims_gaps_and_ties():
    assert fc.fit_dims(40, 40, 40) == (40, 40, 0, 0)
    assert fc.fit_dims(40, 39, 40) == (40, 39, 0, 0)               # a gap of 1: the extra line behind the image
    assert fc.fit_dims(37, 40, 40) == (37, 40, 2, 0)               # a gap of 3: two lines in front
    assert fc.fit_dims(10, 20, 40) == (20, 40, 10, 0) and fc.fit_dims(20, 10, 40) == (40, 20, 0, 10)
    assert fc.fit_dims(597, 598, 299) == (298, 299, 0, 0)          # 298.5 -> 298, half to even
    assert fc.fit_dims(598, 5, 299) == (299, 2, 0, 148) and fc.fit_dims(598, 21, 299) == (299, 10, 0, 144)
    assert fc.fit_dims(600, 1, 299) == (299, 1, 0, 149) and fc.fit_dims(640, 3, 299) == (299, 1, 0, 149)       # clamped / rounded to 1
    assert fc.fit_dims(1, 1, 299) == (299, 299, 0, 0)


def test_numpy_twin_equals_imageops_pad_on_every_case_shape_and_code():
    todo = {}
    for c in fc.FIT:
        for (h, w), code in zip(c['rois'], c['flips']):
            todo.setdefault((h, w, code & 4, c['S'], c['cin']), code)
    rng = np.random.default_rng(11)
    clamp = 0
    for (h, w, _, S, cin), code in sorted(todo.items()):
        a = rng.integers(0, 256, (h, w) if cin == 1 else (h, w, 3), dtype=np.uint8)
        t = fc.seen(a, code)
        for fill in (fc.border_fill(a), [0] * cin, [255] * cin):
            got = fc.fit_u8(t, S, fill)
            if fc.contain_is_zero(t.shape[0], t.shape[1], S):
                clamp += fill == [0] * cin
                assert (h, w) in fc.CLAMP
                # hand-built: a 1-pixel-wide inner image, the seen image resized along its long axis only
                ht, wt = t.shape[:2]
                want = np.empty((S, S, cin), np.uint8)
                want[:] = np.asarray(fill, np.uint8)
                if ht > wt:
                    col = PR.resize_bilinear_u8(t, S, 1).reshape(S, 1, cin)
                    want[:, round((S - 1) * 0.5):round((S - 1) * 0.5) + 1] = col
                else:
                    row = PR.resize_bilinear_u8(t, 1, S).reshape(1, S, cin)
                    want[round((S - 1) * 0.5):round((S - 1) * 0.5) + 1] = row
                assert np.array_equal(got, want), (h, w, code, S)
                continue
            assert np.array_equal(got, _pil_pad(t, S, fill)), (h, w, code, S, fill)
    # (600, 1) and (1, 600) at 299, each turned and unturned ((640, 3) and (301, 2) round to 1 without the clamp)
    assert clamp == 4


GRID_S = (299, 224, 160, 384)
# the clamp shapes of the case table, at their sizes: the only grid points where ImageOps.contain asks for a zero size
GRID_CLAMP = [(600, 1, 299), (1, 600, 299)]


def _grid():
    shapes = list(GRID_CLAMP)
    for S in GRID_S:
        for h, w in ((598, 5), (1000, 9), (2000, 19), (2000, 21), (301, 2), (5, 598), (1212, 12), (1213, 12), (707, 7), (708, 7), (101, 1), (203, 2),
                     (2 * S + 1, 20), (S, S - 1), (S + 1, S), (S - 1, S), (2 * S - 1, 2 * S), (3, 5), (5, 3), (2, 7), (1, 2), (2, 1), (S // 2, S // 3),
                     (3 * S + 1, 31), (7, S + 2), (S + 2, 7), (150, 61), (1, 1), (2, 2), (33, 34), (3 * S, 2 * S), (4 * S + 3, 4 * S + 2)):
            shapes += [(h, w, S), (w, h, S)]
    return sorted(set(shapes))


def test_numpy_twin_equals_imageops_pad_on_a_wider_grid_including_the_vertical_first_region():
    rng = np.random.default_rng(12)
    left_out, vf = [], set()
    for h, w, S in _grid():
        if fc.contain_is_zero(h, w, S):
            left_out.append((h, w, S))
            continue
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        nh = fc.fit_dims(h, w, S)[0]
        if PR.vertical_first(h, w, nh):
            vf.add(S)
        fill = fc.border_fill(a)
        assert np.array_equal(fc.fit_u8(a, S, fill), _pil_pad(a, S, fill)), (h, w, S)
    assert vf == set(GRID_S)                                       # h > 100 w at every S
    # left out: the listed clamp shapes and nothing else
    assert len(left_out) == 2 and sorted(left_out) == sorted(GRID_CLAMP)
    assert {(h, w) for h, w, _ in GRID_CLAMP} == fc.CLAMP


def test_border_fill_against_a_brute_force_mask_sum():
    rng = np.random.default_rng(13)
    for h in (1, 2, 3, 4, 7):
        for w in (1, 2, 3, 5, 40):
            for cin in (1, 3):
                a = rng.integers(0, 256, (h, w) if cin == 1 else (h, w, 3), dtype=np.uint8)
                mask = np.zeros((h, w), bool)
                mask[0] = mask[-1] = True
                mask[:, 0] = mask[:, -1] = True
                if h <= 2 or w <= 2:
                    assert mask.all()
                px = a.reshape(h, w, cin)[mask].astype(np.int64)
                want = [int(np.floor(s / len(px) + 0.5)) for s in px.sum(0)]
                assert fc.border_fill(a) == want, (h, w, cin)
                # invariant under flips and transposes
                for code in range(8):
                    assert fc.border_fill(fc.seen(a, code)) == want
    a = np.zeros((5, 5), np.uint8)
    a[1:4, 1:4] = 255                                             # the interior does not count
    assert fc.border_fill(a) == [0]
    assert fc.border_fill(np.array([[1, 2]], np.uint8)) == [2]    # 1.5 rounds up


def test_fit_path_predicates_quote_the_source_and_every_path_is_reached():
    src = _norm(open(os.path.join(CSRC, 'roi_fit.hip')).read())
    for name, (pred, cond) in fc.PATHS.items():
        assert _norm(cond) in src, '%s: %r is no longer in roi_fit.hip' % (name, cond)
    for q in fc.QUOTED:
        assert _norm(q) in src, q
    shared = _norm(open(os.path.join(CSRC, 'roi_resample.h')).read())
    for q in fc.tc.rb.QUOTED_SHARED:
        assert _norm(q) in shared, q
    dims = _norm(open(os.path.join(CSRC, 'roi_fit_dims.h')).read())
    for q in fc.QUOTED_DIMS:
        assert _norm(q) in dims, q
    # every kernel of roi_fit.hip has a predicate
    kernels = set(re.findall(r'__global__ (?:__launch_bounds__\(\d+\) )?void (\w+)\(', src))
    assert kernels == {'roi_fit_setup_kernel', 'roi_fit_resize3_kernel', 'roi_fit_resize_kernel'}
    assert kernels == {p.split(' ')[0] for p in fc.PATHS}
    assert 'roi_fit.hip' in open(os.path.join(CSRC, 'Makefile')).read()
    reached = {p: set() for p in fc.PATHS}
    vf = set()
    for c in fc.FIT:
        assert {f & 4 for f in c['flips']} == {0, 4}, c['name']
        for (h, w), code, ps, v in zip(c['rois'], c['flips'], fc.paths(c), fc.vfirst(c)):
            for p in ps:
                reached[p].add(code & 4)
                if v:
                    vf.add(p)
    for p, t in reached.items():
        assert t == {0, 4}, '%s: reached turned / unturned: %s' % (p, sorted(t))
    assert {'roi_fit_resize_kernel staged', 'roi_fit_resize_kernel generic'} <= vf and 'roi_fit_resize3_kernel' not in vf
    by = {c['name']: c for c in fc.FIT}
    assert fc.kmax(by['fit small40']) == 3 and fc.kmax(by['fit small299 fill77']) == 3
    assert fc.kmax(by['fit mid299']) == 9 and fc.kmax(by['fit mid224 fp32 fill128']) == 7 and fc.kmax(by['fit stage384']) == 7
    # the 640-wide staging limit decides on the seen width: (30, 641) is generic unturned and staged turned, (641, 30) the reverse
    c = by['fit stage384']
    pv = {(h, w, bool(code & 4)): ps for (h, w), code, ps in zip(c['rois'], c['flips'], fc.paths(c))}
    assert 'roi_fit_resize_kernel generic' in pv[(30, 641, False)] and 'roi_fit_resize_kernel staged' in pv[(30, 641, True)]
    assert 'roi_fit_resize_kernel generic' in pv[(641, 30, True)] and 'roi_fit_resize_kernel staged' in pv[(641, 30, False)]
    assert all(pv[(200, 321, t)] >= {'roi_fit_resize_kernel staged'} for t in (True, False))
    # fill modes and output forms of the issue's list
    assert {c['fill'] for c in fc.FIT} >= {'border', 0, 255, 128}
    assert any(c['cout'] == 16 for c in fc.FIT) and any(not c['out'] for c in fc.FIT) and any(not c['u8'] for c in fc.FIT)
    assert {c['dtype'] for c in fc.FIT} == {'bf16', 'fp32'} and any(c['cin'] == 3 for c in fc.FIT)
    # every shape of the issue's table is in a batch of its group
    for name, shapes in (('fit small40', fc.S40), ('fit mid299', fc.S299), ('fit mid224 fp32 fill128', fc.S224), ('fit stage384', fc.S384),
                         ('fit rgb299', fc.RGB299)):
        assert by[name]['rois'] == shapes + shapes


def test_tap_bound_holds_where_the_squash_bound_does_not():
    """ifcbk_fit_kmax against the windows Pillow's coefficient maths gives for the fitted sizes"""
    worst = {}
    for S in (299, 224, 40):
        for L in list(range(1, 2 * S + 40)) + [3 * S, 3 * S + 1, 4 * S - 1, 1000, 2000]:
            k = fc.fit_kmax(L, L, S)
            for s in sorted({1, 2, 3, 4, 5, 7, 10, 21, L // 100 + 1, L // 3 + 1, L - 1, L} & set(range(1, L + 1))):
                nh, nw, _, _ = fc.fit_dims(L, s, S)
                t = max(int(PR._coeffs(s, nw)[0][:, 1].max()), int(PR._coeffs(L, nh)[0][:, 1].max()))
                assert t <= k, (L, s, S, t, k)
                if t > rb.kmax_for(L, L, S):
                    worst[(L, s, S)] = t
    # a window that holds more taps than the squash path's table has room for: 1000 x 334 at 40 has nw = 13, a scale of 25.7 against
    # 1000 / 40 = 25, and windows of 52 taps against kmax_for's 51
    assert worst.get((1000, 334, 40)) == 52 and rb.kmax_for(1000, 1000, 40) == 51 and fc.fit_kmax(1000, 1000, 40) == 77
    # the issue's examples: the short axis's scale exceeds the squash bound's max / S = 2.0, so Pillow's table width 2 ceil(scale) + 1
    # exceeds kmax_for (their windows themselves are cut to 4 and 5 taps by an input of 5 and 21 pixels)
    for (h, w), scale in (((598, 5), 2.5), ((598, 21), 2.1)):
        nw = fc.fit_dims(h, w, 299)[1]
        assert w / nw == scale and scale > max(h, w) / 299
        assert int(np.ceil(scale)) * 2 + 1 > rb.kmax_for(h, w, 299) and int(np.ceil(scale)) * 2 + 1 <= fc.fit_kmax(h, w, 299)
    assert fc.fit_kmax(299, 299, 299) == 3 and fc.fit_kmax(300, 1, 299) == 5 and fc.fit_kmax(598, 598, 299) == 7


def test_band_of_a_row_block_fits_the_strip_for_every_enlarging_axis():
    """roi_fit_resize3_kernel stages, per block of BAND_RPB = 8 output rows, at most BAND_ROWS = 12 rows: 8 consecutive inner rows of an axis that
    does not shrink (input size <= inner size <= S) span at most 10 input rows"""
    for S in (299, 40):
        for n_out in sorted({S, S - 1, S // 2, S // 3, 7, 2, 1}):
            for size in range(1, n_out + 1):
                b = PR._coeffs(size, n_out)[0]
                assert int(b[:, 1].max()) <= 3
                for lo in range(n_out):
                    hi = min(lo + 7, n_out - 1)
                    assert b[hi][0] + b[hi][1] - b[lo][0] <= 10, (S, n_out, size, lo)


# ------------------------------------------------------------------------------------------ host plumbing
def test_pad_command_line():
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd import neuston_util as nu
    p = nn_.argparse_nn()
    base = ['TRAIN', 'src', 'resnet18', 'id1']
    assert p.parse_args(base).pad is None
    assert p.parse_args(base + ['--pad']).pad == 'border'
    assert p.parse_args(base + ['--pad', 'border']).pad == 'border'
    assert p.parse_args(base + ['--pad', '0']).pad == 0 and p.parse_args(base + ['--pad', '255']).pad == 255
    t = p.parse_args(base + ['--flip', 'xy', '--pad', '--rot90', '--emax', '3'])
    assert (t.flip, t.pad, t.rot90, t.emax) == ('xy', 'border', 'T', 3)
    for bad in ('256', '-2', 'x', '1.5', ''):
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--pad', bad])
    with pytest.raises(SystemExit):
        p.parse_args(['RUN', 'src', 'm.ptl', 'rid', '--pad'])       # RUN has no flag of its own
    assert 'behind the positionals' in _norm(p._subparsers._group_actions[0].choices['TRAIN'].format_help())
    u = nu.argparse_init()
    assert u.parse_args(['CALC_IMG_NORM', 'src']).pad is None
    assert u.parse_args(['CALC_IMG_NORM', 'src', '--pad']).pad == 'border'
    assert u.parse_args(['CALC_IMG_NORM', 'src', '--pad', '17']).pad == 17
    with pytest.raises(SystemExit):
        u.parse_args(['CALC_IMG_NORM', 'src', '--pad', '256'])


def _parent_flip_code(vflip, hflip):
    code = 0
    if vflip and random.random() < 0.5:
        code |= 1
    if hflip and random.random() < 0.5:
        code |= 2
    return code


def test_transform_and_upload_carry_pad_and_draw_nothing_for_it():
    from ifcb_classifier_amd._lib import pad_fill
    from ifcb_classifier_amd.neuston_data import (IfcbBinDataset, ImageDataset, RoiTransform, collate_rois, get_trainval_transforms, parse_pad,
                                                  rois_to_device)
    assert RoiTransform(224).pad is None and RoiTransform(224, pad='border').pad == 'border' and RoiTransform(224, pad='7').pad == 7
    for bad in (256, -1, 'x', True, 1.5):
        with pytest.raises(ValueError):
            RoiTransform(224, pad=bad)
    assert (pad_fill('border'), pad_fill(0), pad_fill(255)) == (-1, 0, 255)
    for bad in (None, 256, -1, '7'):
        with pytest.raises(ValueError):
            pad_fill(bad)
    assert parse_pad(np.int64(5)) == 5 and isinstance(parse_pad(np.int64(5)), int)
    # geometry, not augmentation: both transforms, no random number
    a = argparse.Namespace(MODEL='resnet18', img_norm=None, flip='xy', rot90=None, pad=40)
    train, val = get_trainval_transforms(a)
    assert (train.pad, val.pad) == (40, 40) and train.vflip and not val.vflip
    train, val = get_trainval_transforms(argparse.Namespace(MODEL='resnet18', img_norm=None, flip=None))      # an args object without the key
    assert train.pad is None and val.pad is None
    for pad in (None, 'border'):
        t = RoiTransform(224, None, True, True, pad=pad)
        random.seed(12)
        got = [t.flip_code() for _ in range(200)] + [random.random()]
        random.seed(12)
        want = [_parent_flip_code(True, True) for _ in range(200)] + [random.random()]
        assert got == want
    imgs = [np.full((5, 3), 7, np.uint8), np.full((2, 4), 9, np.uint8)]
    batch = collate_rois([((imgs[0], 0), 1, 'a'), ((imgs[1], 3), 0, 'b')])[0]
    assert 'pad' not in batch
    # absent: the kwargs of today
    assert sorted(rois_to_device(batch, 'cpu')) == ['flips', 'hs', 'in_channels', 'max_h', 'max_w', 'offs', 'pixels', 'ws']
    assert sorted(rois_to_device(batch, 'cpu', RoiTransform(224))) == ['flips', 'hs', 'in_channels', 'max_h', 'max_w', 'offs', 'pixels', 'ws']
    kw = rois_to_device(batch, 'cpu', RoiTransform(224, pad='border'))
    assert kw['pad'] == 'border' and 'turn' not in kw
    assert rois_to_device(batch, 'cpu', RoiTransform(224, ((0.5,) * 3, (0.2,) * 3), pad=0))['pad'] == 0          # level 0 is a setting, not "unset"
    kw = rois_to_device(batch, 'cpu', RoiTransform(224, rot90=True, pad=9))
    assert kw['pad'] == 9 and kw['turn'] is True
    assert ImageDataset(['a.png'], resize=224, pad='border').transform.pad == 'border' and ImageDataset(['a.png'], resize=224).transform.pad is None

    class _Pid:
        def with_target(self, n):
            return n

    class _Bin:
        pid, schema, images = _Pid(), 'v2', {1: np.zeros((3, 4), np.uint8)}
    assert IfcbBinDataset(_Bin(), 224, pad=3).transform.pad == 3 and IfcbBinDataset(_Bin(), 224).transform.pad is None


def test_pad_round_trips_through_args_yml_the_ptl_and_the_onnx_metadata(tmp_path):
    import yaml
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd import onnx_export
    from ifcb_classifier_amd.neuston_data import parse_pad
    from ifcb_classifier_amd.neuston_models import load_checkpoint_file
    p = nn_.argparse_nn()
    for argv, want in ((['--pad'], 'border'), (['--pad', '0'], 0), (['--pad', '200'], 200), ([], None)):
        args = p.parse_args(['TRAIN', 'src', 'resnet18', 'id1'] + argv)
        # args.yml as do_training writes it
        text = yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v)) for k, v in vars(args).items()})
        back = yaml.safe_load(text)
        assert back['pad'] == want and type(back['pad']) is type(want)
        # the .ptl's hyper_parameters as checkpoint_dict writes them (a Namespace's vars), read by the tolerant unpickler
        hp = dict(vars(argparse.Namespace(**vars(args))), classes=['a', 'b'])
        path = str(tmp_path / ('m%s.ptl' % want))
        torch.save(dict(hyper_parameters=hp, state_dict={}), path)
        got = load_checkpoint_file(path)['hyper_parameters']
        assert got['pad'] == want and parse_pad(getattr(argparse.Namespace(**got), 'pad', None)) == want
    # a checkpoint without the key
    path = str(tmp_path / 'old.ptl')
    torch.save(dict(hyper_parameters=dict(MODEL='resnet18', classes=['a', 'b']), state_dict={}), path)
    assert getattr(argparse.Namespace(**load_checkpoint_file(path)['hyper_parameters']), 'pad', None) is None
    # ONNX metadata through onnx_export's own decoder
    assert onnx_export.read_pad({}) is None and onnx_export.read_pad({'ifcbk.model': 'resnet18'}) is None
    assert onnx_export.read_pad({'ifcbk.pad': 'border'}) == 'border' and onnx_export.read_pad({'ifcbk.pad': '0'}) == 0
    with pytest.raises(ValueError):
        onnx_export.read_pad({'ifcbk.pad': '300'})


def test_onnx_file_carries_pad_only_when_set_and_export_reads_it_from_the_ptl(tmp_path):
    from ifcb_classifier_amd import neuston_onnx, onnx_export
    from oracle.tv_models import get_namebrand_model
    torch.manual_seed(0)
    sd = get_namebrand_model('squeezenet', 3, False).state_dict()
    for pad, want in ((None, None), ('border', 'border'), (0, 0), (255, 255)):
        path = str(tmp_path / 'm.onnx')
        onnx_export.export(sd, 'squeezenet', ['a', 'b', 'c'], False, path, pad=pad)
        meta = onnx_export.read(path)['metadata']
        assert ('ifcbk.pad' in meta) == (pad is not None)
        assert onnx_export.read_pad(meta) == want
    # EXPORT of a .ptl: with the key, and an older file without it
    for hp_pad, want in (({'pad': 'border'}, 'border'), ({'pad': 12}, 12), ({'pad': None}, None), ({}, None)):
        ptl = str(tmp_path / 'm.ptl')
        torch.save(dict(hyper_parameters=dict(MODEL='squeezenet', classes=['a', 'b', 'c'], pretrained=False, **hp_pad),
                        state_dict={'model.' + k: v for k, v in sd.items()}), ptl)
        out, _ = neuston_onnx.main(['EXPORT', ptl])
        assert onnx_export.read_pad(onnx_export.read(out)['metadata']) == want
