"""TRAIN --resident without a GPU: ResidentSet.build draws nothing and holds what default_loader gives, file by file; the resident loader's
order is ShardedLoader's; the per-item draws of the resident path are those of a DataLoader without workers; the flag's argparse
surface and its presence / absence in what args.yml is written from; and the declarations of ifcbk_roi_gather.  The kernel runs in
tests/test_gpu_roi_gather.py, the staging in test_gpu_resident_model.py, the command line in test_gpu_resident_cli.py."""
import argparse
import os
import random
import re

import numpy as np
import pytest
import torch

import resident_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset(tmp_path, kind='grey', **tf):
    from ifcb_classifier_amd.neuston_data import NeustonDataset, RoiTransform
    ds = NeustonDataset(rc.write_tree(str(tmp_path / kind), kind))
    ds.transforms = RoiTransform(224, **tf)
    return ds


def _states():
    return random.getstate(), np.random.get_state(), torch.get_rng_state()


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])


@pytest.mark.parametrize('loaders', [0, 2])
def test_build_draws_nothing_and_holds_default_loader_output_in_dataset_order(tmp_path, loaders):
    from ifcb_classifier_amd.neuston_data import ResidentSet, default_loader
    ds = _dataset(tmp_path, vflip=True, hflip=True, rot90=True, jitter=[0.2, 0.3])
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    before = _states()
    res = ResidentSet.build(ds, loaders)
    assert _same(before, _states())
    assert len(res) == len(ds) == 24 and res.paths == list(ds.images) and res.in_channels == 1
    assert res.targets.dtype == np.int64 and res.targets.tolist() == list(ds.targets)
    assert res.offs.dtype == np.int64 and res.hs.dtype == np.int32 and res.ws.dtype == np.int32 and res.blob.dtype == np.uint8
    assert res.offs.shape == (25,) and res.offs[0] == 0 and res.offs[-1] == res.blob.size
    for i, p in enumerate(ds.images):
        im = default_loader(p)
        assert im.ndim == 2 and (res.hs[i], res.ws[i]) == im.shape
        assert np.array_equal(res.blob[res.offs[i]:res.offs[i + 1]].reshape(im.shape), im)
    assert res.nbytes == res.blob.size + 25 * 8 + 24 * 4 * 2 + 24 * 8
    ds[0]
    assert not _same(before, _states())                              # ... where __getitem__ does draw


@pytest.mark.parametrize('kind', ['rgb', 'mixed'])
def test_a_set_with_an_rgb_image_is_held_with_three_channels(tmp_path, kind):
    from ifcb_classifier_amd.neuston_data import ResidentSet, default_loader
    ds = _dataset(tmp_path, kind)
    res = ResidentSet.build(ds)
    assert res.in_channels == 3
    ndim = set()
    for i, p in enumerate(ds.images):
        im = default_loader(p)
        ndim.add(im.ndim)
        if im.ndim == 2:
            im = np.repeat(im[:, :, None], 3, 2)                    # replicated once, at build time
        assert np.array_equal(res.blob[res.offs[i]:res.offs[i + 1]].reshape(im.shape), im)
    assert ndim == ({3} if kind == 'rgb' else {2, 3})
    assert np.array_equal(np.diff(res.offs), res.hs.astype(np.int64) * res.ws * 3)


def test_check_indices_is_the_range_check_of_the_host_copy(tmp_path):
    from ifcb_classifier_amd.neuston_data import ResidentSet
    res = ResidentSet.build(_dataset(tmp_path))
    assert res.check_indices([0, 23, 5, 5]).tolist() == [0, 23, 5, 5]
    for bad in ([24], [-1, 2], []):
        with pytest.raises(IndexError):
            res.check_indices(bad)


@pytest.mark.parametrize('world,rank', [(1, 0), (2, 0), (2, 1)])
def test_the_resident_order_is_sharded_loaders(tmp_path, world, rank):
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import ResidentSet
    ds = _dataset(tmp_path)
    keep = ds.images[:23]                                            # an odd count: world 2 wraps around
    ds.images, ds.targets = keep, ds.targets[:23]
    res = ResidentSet.build(ds)
    assert nn_.ResidentLoader.indices is nn_.ShardedLoader.indices and nn_.ResidentLoader.__len__ is nn_.ShardedLoader.__len__
    for shuffle in (True, False):
        a = nn_.ShardedLoader(ds, 5, shuffle, 0, rank, world, 3)
        b = nn_.ResidentLoader(ds, res, 5, shuffle, rank, world, 3)
        orders = []
        for epoch in (0, 1):
            a.set_epoch(epoch); b.set_epoch(epoch)
            idx, bounds = b.host_batches()
            assert idx.dtype == np.int64 and idx.tolist() == a.indices() and len(idx) == (12 if world == 2 else 23)
            assert len(b) == len(a) == len(bounds) and bounds[0] == (0, 5) and bounds[-1][1] == len(idx)
            assert all(i1 - i0 == 5 for i0, i1 in bounds[:-1]) and bounds[-1][1] - bounds[-1][0] == len(idx) - 5 * (len(bounds) - 1)
            orders.append(idx.tolist())
        assert (orders[0] != orders[1]) == shuffle
    with pytest.raises(ValueError):
        ds.images = keep[:20]
        nn_.ResidentLoader(ds, res, 5, True, 0, 1, 3)


@pytest.mark.parametrize('tf', [dict(vflip=True, hflip=True), dict(vflip=True, hflip=True, rot90=True), dict(jitter='0.2,0.3'),
                                dict(vflip=True, jitter='0.2'), dict()], ids=['flip xy', 'flip xy rot90', 'jitter 0.2,0.3', 'flip x jitter 0.2', 'plain'])
def test_the_resident_draws_are_those_of_a_dataloader_without_workers(tmp_path, tf):
    from torch.utils.data import DataLoader, Subset
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import collate_rois, draw_items
    ds = _dataset(tmp_path, **tf)
    order = nn_.ShardedLoader(ds, 7, True, 0, 0, 1, 3).indices()
    random.seed(11)
    want = [b[0] for b in DataLoader(Subset(ds, order), batch_size=7, shuffle=False, num_workers=0, collate_fn=collate_rois)]
    end = random.getstate()
    random.seed(11)
    got = [draw_items(ds.transforms, min(7, len(order) - i)) for i in range(0, len(order), 7)]
    assert random.getstate() == end                                  # the same number of draws, so the same stream afterwards
    assert len(got) == len(want) == 4
    keys = ('flips', 'brightness', 'contrast', 'turn')
    for g, w in zip(got, want):
        assert {k for k in keys if k in g} == {k for k in keys if k in w}
        for k in keys[:3]:
            if k in w:
                assert g[k].dtype == w[k].dtype and torch.equal(g[k], w[k]), k
        assert g.get('turn') == w.get('turn')
    if 'jitter' in tf:
        assert 'brightness' in got[0] and ('contrast' in got[0]) == (',' in tf['jitter'])
    if tf.get('rot90'):
        assert got[0].get('turn') is True
    if not tf:
        assert set(got[0]) == {'flips'} and not got[0]['flips'].any()
    assert draw_items(None, 3)['flips'].tolist() == [0, 0, 0]


def test_the_flag_defaults_to_unset_and_only_a_set_flag_reaches_args_yml():
    import yaml
    from ifcb_classifier_amd import neuston_net as nn_
    p = nn_.argparse_nn()
    base = ['--batch', '8', 'TRAIN', 'src', 'resnet18', 'tid']
    off, on = p.parse_args(base), p.parse_args(base + ['--resident'])
    assert off.resident is False and on.resident is True
    assert p.parse_args(['TRAIN', '--resident', 'src', 'resnet18', 'tid']).SRC == 'src'          # a bare switch takes no value
    with pytest.raises(SystemExit):
        p.parse_args(['RUN', 'src', 'm.ptl', 'rid', '--resident'])
    assert nn_.resident_flag(off) is False and not hasattr(off, 'resident')
    assert nn_.resident_flag(on) is True and on.resident is True
    assert nn_.resident_flag(argparse.Namespace()) is False          # a namespace built by hand, without the entry

    def dump(a):                                                     # what do_training writes
        return yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v)) for k, v in vars(a).items()})
    assert 'resident' not in dump(off) and yaml.safe_load(dump(on))['resident'] is True
    assert dump(on).replace('resident: true\n', '') == dump(off)     # the one key
    helps = [a.help for a in p._subparsers._group_actions[0].choices['TRAIN']._actions if a.dest == 'resident']
    assert len(helps) == 1 and 'GPU' in helps[0]
    groups = {g.title: [a.dest for a in g._group_actions] for g in p._subparsers._group_actions[0].choices['TRAIN']._action_groups}
    assert 'resident' in groups['Dataset Adjustments']


def test_header_binding_makefile_and_source_agree_on_the_entry_point():
    from ifcb_classifier_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))
    proto = ('IFCBK_API int ifcbk_roi_gather(ifcbk_ctx*, const uint8_t* src_pixels, const int64_t* src_offs, const int32_t* src_hs, '
             'const int32_t* src_ws, const int64_t* idx , int n, int in_channels , uint8_t* dst_pixels, int64_t dst_capacity, '
             'int64_t* dst_offs , int32_t* dst_hs, int32_t* dst_ws, void* stream);')
    assert proto in flat
    assert "THE RANGE OF idx IS THE CALLER'S CONTRACT" in hdr
    res, args = _lib._PROTOS['ifcbk_roi_gather']
    assert res is _lib._i and len(args) == proto.count(',') + 1 == 14 and args[9] is _lib.C.c_int64 and args[6] is args[7] is _lib._i
    for name, val in (('IFCBK_ROI_GATHER_MAX_N', rc.MAX_N), ('IFCBK_ROI_GATHER_CHUNK', rc.CHUNK)):
        assert re.search(r'#define %s\s+%d\b' % (name, val), hdr), name
    assert (_lib.ROI_GATHER_MAX_N, _lib.ROI_GATHER_CHUNK) == (rc.MAX_N, rc.CHUNK)
    csrc = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')
    srcs = re.search(r'^SRCS\s*=(.*)$', open(os.path.join(csrc, 'Makefile')).read(), re.M).group(1).split()
    assert 'roi_gather.hip' in srcs
    src = open(os.path.join(csrc, 'roi_gather.hip')).read()
    assert 'extern "C" int ifcbk_roi_gather(' in src
    assert 'GT * GUNITS * 16 == IFCBK_ROI_GATHER_CHUNK' in src and 'GITEMS * GS == IFCBK_ROI_GATHER_MAX_N' in src


def test_the_numpy_model_and_the_case_table():
    """the model against a loop over the bytes, and the table holds what the issue lists"""
    blob, offs, hs, ws = rc.layout([(2, 3), (0, 5), (1, 4)], ch=3)
    px, d, h, w = rc.gather(blob, offs, hs, ws, [2, 1, 0, 2], 3)
    assert d.tolist() == [0, 12, 12, 30, 42] and h.tolist() == [1, 0, 2, 1] and w.tolist() == [4, 5, 3, 4]
    assert px.tolist() == blob[offs[2]:offs[2] + 12].tolist() + blob[offs[0]:offs[0] + 18].tolist() + blob[offs[2]:offs[2] + 12].tolist()
    ns = {len(c['idx']) for c in rc.CASES}
    assert {1, 64, 65, 256, 257, 1025, rc.MAX_N} <= ns
    widths = {s[1] for c in rc.CASES for s in c['shapes'] if s[0] == 1}
    assert {rc.CHUNK - 1, rc.CHUNK, rc.CHUNK + 1} <= widths
    assert any(c['ch'] == 3 for c in rc.CASES) and any(c['extra'] > rc.CHUNK for c in rc.CASES)
    assert any((1000, 1200) in c['shapes'] and (1, 1) in c['shapes'] and (3, 5) in c['shapes'] for c in rc.CASES)
    assert len(rc.alignment_case(3)['idx']) == 2 * 16 * 33 <= rc.MAX_N
