"""TRAIN --pad on the GPU: every path of ifcbk_roi_preprocess_fit (csrc/roi_fit.hip) bit for bit against the numpy twin of
PIL.ImageOps.pad (tests/roi_fit_cases.py; tests/test_roi_fit_cpu.py proves the twin equal to the installed Pillow), the float stage
per element against float64, the workspace size with guard bytes behind it, square ROIs against ifcbk_roi_preprocess, the error
returns, Engine.load_rois(pad=...) and one TRAIN --pad / RUN round trip through the command line.

Each run allocates out, out_u8 and the pixel blob between poisoned margins: the margins must come back untouched."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import roi_bounds as rb
import roi_fit_cases as fc
from test_gpu_roi_turn import MARGIN, _batch, _guarded, _kw, _margins_intact, _prefetch
from test_gpu_roi_turn import run as run_squash

pytestmark = pytest.mark.gpu
CANARY = 4096


class _Raw:
    """device bytes at a raw address, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr='|u1', data=(int(ptr), False), version=2, strides=None)


def _arena(ctx, off, n):
    base = ctx.lib.ifcbk_ctx_workspace_ptr(ctx.h)
    assert base and ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h) >= off + n
    return torch.as_tensor(_Raw(base + off, n), device='cuda')


def run(ctx, case, rois, valid=2, codes=None, poison=0xA5, fill=None, maxima=None):
    """-> (out [n][S][S][cout] or None, u8 [n][S][S][cin] numpy or None)"""
    from ifcb_classifier_amd import _lib
    n, S, cin, cout = len(rois), case['S'], case['cin'], case['cout']
    codes = case['flips'] if codes is None else codes
    hs = torch.tensor([r.shape[0] for r in rois], dtype=torch.int32)
    ws = torch.tensor([r.shape[1] for r in rois], dtype=torch.int32)
    sizes = [int(r.size) for r in rois]
    offs, pos = [], MARGIN
    for s in sizes:
        offs.append(pos)
        pos += s
    blob = np.full(pos + MARGIN, poison, np.uint8)
    for o, s, r in zip(offs, sizes, rois):
        blob[o:o + s] = r.reshape(-1)
    pix = torch.from_numpy(blob).cuda()
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels = n, S, cin, cout
    d.dtype = _lib.BF16 if case['dtype'] == 'bf16' else _lib.F32
    d.flip_bits_valid = valid
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = case['mean'][k], case['std'][k], case['tsc'][k], case['tsh'][k]
    mh, mw = maxima or rb.maxima(case)
    need = ctx.lib.ifcbk_roi_preprocess_fit_workspace(C.byref(d), mh, mw)
    assert need == fc.workspace_bytes(n, S, fc.fit_kmax(mh, mw, S))
    if ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h) < need + CANARY:
        ctx.reserve(need + CANARY)
    canary = _arena(ctx, need, CANARY)
    canary.fill_(poison)
    esz = 2 if case['dtype'] == 'bf16' else 4
    tdt = torch.bfloat16 if case['dtype'] == 'bf16' else torch.float32
    ob_, ov = _guarded(n * S * S * cout * esz, poison) if case['out'] else (None, None)
    ub_, uv = _guarded(n * S * S * cin, poison) if case['u8'] else (None, None)
    fl = torch.tensor(codes, dtype=torch.uint8).cuda()
    offs_d, hs_d, ws_d = torch.tensor(offs, dtype=torch.int64).cuda(), hs.cuda(), ws.cuda()
    ctx.call('ifcbk_roi_preprocess_fit', C.byref(d), _lib.ptr(pix), _lib.ptr(offs_d), _lib.ptr(hs_d), _lib.ptr(ws_d), _lib.ptr(fl), mh, mw,
             fc.fill_arg(case) if fill is None else fill, _lib.ptr(ov), _lib.ptr(uv), _lib.cur_stream())
    torch.cuda.synchronize()
    assert bool((canary == poison).all()), case['name'] + ': bytes behind the workspace were written'
    out = u8 = None
    if case['out']:
        _margins_intact(case['name'] + ' out', ob_, ov.numel(), poison)
        out = ov.view(tdt).reshape(n, S, S, cout).clone()
    if case['u8']:
        _margins_intact(case['name'] + ' out_u8', ub_, uv.numel(), poison)
        u8 = uv.reshape(n, S, S, cin).cpu().numpy()
    assert np.array_equal(pix.cpu().numpy(), blob), case['name'] + ': the blob was written'
    return out, u8


@pytest.mark.parametrize('case', fc.FIT, ids=[c['name'] for c in fc.FIT])
def test_fit_paths_u8_bit_exact_float_stage_bounded_and_fill_exact(ctx, case):
    rois = rb.pixels(case)
    want = fc.expected_u8(case, rois)
    out, u8 = run(ctx, case, rois)
    if case['u8']:
        rb.check_u8(case['name'], u8, want)
    if case['out']:
        rb.check_float(case['name'], out, want, case)
        # fill pixels: one value per image and channel, the one an inner pixel of that level gets
        inner = torch.from_numpy(fc.inner_mask(case))
        w3 = torch.from_numpy(np.repeat(want, 3, -1) if case['cin'] == 1 else want)
        o = out.cpu().view(torch.int16 if case['dtype'] == 'bf16' else torch.int32)
        for i, f in enumerate(fc.fills(case, rois)):
            outside = ~inner[i]
            if not bool(outside.any()):
                continue
            for c in range(3):
                vals = o[i, :, :, c][outside]
                assert bool((vals == vals[0]).all()), (case['name'], i, c)
                level = f[c if case['cin'] == 3 else 0]
                assert bool((w3[i, :, :, c][outside] == level).all())
                same = (w3[:, :, :, c] == level) & inner
                if bool(same.any()):
                    assert bool((o[:, :, :, c][same] == vals[0]).all()), (case['name'], i, c)
    # another poison value: the same bytes out
    out2, u82 = run(ctx, case, rois, poison=0x3C)
    if case['u8']:
        assert np.array_equal(u8, u82), case['name']
    if case['out']:
        assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8)), case['name']


def test_square_rois_give_the_bytes_of_the_squash_call_for_every_fill(ctx):
    for S, shapes, extra in ((299, [(299, 299), (1, 1), (57, 57), (221, 221), (7, 7), (300, 300), (598, 598)], dict(mean=fc.MEAN, std=fc.STD)),
                             (224, [(224, 224), (3, 3), (100, 100), (150, 150)], dict(dtype='fp32', tsc=fc.TSC, tsh=fc.TSH)),
                             (299, [(41, 41), (299, 299), (350, 350), (1, 1)], dict(cin=3))):
        case = fc._fcase('square %d %s' % (S, sorted(extra)), shapes, S, 'border', **extra)
        rois = rb.pixels(case)
        o0, u0 = run_squash(ctx, case, rois)
        for fill in (-1, 0, 255, 131):
            o1, u1 = run(ctx, case, rois, fill=fill)
            assert np.array_equal(u0, u1), (case['name'], fill)
            assert torch.equal(o0.view(torch.uint8), o1.view(torch.uint8)), (case['name'], fill)


def test_codes_are_read_as_flip_bits_valid_says(ctx):
    """0: no code counts; 1: flips only (bit 2 ignored); 2: all three bits"""
    case = fc._fcase('valid', [(20, 31), (31, 20), (40, 9), (5, 5)], 40, 'border')
    rois = rb.pixels(case)
    codes = case['flips']
    assert {c & 4 for c in codes} == {0, 4}
    for valid, eff in ((0, [0] * len(codes)), (1, [c & 3 for c in codes]), (2, codes)):
        _, u8 = run(ctx, case, rois, valid=valid)
        rb.check_u8('valid %d' % valid, u8, fc.expected_u8(case, rois, eff))


def test_error_returns(ctx):
    from ifcb_classifier_amd import _lib
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels, d.dtype, d.flip_bits_valid = 1, 40, 1, 8, _lib.BF16, 0
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
    pix = torch.zeros(64, dtype=torch.uint8, device='cuda')
    offs = torch.zeros(1, dtype=torch.int64, device='cuda')
    hs = torch.full((1,), 8, dtype=torch.int32, device='cuda')
    ws = torch.full((1,), 8, dtype=torch.int32, device='cuda')
    u8 = torch.zeros(40 * 40, dtype=torch.uint8, device='cuda')

    def call(desc, mh, mw, fill, out_u8):
        rc = ctx.lib.ifcbk_roi_preprocess_fit(ctx.h, C.byref(desc), _lib.ptr(pix), _lib.ptr(offs), _lib.ptr(hs), _lib.ptr(ws), None, mh, mw, fill,
                                              None, _lib.ptr(out_u8), _lib.cur_stream())
        return rc, ctx.lib.ifcbk_last_error(ctx.h).decode()

    EINVAL = -1
    for args, word in (((d, 8, 8, 256, u8), 'fill'), ((d, 8, 8, -2, u8), 'fill'), ((d, 8, 8, -1, None), 'NULL'), ((d, 0, 8, -1, u8), 'max dims'),
                       ((d, 8, 0, 0, u8), 'max dims')):
        rc, msg = call(*args)
        assert rc == EINVAL and word in msg, (args[1:4], rc, msg)
    bad = _lib.RoiDesc.from_buffer_copy(d)
    bad.in_channels = 2
    rc, msg = call(bad, 8, 8, 0, u8)
    assert rc == EINVAL and 'bad desc' in msg
    empty = _lib.RoiDesc.from_buffer_copy(d)
    empty.n_img = 0
    assert call(empty, 8, 8, 999, None)[0] == 0                    # n_img = 0 is a no-op, whatever else is handed over
    assert ctx.lib.ifcbk_roi_preprocess_fit_workspace(C.byref(empty), 8, 8) == 0
    rc, _ = call(d, 8, 8, 17, u8)
    torch.cuda.synchronize()
    assert rc == 0 and int(u8.view(40, 40)[0, 0]) == 0 and bool((u8 == 0).all())        # a black square ROI fills the plane: no fill pixel


SHAPES4 = [(57, 131), (299, 88), (30, 299), (120, 45)]


@pytest.mark.parametrize('stem', ['1', '0'])
def test_engine_load_rois_pad_on_inception_v3(monkeypatch, stem):
    """the u8-stem branch (IFCBK_STEM_U8 unset / 1) and the tensor branch (IFCBK_STEM_U8=0) see the same padded plane, the prefetch slot
    equals the current slot, and pad=None is today's call bit for bit"""
    monkeypatch.setenv('IFCBK_STEM_U8', stem)
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 4
    rois = _batch(SHAPES4, 31)
    codes = [4, 7, 2, 5]
    case = fc._fcase('engine', SHAPES4, 299, 'border')
    case = dict(case, rois=SHAPES4, flips=codes)
    e = Engine(graph.build('inception_v3', 4), 0, max_batch=B)
    assert (e.stem_u8 is not None) == (stem == '1')
    dev = _kw(rois, flips=torch.tensor(codes, dtype=torch.uint8).cuda(), turn=True)

    def plane(slot):
        torch.cuda.synchronize()
        if stem == '1':
            assert e.in_kind[slot] == 'u8'
            return e.in_u8[slot][:B].clone().cpu().numpy()[..., None]
        assert e.in_kind[slot] == 'nhwc'
        return e.in_bufs[slot][:B].clone()

    def check(got, want_u8):
        if stem == '1':
            rb.check_u8('engine plane', got, want_u8)
        else:
            tin = e.net.transform_input
            fcase = dict(case, dtype='bf16' if e.in_bufs[0].dtype == torch.bfloat16 else 'fp32', mean=(0, 0, 0), std=(1, 1, 1),
                         tsc=tuple(s / 0.5 for s in (0.229, 0.224, 0.225)) if tin else (1, 1, 1),
                         tsh=tuple((m - 0.5) / 0.5 for m in (0.485, 0.456, 0.406)) if tin else (0, 0, 0))
            rb.check_float('engine tensor', got.reshape(B, 299, 299, -1), want_u8, fcase)

    for pad in ('border', 0, 200):
        want = fc.expected_u8(dict(case, fill=pad), rois)
        e.load_rois(pad=pad, **dev)
        cur = plane(e.in_slot)
        check(cur, want)
        slot = _prefetch(e, dict(dev, pad=pad))
        pre = plane(slot)
        assert e.in_slot == slot
        assert np.array_equal(cur, pre) if stem == '1' else torch.equal(cur.view(torch.uint8), pre.view(torch.uint8))
    # pad=None: the squash call, as without the argument
    e.load_rois(**dev)
    a = plane(e.in_slot)
    e.load_rois(pad=None, **dev)
    b = plane(e.in_slot)
    assert np.array_equal(a, b) if stem == '1' else torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    if stem == '1':
        import roi_turn_cases as tc
        rb.check_u8('engine squash plane', a, tc.expected_u8(case, rois))
    with pytest.raises(ValueError):
        e.load_rois(pad=256, **dev)
    del e


def _make_dataset(root, per_class=5):
    from PIL import Image
    rng = np.random.default_rng(17)
    for cls, mean in (('cls_a', 90), ('cls_b', 170)):
        os.makedirs(os.path.join(root, cls))
        for i in range(per_class):
            h, w = (int(rng.integers(20, 40)), int(rng.integers(120, 200))) if i % 2 else (int(rng.integers(120, 200)), int(rng.integers(15, 30)))
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(root, cls, 'roi_%s_%02d.png' % (cls, i)))


def test_cli_train_pad_then_run_from_the_ptl(tmp_path, monkeypatch):
    """TRAIN --pad on a tiny dataset of non-square ROIs, one epoch, then RUN --type img from its .ptl: the scores are eval_batch's on
    the padded input, not on the squashed one; args.yml and the .ptl hold ``pad``"""
    import yaml
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import ImageDataset, RoiTransform, collate_rois, rois_to_device
    from ifcb_classifier_amd.neuston_models import NeustonModel, load_checkpoint_file
    src = str(tmp_path / 'data')
    os.makedirs(src)
    _make_dataset(src)
    outdir = str(tmp_path / 'out')
    args = nn_.argparse_nn().parse_args(['--batch', '8', '--loaders', '0', 'TRAIN', src, 'resnet18', 'pd', '--untrain', '--seed', '1', '--emax', '1',
                                         '--emin', '1', '--estop', '0', '--outdir', outdir, '--pad'])
    assert args.pad == 'border'
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    ptl = os.path.join(outdir, 'pd.ptl')
    assert yaml.safe_load(open(os.path.join(outdir, 'args.yml')))['pad'] == 'border'
    assert load_checkpoint_file(ptl)['hyper_parameters']['pad'] == 'border'

    got = []
    test = nn_.Trainer.test
    monkeypatch.setattr(nn_.Trainer, 'test', lambda self, *a: (lambda r: (got.append(r[0]), r)[1])(test(self, *a)))
    rargs = nn_.argparse_nn().parse_args(['--batch', '16', '--loaders', '0', 'RUN', src, ptl, 'r1', '--type', 'img', '--outdir', str(tmp_path / 'run'),
                                          '--outfile', 'img_results.json'])
    nn_.argparse_nn_runtimeparams(rargs)
    nn_.main(rargs)
    rr = got[0]
    assert len(rr.inputs) == 10
    m = NeustonModel.load_from_checkpoint(ptl, max_batch=16, inference=True)
    assert m.hparams.pad == 'border'
    ds = ImageDataset(list(rr.inputs), resize=224)
    batch = collate_rois([ds[i] for i in range(len(ds))])[0]
    scores = {}
    for pad in ('border', None):
        probs, _ = m.eval_batch(rois_to_device(batch, m.model.engine.dev, RoiTransform(224, pad=pad)))
        torch.cuda.synchronize()
        scores[pad] = probs.float().cpu().numpy()
    assert np.array_equal(np.asarray(rr.outputs, np.float32), scores['border'])
    assert not np.array_equal(scores['border'], scores[None])
