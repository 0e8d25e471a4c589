"""Every arithmetic path of ifcbk_roi_preprocess (csrc/roi.hip) bit for bit against the Pillow-equal oracle, and its float stage
per element against float64 (tests/roi_bounds.py: the case table, the path predicates and the bounds; tests/test_roi_paths_cpu.py
proves on the CPU that the oracle equals the installed Pillow for every shape used here, so no Pillow is needed on the GPU box).

Each run allocates out, out_u8 and the pixel blob between poisoned margins: the margins must come back untouched, and the bytes
behind the blob (and in the gaps of a non-packed blob) must not influence the result.  (The coefficient workspace belongs to the
context and has no address a test can put a margin around; its size formula is checked against the table layout in the CPU twin.)"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import roi_bounds as rb

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MARGIN = 4096           # bytes on both sides (a multiple of 16: the float stores are 16-byte vectors)


def _guarded(nbytes, poison):
    buf = torch.full((MARGIN + nbytes + MARGIN,), poison, dtype=torch.uint8, device='cuda')
    return buf, buf[MARGIN:MARGIN + nbytes]


def _margins_intact(name, buf, nbytes, poison):
    b = buf.cpu()
    assert bool((b[:MARGIN] == poison).all()), '%s: bytes in front of the buffer were written' % name
    assert bool((b[MARGIN + nbytes:] == poison).all()), '%s: bytes behind the buffer were written' % name


def run(ctx, case, rois, poison=0xA5, layout='packed'):
    """-> (out [n][S][S][cout] or None, u8 [n][S][S][cin] numpy or None)"""
    from ifcb_classifier_amd import _lib
    n, S, cin, cout = len(rois), case['S'], case['cin'], case['cout']
    hs = torch.tensor([r.shape[0] for r in rois], dtype=torch.int32)
    ws = torch.tensor([r.shape[1] for r in rois], dtype=torch.int32)
    sizes = [int(r.size) for r in rois]
    order = list(range(n)) if layout == 'packed' else list(range(n - 1, -1, -1))      # 'reverse': last ROI first, 7 poison bytes between
    gap = 0 if layout == 'packed' else 7
    offs = [0] * n
    pos = gap
    for i in order:
        offs[i] = pos
        pos += sizes[i] + gap
    blob = np.full(pos + MARGIN, poison, np.uint8)                                     # poison behind the last ROI
    for i in order:
        blob[offs[i]:offs[i] + sizes[i]] = rois[i].reshape(-1)
    pix = torch.from_numpy(blob).cuda()
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels = n, S, cin, cout
    d.dtype = _lib.BF16 if case['dtype'] == 'bf16' else _lib.F32
    d.flip_bits_valid = 1 if case['flips'] is not None else 0
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = case['mean'][k], case['std'][k], case['tsc'][k], case['tsh'][k]
    mh, mw = rb.maxima(case)
    need = ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), mh, mw)
    assert need == n * 2 * S * (2 + rb.kmax(case)) * 4
    ctx.reserve(need)
    esz = 2 if case['dtype'] == 'bf16' else 4
    tdt = torch.bfloat16 if case['dtype'] == 'bf16' else torch.float32
    ob_, ov = _guarded(n * S * S * cout * esz, poison) if case['out'] else (None, None)
    ub_, uv = _guarded(n * S * S * cin, poison) if case['u8'] else (None, None)
    # flip_bits_valid = 0: the flips array is handed over all the same and must be ignored
    fl = torch.tensor(case['flips'] if case['flips'] is not None else [3] * n, dtype=torch.uint8).cuda()
    offs_d, hs_d, ws_d = torch.tensor(offs, dtype=torch.int64).cuda(), hs.cuda(), ws.cuda()
    ctx.call('ifcbk_roi_preprocess', C.byref(d), _lib.ptr(pix), _lib.ptr(offs_d), _lib.ptr(hs_d), _lib.ptr(ws_d), _lib.ptr(fl), mh, mw,
             _lib.ptr(ov), _lib.ptr(uv), _lib.cur_stream())
    torch.cuda.synchronize()
    out = u8 = None
    if case['out']:
        _margins_intact(case['name'] + ' out', ob_, ov.numel(), poison)
        out = ov.view(tdt).reshape(n, S, S, cout).clone()
    if case['u8']:
        _margins_intact(case['name'] + ' out_u8', ub_, uv.numel(), poison)
        u8 = uv.reshape(n, S, S, cin).cpu().numpy()
    assert bool((pix.cpu()[pos:] == poison).all())
    return out, u8


@pytest.mark.parametrize('case', rb.ROI, ids=[c['name'] for c in rb.ROI])
def test_roi_paths_u8_bit_exact_and_float_stage_bounded(ctx, case):
    rois = rb.pixels(case)
    want = rb.expected_u8(case, rois)
    out, u8 = run(ctx, case, rois)
    if case['u8']:
        rb.check_u8(case['name'], u8, want)
    if case['out']:
        # (out_u8 = NULL: the float output must still be the one derived from the expected plane)
        rb.check_float(case['name'], out, want, case)
    # poison behind the blob and another blob layout: the same bytes out
    out2, u82 = run(ctx, case, rois, poison=0x3C, layout='reverse')
    if case['u8']:
        assert np.array_equal(u8, u82), case['name']
    if case['out']:
        assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8)), case['name']


def test_overstated_maxima_move_the_batch_to_a_slower_path_with_identical_planes(ctx):
    by = {c['name']: c for c in rb.ROI}
    cases = [by['small299 norm'], by['small299 as kmax5'], by['small299 as kmax7']]
    assert [rb.kmax(c) for c in cases] == [3, 5, 7]
    assert [set(rb.paths(c)) for c in cases] == [{'roi_resize3_kernel'}, {'roi_resize_kernel lds_ok'}, {'roi_resize_kernel generic'}]
    rois = rb.pixels(cases[0])
    res = [run(ctx, c, rois) for c in cases]
    for o, u in res[1:]:
        assert np.array_equal(u, res[0][1])
        assert torch.equal(o.view(torch.uint8), res[0][0].view(torch.uint8))


@pytest.mark.parametrize('S', [299, 224])
def test_each_golden_roi_in_a_batch_of_its_own_vs_pillow_sha256(ctx, S):
    """every committed Pillow vector down the path its own size selects (pil_resize_cases: the original twelve shapes;
    pil_resize_order_cases: shapes inside and just outside the vertical-first region)"""
    seen = set()
    for stem in ('pil_resize_cases', 'pil_resize_order_cases'):
        z = np.load(os.path.join(GOLD, stem + '.npz'))
        for c in json.load(open(os.path.join(GOLD, stem + '.json')))['cases']:
            if c['S'] != S:
                continue
            roi = z['in_%d' % c['case']]
            case = rb._case('golden %dx%d' % roi.shape, [tuple(roi.shape)], S, flips=None)
            out, u8 = run(ctx, case, [roi])
            assert hashlib.sha256(u8[0, :, :, 0].tobytes()).hexdigest() == c['sha256'], c
            rb.check_float(case['name'], out, u8, case, family=None)
            seen |= set(rb.paths(case))
    assert seen == {'roi_resize3_kernel', 'roi_resize_kernel lds_ok', 'roi_resize_kernel generic'}
