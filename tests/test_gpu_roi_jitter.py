"""TRAIN --jitter on the GPU: ifcbk_roi_jitter (csrc/roi_jitter.hip) byte for byte against the numpy twin (tests/jitter_cases.py) and the
installed Pillow's ImageEnhance chain, with 32 guard bytes in front of, between and behind the ROIs, in place and out of place, with
out aligned like pixels and not, twice; the error returns; and Engine.load_rois(jitter=...) against the Pillow-exact resize twins
applied to the Pillow-enhanced ROIs."""
import ctypes as C

import numpy as np
import pytest
import torch

import jitter_cases as jc
import roi_bounds as rb
import roi_fit_cases as fc
import roi_turn_cases as tc

pytestmark = pytest.mark.gpu
CANARY = 256


class _Raw:
    """device bytes at a raw address, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr='|u1', data=(int(ptr), False), version=2, strides=None)


def _f32(v):
    return None if v is None else torch.tensor(v, dtype=torch.float32).cuda()


def run(ctx, case, rois, mode, inplace=False, poison=0xA5, lead=0, out_shift=0, maxima=None):
    """-> the jittered ROIs.  Out of place, ``out`` starts as another poison value: every byte of it outside the ROIs and every byte of
    the blob must come back as it was.  In place the guard bytes must.  out_shift: out is moved by that many bytes against pixels'
    alignment."""
    from ifcb_classifier_amd import _lib
    n, cin = len(rois), case['cin']
    blob, offs = jc.layout(rois, poison=poison, lead=lead)
    pix = torch.from_numpy(blob).cuda()
    assert pix.data_ptr() % 16 == 0
    opoison = poison ^ 0xFF
    obuf = torch.full((blob.size + 16,), opoison, dtype=torch.uint8, device='cuda')
    out = pix if inplace else obuf[out_shift:out_shift + blob.size]
    hs = torch.tensor([r.shape[0] for r in rois], dtype=torch.int32).cuda()
    ws = torch.tensor([r.shape[1] for r in rois], dtype=torch.int32).cuda()
    offs_d = torch.tensor(offs, dtype=torch.int64).cuda()
    fb, fc_ = jc.factors(case, mode)
    b_d, c_d = _f32(fb), _f32(fc_)
    mh, mw = maxima or (max(r.shape[0] for r in rois), max(r.shape[1] for r in rois))
    need = ctx.lib.ifcbk_roi_jitter_workspace(n)
    assert need == 8 * n
    assert ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h) >= need + CANARY
    canary = torch.as_tensor(_Raw(ctx.lib.ifcbk_ctx_workspace_ptr(ctx.h) + need, CANARY), device='cuda')
    canary.fill_(poison)
    ctx.call('ifcbk_roi_jitter', _lib.ptr(pix), _lib.ptr(offs_d), _lib.ptr(hs), _lib.ptr(ws), n, cin, mh, mw, _lib.ptr(b_d), _lib.ptr(c_d),
             _lib.ptr(out), _lib.cur_stream())
    torch.cuda.synchronize()
    assert bool((canary == poison).all()), case['name'] + ': bytes behind the workspace were written'
    res = out.cpu().numpy()
    inside = np.zeros(blob.size, bool)
    for o, r in zip(offs, rois):
        inside[o:o + r.size] = True
    guard = poison if inplace else opoison
    bad = np.flatnonzero(~inside & (res != guard))
    assert bad.size == 0, '%s (%s): %d bytes outside the ROIs were written, first at %d' % (case['name'], mode, bad.size, bad[0])
    if not inplace:
        assert np.array_equal(pix.cpu().numpy(), blob), case['name'] + ': pixels was written by an out-of-place call'
        ob = obuf.cpu().numpy()
        assert (ob[:out_shift] == opoison).all() and (ob[out_shift + blob.size:] == opoison).all()
    return [res[o:o + r.size].reshape(r.shape) for o, r in zip(offs, rois)]


def _check(name, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = g != w
        if bad.any():
            idx = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError('%s: ROI %d %s: %d of %d bytes differ, first at %s: got %d want %d' % (
                name, i, g.shape, int(bad.sum()), g.size, idx, int(g[idx]), int(w[idx])))


def _pillow(case, rois, mode):
    fb, fc_ = jc.factors(case, mode)
    return [jc.pillow_jitter(r, None if fb is None else jc.sane(fb[i]), None if fc_ is None else jc.sane(fc_[i])) for i, r in enumerate(rois)]


@pytest.mark.parametrize('mode', jc.MODES)
@pytest.mark.parametrize('case', jc.CASES, ids=[c['name'] for c in jc.CASES])
def test_jitter_equals_the_twin_and_pillow_byte_for_byte(ctx, case, mode):
    rois = jc.pixels(case)
    want = jc.expected(case, rois, mode)
    _check(case['name'] + ' twin vs Pillow', want, _pillow(case, rois, mode))
    name = '%s (%s)' % (case['name'], mode)
    got = run(ctx, case, rois, mode)
    _check(name, got, want)
    _check(name + ' in place', run(ctx, case, rois, mode, inplace=True), want)
    # twice, with another poison value and the blob moved by 5 bytes: the same bytes
    _check(name + ' second run', run(ctx, case, rois, mode, poison=0x3C, lead=5), got)
    _check(name + ' in place, moved', run(ctx, case, rois, mode, inplace=True, lead=11), got)
    # out not aligned like pixels: bytewise stores
    _check(name + ' out shifted', run(ctx, case, rois, mode, out_shift=3), got)


def test_every_alignment_of_a_roi_that_is_all_head_and_tail(ctx):
    case = jc._case('1x17 every lead', [(1, 17), (1, 31), (1, 16), (2, 16)])
    rois = jc.pixels(case)
    want = jc.expected(case, rois, 'both')
    for lead in range(16):
        _check('lead %d' % lead, run(ctx, case, rois, 'both', lead=lead), want)
        _check('lead %d in place' % lead, run(ctx, case, rois, 'both', inplace=True, lead=lead), want)


def test_understated_maxima_stay_exact(ctx):
    """the grid is sized by max_h x max_w; the blocks stride over what lies behind it"""
    for case in (jc.CASES[3], jc.CASES[5]):
        rois = jc.pixels(case)
        _check(case['name'] + ' maxima 1 x 1', run(ctx, case, rois, 'both', maxima=(1, 1)), jc.expected(case, rois, 'both'))


def test_error_returns(ctx):
    from ifcb_classifier_amd import _lib
    pix = torch.full((64,), 9, dtype=torch.uint8, device='cuda')
    offs = torch.zeros(1, dtype=torch.int64, device='cuda')
    hs = torch.full((1,), 4, dtype=torch.int32, device='cuda')
    ws = torch.full((1,), 4, dtype=torch.int32, device='cuda')
    f = torch.full((1,), 0.5, dtype=torch.float32, device='cuda')
    P = _lib.ptr
    good = dict(pixels=P(pix), offs=P(offs), hs=P(hs), ws=P(ws), n=1, ch=1, b=P(f), c=P(f), out=P(pix))

    def call(**kw):
        a = dict(good, **kw)
        rc = ctx.lib.ifcbk_roi_jitter(ctx.h, a['pixels'], a['offs'], a['hs'], a['ws'], a['n'], a['ch'], 4, 4, a['b'], a['c'], a['out'], _lib.cur_stream())
        return rc, ctx.lib.ifcbk_last_error(ctx.h).decode()

    for kw, word in ((dict(b=None, c=None), 'both NULL'), (dict(n=0), 'n_img'), (dict(n=-3), 'n_img'), (dict(ch=2), 'in_channels'),
                     (dict(ch=0), 'in_channels'), (dict(ch=4), 'in_channels'), (dict(pixels=None), 'NULL'), (dict(offs=None), 'NULL'),
                     (dict(hs=None), 'NULL'), (dict(ws=None), 'NULL'), (dict(out=None), 'NULL')):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((pix == 9).all())                                   # a refused call writes nothing
    assert ctx.lib.ifcbk_roi_jitter_workspace(0) == 0 and ctx.lib.ifcbk_roi_jitter_workspace(7) == 56
    for kw in (dict(c=None), dict(b=None), dict()):
        assert call(**kw)[0] == 0
    torch.cuda.synchronize()
    # in place, the three calls in turn: 9 -> 4 (brightness 0.5), 4 -> 4 (contrast around the mean 4), 4 -> 2 -> 2 (both)
    assert bool((pix[:16] == 2).all()) and bool((pix[16:] == 9).all())


# ------------------------------------------------------------------------------------------------------------------------ the engine
SHAPES4 = [(57, 131), (299, 88), (30, 299), (120, 45)]
FB4, FC4 = [0.37, 1.63, 1.0, 2.0], [1.63, 0.0, 0.37, 1.2]


def _kw(rois, **more):
    hs = np.array([r.shape[0] for r in rois], np.int32)
    ws = np.array([r.shape[1] for r in rois], np.int32)
    offs = np.zeros(len(rois), np.int64)
    offs[1:] = np.cumsum(hs.astype(np.int64) * ws)[:-1]
    blob = np.concatenate([r.reshape(-1) for r in rois])
    kw = dict(pixels=torch.from_numpy(blob).cuda(), offs=torch.from_numpy(offs).cuda(), hs=torch.from_numpy(hs).cuda(),
              ws=torch.from_numpy(ws).cuda(), max_h=int(hs.max()), max_w=int(ws.max()))
    kw.update(more)
    return kw


def _prefetch(e, kw):
    slot, side = e.prefetch_begin()
    with torch.cuda.stream(side):
        e.load_rois(slot=slot, **kw)
    e.prefetch_end(slot)
    e.use_prefetched()
    return slot


@pytest.mark.parametrize('stem', ['1', '0'])
def test_engine_load_rois_jitter_on_inception_v3(monkeypatch, stem):
    """the u8-stem branch (IFCBK_STEM_U8 unset / 1) and the tensor branch (IFCBK_STEM_U8=0): squash, pad='border' and a batch with
    transpose codes, each on the current and on a prefetch slot, against the resize twins of the Pillow-enhanced ROIs; jitter=None is
    today's call"""
    monkeypatch.setenv('IFCBK_STEM_U8', stem)
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 4
    rois = [np.random.default_rng(41 + i).integers(0, 256, s, dtype=np.uint8) for i, s in enumerate(SHAPES4)]
    e = Engine(graph.build('inception_v3', 4), 0, max_batch=B)
    assert (e.stem_u8 is not None) == (stem == '1')

    def plane(slot):
        torch.cuda.synchronize()
        if stem == '1':
            assert e.in_kind[slot] == 'u8'
            return e.in_u8[slot][:B].clone().cpu().numpy()[..., None]
        assert e.in_kind[slot] == 'nhwc'
        return e.in_bufs[slot][:B].clone()

    def check(name, case, got, want_u8):
        if stem == '1':
            rb.check_u8(name, got, want_u8)
        else:
            tin = e.net.transform_input
            fcase = dict(case, dtype='bf16' if e.in_bufs[0].dtype == torch.bfloat16 else 'fp32', mean=(0, 0, 0), std=(1, 1, 1),
                         tsc=tuple(s / 0.5 for s in (0.229, 0.224, 0.225)) if tin else (1, 1, 1),
                         tsh=tuple((m - 0.5) / 0.5 for m in (0.485, 0.456, 0.406)) if tin else (0, 0, 0))
            rb.check_float(name, got.reshape(B, 299, 299, -1), want_u8, fcase)

    for pad, codes, turn, fb, fcn in ((None, [0, 1, 2, 3], False, FB4, FC4), ('border', [0, 1, 2, 3], False, FB4, FC4),
                                      (None, [4, 7, 2, 5], True, FB4, FC4), ('border', [4, 7, 2, 5], True, None, FC4), (None, None, False, FB4, None)):
        name = 'engine pad=%s codes=%s fb=%s fc=%s' % (pad, codes, fb is not None, fcn is not None)
        case = dict(fc._fcase('engine', SHAPES4, 299, 'border'), rois=SHAPES4, flips=codes or [0] * B)
        seen = [jc.pillow_jitter(r, None if fb is None else fb[i], None if fcn is None else fcn[i]) for i, r in enumerate(rois)]
        _check(name + ' twin', [jc.jitter(r, None if fb is None else fb[i], None if fcn is None else fcn[i]) for i, r in enumerate(rois)], seen)
        want = fc.expected_u8(dict(case, fill=pad), seen) if pad else tc.expected_u8(case, seen)

        def dev():                                        # a fresh upload per call: load_rois overwrites pixels
            more = dict(jitter=(_f32(fb), _f32(fcn)))
            if codes:
                more['flips'] = torch.tensor(codes, dtype=torch.uint8).cuda()
            if turn:
                more['turn'] = True
            if pad:
                more['pad'] = pad
            return _kw(rois, **more)

        kw = dev()
        e.load_rois(**kw)
        cur = plane(e.in_slot)
        check(name, case, cur, want)
        blob = kw['pixels'].cpu().numpy()
        assert np.array_equal(blob, np.concatenate([s.reshape(-1) for s in seen]))          # documented: pixels holds the jittered ROIs
        slot = _prefetch(e, dev())
        pre = plane(slot)
        assert e.in_slot == slot
        assert np.array_equal(cur, pre) if stem == '1' else torch.equal(cur.view(torch.uint8), pre.view(torch.uint8))
    # jitter=None and (None, None): the call without the argument, pixels untouched
    planes = []
    for more in (dict(), dict(jitter=None), dict(jitter=(None, None))):
        kw = _kw(rois, **more)
        e.load_rois(**kw)
        planes.append(plane(e.in_slot))
        assert np.array_equal(kw['pixels'].cpu().numpy(), np.concatenate([r.reshape(-1) for r in rois]))
    for p in planes[1:]:
        assert np.array_equal(planes[0], p) if stem == '1' else torch.equal(planes[0].view(torch.uint8), p.view(torch.uint8))
    with pytest.raises(ValueError):
        e.load_rois(**_kw(rois, jitter=(torch.ones(B, dtype=torch.float64).cuda(), None)))
    with pytest.raises(ValueError):
        e.load_rois(**_kw(rois, jitter=(torch.ones(B + 1).cuda(), None)))
    del e


def test_fit_batch_with_factors_equals_the_step_on_host_jittered_rois():
    """one fused training step of resnet18, batch 8, through collate_rois / rois_to_device / fit_batch: items that carry factors against
    the same step on the Pillow-enhanced ROIs without any -- bitwise in loss and updated weights"""
    import argparse
    from ifcb_classifier_amd.neuston_data import RoiTransform, collate_rois, rois_to_device
    from ifcb_classifier_amd.neuston_models import NeustonModel
    B = 8
    shapes = [(57, 131), (203, 88), (224, 1), (30, 30), (1, 224), (120, 224), (99, 45), (224, 173)]
    rois = [np.random.default_rng(61 + i).integers(0, 256, s, dtype=np.uint8) for i, s in enumerate(shapes)]
    fb = [0.5, 1.5, 1.0, 0.8, 1.2, 0.0, 2.0, 1.1]
    fcn = [1.5, 0.5, 0.9, 1.0, 0.0, 1.3, 0.7, 2.0]
    codes = [0, 1, 2, 3, 0, 1, 2, 3]
    y = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2])
    hp = argparse.Namespace(MODEL='resnet18', classes=list('abcde'), pretrained=False, batch_size=B)
    torch.manual_seed(3)
    m = NeustonModel(hp)
    eng = m.model.engine
    tf = RoiTransform(224, ((0.5, 0.4, 0.3), (0.2, 0.25, 0.3)), True, True, jitter=[1.0, 1.0])
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    res = []
    for dev_side in (True, False):
        m.load_state_dict(sd0)
        eng.nbt.zero_(); eng.M.zero_(); eng.V.zero_(); eng.step_count = 0
        p0 = eng.P.clone()
        if dev_side:
            batch, tgt = collate_rois([((r, c, False, b, k), int(t)) for r, c, b, k, t in zip(rois, codes, fb, fcn, y)])
        else:
            batch, tgt = collate_rois([((jc.pillow_jitter(r, b, k), c), int(t)) for r, c, b, k, t in zip(rois, codes, fb, fcn, y)])
        kw = rois_to_device(batch, eng.dev, tf)
        assert ('jitter' in kw) is dev_side
        m.fit_batch(kw, tgt.cuda())
        torch.cuda.synchronize()
        res.append((eng.loss.clone(), eng.P.clone()))
    assert bool(torch.isfinite(res[0][0]).all()) and not torch.equal(res[0][1], p0)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
