"""TRAIN --rot90 on the GPU: every path of the quarter-turn kernels (csrc/roi_turn.hip, ifcbk_roi_preprocess with
flip_bits_valid == 2) bit for bit against the Pillow-equal oracle's resize of the numpy-turned ROI, the float stage per element
against float64 (tests/roi_turn_cases.py: the case table and the path predicates; tests/test_roi_turn_cpu.py proves on the CPU that
the oracle equals the installed Pillow on every turned shape), the ABI's promises about flip_bits_valid 0 / 1 / 2, and the flag
through Engine.load_rois and NeustonModel.fit_batch.

Each run allocates out, out_u8 and the pixel blob between poisoned margins: the margins must come back untouched."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import roi_bounds as rb
import roi_turn_cases as tc

pytestmark = pytest.mark.gpu
MARGIN = 4096           # bytes on both sides (a multiple of 16: the float stores are 16-byte vectors)


def _guarded(nbytes, poison):
    buf = torch.full((MARGIN + nbytes + MARGIN,), poison, dtype=torch.uint8, device='cuda')
    return buf, buf[MARGIN:MARGIN + nbytes]


def _margins_intact(name, buf, nbytes, poison):
    b = buf.cpu()
    assert bool((b[:MARGIN] == poison).all()), '%s: bytes in front of the buffer were written' % name
    assert bool((b[MARGIN + nbytes:] == poison).all()), '%s: bytes behind the buffer were written' % name


def run(ctx, case, rois, valid=2, codes=None, poison=0xA5, layout='packed', maxima=None):
    """-> (out [n][S][S][cout] or None, u8 [n][S][S][cin] numpy or None); the blob lies between poisoned margins too"""
    from ifcb_classifier_amd import _lib
    n, S, cin, cout = len(rois), case['S'], case['cin'], case['cout']
    codes = case['flips'] if codes is None else codes
    hs = torch.tensor([r.shape[0] for r in rois], dtype=torch.int32)
    ws = torch.tensor([r.shape[1] for r in rois], dtype=torch.int32)
    sizes = [int(r.size) for r in rois]
    order = list(range(n)) if layout == 'packed' else list(range(n - 1, -1, -1))      # 'reverse': last ROI first, 7 poison bytes between
    gap = 0 if layout == 'packed' else 7
    offs = [0] * n
    pos = MARGIN + gap
    for i in order:
        offs[i] = pos
        pos += sizes[i] + gap
    blob = np.full(pos + MARGIN, poison, np.uint8)                                     # poison in front of the first and behind the last ROI
    for i in order:
        blob[offs[i]:offs[i] + sizes[i]] = rois[i].reshape(-1)
    pix = torch.from_numpy(blob).cuda()
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels = n, S, cin, cout
    d.dtype = _lib.BF16 if case['dtype'] == 'bf16' else _lib.F32
    d.flip_bits_valid = valid
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = case['mean'][k], case['std'][k], case['tsc'][k], case['tsh'][k]
    mh, mw = maxima or rb.maxima(case)                                                 # the SOURCE dims, turned or not
    kmax = rb.kmax_for(mh, mw, S)
    need = ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), mh, mw)
    assert need == n * 2 * S * (2 + kmax) * 4
    ctx.reserve(need)
    esz = 2 if case['dtype'] == 'bf16' else 4
    tdt = torch.bfloat16 if case['dtype'] == 'bf16' else torch.float32
    ob_, ov = _guarded(n * S * S * cout * esz, poison) if case['out'] else (None, None)
    ub_, uv = _guarded(n * S * S * cin, poison) if case['u8'] else (None, None)
    fl = torch.tensor(codes, dtype=torch.uint8).cuda()
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
    assert np.array_equal(pix.cpu().numpy(), blob), case['name'] + ': the blob was written'
    return out, u8


@pytest.mark.parametrize('case', tc.TURN, ids=[c['name'] for c in tc.TURN])
def test_turned_roi_paths_u8_bit_exact_and_float_stage_bounded(ctx, case):
    rois = rb.pixels(case)
    want = tc.expected_u8(case, rois)
    out, u8 = run(ctx, case, rois)
    if case['u8']:
        rb.check_u8(case['name'], u8, want)
    if case['out']:
        rb.check_float(case['name'], out, want, case)
    # another poison value and the reversed, gapped blob layout: the same bytes out
    out2, u82 = run(ctx, case, rois, poison=0x3C, layout='reverse')
    if case['u8']:
        assert np.array_equal(u8, u82), case['name']
    if case['out']:
        assert torch.equal(out.view(torch.uint8), out2.view(torch.uint8)), case['name']


OLD = ('small299 norm', 'mid299', 'big224 kmax7')           # roi_bounds.ROI cases with flip codes 0..3: one per kmax class


def test_codes_below_four_give_the_same_bytes_under_flip_bits_valid_1_and_2(ctx):
    by = {c['name']: c for c in rb.ROI}
    assert [rb.kmax(by[n]) for n in OLD] == [3, 5, 7]
    for name in OLD:
        case = by[name]
        assert set(case['flips']) == {0, 1, 2, 3}
        rois = rb.pixels(case)
        o1, u1 = run(ctx, case, rois, valid=1)
        o2, u2 = run(ctx, case, rois, valid=2)
        rb.check_u8(name, u1, rb.expected_u8(case, rois))
        assert np.array_equal(u1, u2), name
        assert torch.equal(o1.view(torch.uint8), o2.view(torch.uint8)), name


def test_bit_2_is_ignored_under_flip_bits_valid_0_and_1(ctx):
    by = {c['name']: c for c in rb.ROI}
    for name in OLD:
        case = by[name]
        rois = rb.pixels(case)
        high = [f | 4 for f in case['flips']]
        o1, u1 = run(ctx, case, rois, valid=1)
        o2, u2 = run(ctx, case, rois, valid=1, codes=high)
        assert np.array_equal(u1, u2) and torch.equal(o1.view(torch.uint8), o2.view(torch.uint8)), name
        o0, u0 = run(ctx, case, rois, valid=0, codes=high)
        rb.check_u8(name + ' no codes', u0, rb.expected_u8(dict(case, flips=None), rois))


def test_understated_maxima_stay_in_bounds(ctx):
    """a kmax == 3 batch (maxima 224 x 224 handed over) holding ROIs larger than S, turned and not: their planes are unspecified,
    the margins of out, out_u8 and the blob stay intact and every other ROI's plane is right.  (roi_turn_resize3_kernel clamps the
    band rows to the staged ones and the columns to the staged width; the coefficient kernel clamps the tap count to kmax.)"""
    shapes = [(40, 60), (300, 250), (224, 224), (250, 330), (330, 20), (17, 5), (5, 400), (100, 100)]
    codes = [5, 4, 6, 7, 5, 2, 4, 1]
    case = rb._case('understated', shapes, 224, flips=codes, mean=tc.MEAN, std=tc.STD)
    assert set(tc.paths(dict(case, maxima=(224, 224)))) == {'roi_turn_resize3_kernel'}
    rois = rb.pixels(case)
    for cds in (codes, [c ^ 4 for c in codes]):
        out, u8 = run(ctx, case, rois, codes=cds, maxima=(224, 224))
        want = tc.expected_u8(case, rois, cds)
        ok = [i for i, (h, w) in enumerate(shapes) if h <= 224 and w <= 224]
        assert len(ok) == 4
        rb.check_u8('understated, ROIs within the maxima', u8[ok], want[ok])


def _batch(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]


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


SHAPES8 = [(57, 131), (203, 88), (224, 1), (30, 30), (1, 224), (120, 224), (99, 45), (224, 173)]


def _prefetch(e, kw):
    slot, side = e.prefetch_begin()
    with torch.cuda.stream(side):
        e.load_rois(slot=slot, **kw)
    e.prefetch_end(slot)
    e.use_prefetched()
    return slot


def test_engine_load_rois_with_codes_equals_host_turned_rois_bitwise():
    """resnet18 at 224, batch 8, eval: codes 0..7 with turn=True against the numpy-turned ROIs without codes, on the current slot
    and on a prefetch slot"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 8
    rois = _batch(SHAPES8, 21)
    codes = list(range(8))
    norm = dict(mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))
    host = _kw([tc.seen(r, c) for r, c in zip(rois, codes)], **norm)
    dev = _kw(rois, flips=torch.tensor(codes, dtype=torch.uint8).cuda(), turn=True, **norm)
    e = Engine(graph.build('resnet18', 5), 0, max_batch=B)
    e.init_weights(seed=4)

    def logits():
        e.forward_eval(B)
        torch.cuda.synchronize()
        return [h.logits[:B].clone() for h in e.heads], e.act[e.net.input.id][:B].clone()

    e.load_rois(**host)
    want, x_want = logits()
    assert x_want.float().abs().sum().item() > 0 and all(bool(torch.isfinite(w).all()) for w in want)
    e.load_rois(**dev)
    got, x_got = logits()
    assert torch.equal(x_got.view(torch.uint8), x_want.view(torch.uint8))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # without the flag the same codes are flips only: another input
    e.load_rois(**dict(dev, turn=False))
    assert not torch.equal(e.act[e.net.input.id][:B].view(torch.uint8), x_want.view(torch.uint8))
    slot = _prefetch(e, dev)
    got, x_got = logits()
    assert e.in_slot == slot and torch.equal(x_got.view(torch.uint8), x_want.view(torch.uint8))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    del e


def test_engine_u8_stem_slot_receives_the_turned_plane():
    """inception_v3's grey input path (only the u8 plane is written): in_u8 of the current and of a prefetch slot equals the plane of
    the host-turned ROIs.  No forward."""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 4
    rois = _batch([(57, 131), (299, 88), (30, 299), (120, 45)], 22)
    codes = [4, 7, 2, 5]
    e = Engine(graph.build('inception_v3', 4), 0, max_batch=B)
    assert e.stem_u8 is not None
    e.load_rois(**_kw([tc.seen(r, c) for r, c in zip(rois, codes)]))
    torch.cuda.synchronize()
    assert e.in_kind[e.in_slot] == 'u8'
    want = e.in_u8[e.in_slot][:B].clone()
    case = rb._case('u8 stem', [r.shape for r in rois], 299, flips=codes)
    rb.check_u8('u8 stem plane', want.cpu().numpy()[..., None], tc.expected_u8(case, rois))
    dev = _kw(rois, flips=torch.tensor(codes, dtype=torch.uint8).cuda(), turn=True)
    e.in_u8[e.in_slot].zero_()
    e.load_rois(**dev)
    torch.cuda.synchronize()
    assert e.in_kind[e.in_slot] == 'u8' and torch.equal(e.in_u8[e.in_slot][:B], want)
    slot = _prefetch(e, dev)
    torch.cuda.synchronize()
    assert e.in_slot == slot and e.in_kind[slot] == 'u8' and torch.equal(e.in_u8[slot][:B], want)
    del e


def test_fit_batch_under_a_rot90_transform_equals_the_step_on_host_turned_rois():
    """one fused training step of resnet18, batch 8: collate_rois / rois_to_device under RoiTransform(rot90=True) against the same
    step on the numpy-turned ROIs without codes -- bitwise in loss and updated weights"""
    from ifcb_classifier_amd.neuston_data import RoiTransform, collate_rois, rois_to_device
    from ifcb_classifier_amd.neuston_models import NeustonModel
    B, nc = 8, 5
    hp = argparse.Namespace(MODEL='resnet18', classes=list('abcde'), pretrained=False, batch_size=B)
    torch.manual_seed(3)
    m = NeustonModel(hp)
    eng = m.model.engine
    tf = RoiTransform(224, ((0.5, 0.4, 0.3), (0.2, 0.25, 0.3)), rot90=True)
    rois = _batch(SHAPES8, 23)
    codes = [7, 6, 5, 4, 3, 2, 1, 0]
    y = torch.tensor([0, 1, 2, 3, 4, 0, 1, 2])
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    res = []
    for turned in (True, False):
        m.load_state_dict(sd0)
        eng.nbt.zero_(); eng.M.zero_(); eng.V.zero_(); eng.step_count = 0
        p0 = eng.P.clone()
        if turned:
            batch, tgt = collate_rois([((r, c, True), int(t)) for r, c, t in zip(rois, codes, y)])
            assert batch['turn'] is True
        else:
            batch, tgt = collate_rois([((tc.seen(r, c), 0), int(t)) for r, c, t in zip(rois, codes, y)])
        kw = rois_to_device(batch, eng.dev, tf if turned else RoiTransform(224, tf.img_norm))
        assert kw.get('turn', False) is turned and ('flips' in kw) is turned
        m.fit_batch(kw, tgt.cuda())
        torch.cuda.synchronize()
        res.append((eng.loss.clone(), eng.P.clone()))
    assert bool(torch.isfinite(res[0][0]).all()) and not torch.equal(res[0][1], p0)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])

