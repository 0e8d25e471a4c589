"""TRAIN --blur on the GPU, whole models: Engine.load_rois(blur=sigmas) against load_rois() followed by the float64 twin of
tests/blur_cases.py on both input kinds (the u8 plane of an engine with the u8 stem, the dense tensor elsewhere), the train step behind
a blurred load in the plain and the graph launch mode, the resident cut against the upload for the same draws, and the pass in one load
with flips, quarter turns, pad, jitter and batch mixing (ifcbk_batch_blur behind the resize, ahead of ifcbk_batch_mix)."""
import argparse
import random

import numpy as np
import pytest
import torch

import blur_cases as bc
import resident_cases as rc

pytestmark = pytest.mark.gpu
SIGMA_MAX, R = 1.0, 3                                               # --blur 1: radius ceil(3 * 1)


def _hp(model, B, **kw):
    hp = dict(MODEL=model, classes=['ant', 'bee', 'cat'], pretrained=False, batch_size=B, precision='fp32', model_id='bl', resize=224,
              img_norm=None, seed=3, blur=SIGMA_MAX, blur_prob=0.5)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _model(model, B, seed=11, **kw):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(seed)
    m = NeustonModel(_hp(model, B, **kw), max_batch=B)
    if model == 'inception_v3':
        m.model.set_dropout_mask((torch.rand(B, 2048, generator=torch.Generator().manual_seed(5)) > 0.5).cuda())
    return m


def _batch(B, seed, extra=()):
    """a collated batch of grey ROIs of mixed sizes with levels 0..63 (the near-tie cap of blur_cases: the bound grows with the level)"""
    from ifcb_classifier_amd.neuston_data import collate_rois
    rng = np.random.default_rng(seed)
    items = []
    for i in range(B):
        h, w = rng.integers(20, 90, 2)
        items.append(((rng.integers(0, 64, (h, w)).astype(np.uint8), 0) + tuple(extra), int(rng.integers(0, 3)), 'roi%d' % i))
    rois, targets, _ = collate_rois(items)
    return rois, targets


def _slot_input(eng, n, slot=None):
    s = eng.in_slot if slot is None else slot
    return (eng.in_u8[s] if eng.in_kind[s] == 'u8' else eng.in_bufs[s])[:n].clone().cpu()


def _hold(tag, after, before, sigmas):
    """``after`` = the slot behind load_rois(blur=sigmas), ``before`` = behind load_rois(): after must be the twin of before"""
    for n, s in enumerate(sigmas):
        s = float(s)
        if s == 0.0:
            assert torch.equal(after[n].view(torch.uint8), before[n].view(torch.uint8)), '%s: image %d (sigma 0) changed' % (tag, n)
        elif before.dtype == torch.uint8:
            x = before[n].numpy()
            ref, bound = bc.twin(x, s, R), bc.fp32_bound(s, R, float(x.max()))
            wrong, share = bc.u8_verdict(after[n].numpy(), ref, bound)
            print('%s image %d sigma %g: near-tie share %.5f, %d wrong' % (tag, n, s, share, int(wrong.sum())))
            assert share <= bc.TIE_CAP and not wrong.any(), (tag, n, share, int(wrong.sum()))
        else:
            form = 'bf16' if before.dtype == torch.bfloat16 else 'f32'
            x, g = before[n].double().numpy(), after[n].double().numpy()
            for c in range(3):
                ref = bc.twin(x[..., c], s, R)
                bound = bc.stored_bound(form, s, R, float(np.abs(x[..., c]).max()), ref)
                ratio = float((np.abs(g[..., c] - ref) / bound).max())
                print('%s image %d channel %d sigma %g: err / bound %.3f' % (tag, n, c, s, ratio))
                assert ratio <= 1.0, (tag, n, c, ratio)
            assert torch.equal(after[n][..., 3:].contiguous().view(torch.uint8), before[n][..., 3:].contiguous().view(torch.uint8))
            assert not torch.equal(after[n][..., :3], before[n][..., :3])


@pytest.mark.parametrize('model,precision', [('inception_v3', 'bf16'), ('resnet18', 'fp32'), ('resnet18', 'bf16')])
def test_load_rois_with_sigmas_is_the_twin_of_the_plain_load(model, precision):
    from ifcb_classifier_amd.neuston_data import rois_to_device
    B = 3
    m = _model(model, B, precision=precision)
    eng = m.model.engine
    assert eng.blur_radius == R
    rois, _ = _batch(B, 1)
    sig = torch.tensor([0.7071, 0.0, 1.0])
    n = eng.load_rois(**rois_to_device(rois, eng.dev, None))
    assert n == B and eng.in_kind[eng.in_slot] == ('u8' if model == 'inception_v3' else 'nhwc')
    before = _slot_input(eng, n)
    assert eng.load_rois(blur=sig.cuda(), **rois_to_device(rois, eng.dev, None)) == B
    torch.cuda.synchronize()
    _hold('%s %s' % (model, precision), _slot_input(eng, n), before, sig)
    # blur=None and no argument: the plain load's bytes
    eng.load_rois(blur=None, **rois_to_device(rois, eng.dev, None))
    assert torch.equal(_slot_input(eng, n).view(torch.uint8), before.view(torch.uint8))
    # the prefetch slot, through the batch's own 'blur' entry: the same bits as the direct form
    eng.load_rois(blur=sig.cuda(), **rois_to_device(rois, eng.dev, None))
    direct = _slot_input(eng, n)
    rois2 = dict(rois, blur=sig)
    n2 = m.stage_batch(rois2, None, None)
    m.use_staged()
    torch.cuda.synchronize()
    assert n2 == B and torch.equal(_slot_input(eng, n2).view(torch.uint8), direct.view(torch.uint8))
    with pytest.raises(ValueError, match='sigmas'):
        eng.load_rois(blur=sig[:2].cuda(), **rois_to_device(rois, eng.dev, None))


def test_an_engine_without_a_radius_refuses_sigmas():
    from ifcb_classifier_amd.neuston_data import rois_to_device
    m = _model('resnet18', 2, blur=None)
    eng = m.model.engine
    rois, _ = _batch(2, 2)
    with pytest.raises(RuntimeError, match='blur_radius'):
        eng.load_rois(blur=torch.ones(2).cuda(), **rois_to_device(rois, eng.dev, None))


def test_the_step_behind_a_blurred_load_has_the_same_bits_in_plain_and_graph_mode():
    from ifcb_classifier_amd.neuston_data import rois_to_device
    B = 4
    rois, t = _batch(B, 3)
    sig = torch.tensor([1.0, 0.3, 0.0, 0.55])
    out = []
    for graph in (False, True):
        m = _model('resnet18', B)
        eng = m.model.engine
        eng.graph_train = graph
        m.model.train()
        losses = []
        for _ in range(2):
            n = eng.load_rois(blur=sig.cuda(), **rois_to_device(rois, eng.dev, None))
            eng.target[:n].copy_(t)
            pl = eng.train_step(n)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert ('fwd_bwd' in pl.graphs) == graph
        out.append(dict(P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(), RB=eng.RB.clone(), loss=torch.stack(losses)))
    a, b = out
    assert bool(torch.isfinite(a['loss']).all())
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from ifcb_classifier_amd.neuston_data import NeustonDataset, ResidentSet
    ds = NeustonDataset(rc.write_tree(str(tmp_path_factory.mktemp('blur') / 'grey'), 'grey'))
    return ds, ResidentSet.build(ds)


def test_the_resident_cut_gives_the_bytes_of_the_upload_for_the_same_draws(tree):
    from ifcb_classifier_amd.neuston_data import RoiTransform, collate_rois
    ds, host = tree
    B = 8
    m = _model('resnet18', B)
    eng = m.model.engine
    res = host.to_device(eng.dev, eng.prefetch_stream())
    idx = [17, 3, 3, 22, 0, 9, 14, 6]
    got = []
    for resident in (False, True):
        tf = RoiTransform(224, None, True, True, jitter=[0.2, 0.3], blur=SIGMA_MAX, blur_prob=0.6, seed=3)
        ds.transforms = tf
        random.seed(4)
        if resident:
            idx_host = np.asarray(idx, np.int64)
            with torch.cuda.stream(res.stream):
                idx_dev = torch.from_numpy(idx_host).to(eng.dev)
            n = m.stage_resident_batch(res, idx_dev, idx_host, tf, train=True)
        else:
            rois, targets, _ = collate_rois([ds[i] for i in idx])
            assert 'blur' in rois and 0 < int((rois['blur'] > 0).sum()) < B
            n = m.stage_batch(rois, tf, targets, train=True)
        m.use_staged()
        torch.cuda.synchronize()
        got.append((n, _slot_input(eng, n), eng.target[:n].clone(), random.getstate(), tf._blur_rng.bit_generator.state))
    a, b = got
    assert a[0] == b[0] == B and torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8)) and torch.equal(a[2], b[2])
    assert a[3] == b[3] and a[4] == b[4]
    # and they are blurred: the same staging without the flag differs
    tf = RoiTransform(224, None, True, True, jitter=[0.2, 0.3])
    ds.transforms = tf
    random.seed(4)
    rois, targets, _ = collate_rois([ds[i] for i in idx])
    m.stage_batch(rois, tf, targets, train=True)
    m.use_staged()
    torch.cuda.synchronize()
    assert not torch.equal(_slot_input(eng, B), a[1])


class _Draw:
    """a BatchMix stand-in that repeats one draw"""

    def __init__(self, lam, box):
        self.lam, self.box = lam, box

    def draw(self, S):
        return self.lam, self.box


@pytest.mark.parametrize('model', ['inception_v3', 'resnet18'])
def test_the_pass_composes_with_flip_rot90_pad_jitter_and_mixup_in_one_load(model):
    """behind the resize (which holds flip, turn, pad and, ahead of it, jitter), ahead of the mix"""
    from ifcb_classifier_amd import _lib
    from ifcb_classifier_amd.neuston_data import RoiTransform, rois_to_device
    B = 4
    m = _model(model, B, mixup=0.4, pad='border')
    eng = m.model.engine
    S = eng.net.S
    rois, t = _batch(B, 5, extra=(True, 1.2, 0.8))                  # (turn, brightness, contrast) fields of the items
    rois['flips'] = torch.tensor([5, 2, 7, 0], dtype=torch.uint8)   # flips and transposes
    sig = torch.tensor([0.9, 0.0, 0.4142, 1.0])
    tf = RoiTransform(S, None, True, True, rot90=True, pad='border', jitter=[0.2, 0.2], blur=SIGMA_MAX, mix=_Draw(0.35, (10, 100, 50, S)))
    # the plain load of the same batch (jitter maps the uploaded blob in place: a fresh upload per load)
    kw = rois_to_device(rois, eng.dev, tf)
    assert kw['turn'] and kw['pad'] == 'border' and kw['jitter'][0] is not None and 'blur' not in kw
    n = eng.load_rois(**kw)
    plain = _slot_input(eng, n)
    # one load with everything, then the mix
    kw = rois_to_device(dict(rois, blur=sig), eng.dev, tf)
    assert torch.equal(kw['blur'].cpu(), sig)
    n = eng.load_rois(**kw)
    torch.cuda.synchronize()
    blurred = _slot_input(eng, n)
    _hold('%s composed' % model, blurred, plain, sig)
    eng.mix_batch(n, 0.35, (10, 100, 50, S))
    torch.cuda.synchronize()
    want = _slot_input(eng, n)
    # the staged form of the same batch: resize, blur, mix on the prefetch stream -- the same bytes
    n2 = m.stage_batch(dict(rois, blur=sig), tf, t, train=True)
    m.use_staged()
    torch.cuda.synchronize()
    assert n2 == B and torch.equal(_slot_input(eng, n2).view(torch.uint8), want.view(torch.uint8))
    # and a direct call of the entry point on the plain load is the pass load_rois makes
    kw = rois_to_device(rois, eng.dev, tf)
    eng.load_rois(**kw)
    s = eng.in_slot
    buf, kind = (eng.in_u8[s], _lib.MIX_U8) if eng.in_kind[s] == 'u8' else (eng.in_bufs[s], eng.cdtype)
    sg = sig.cuda()
    eng.ctx.call('ifcbk_batch_blur', _lib.ptr(buf), kind, n, S, _lib.ptr(sg), R, eng.stream())
    torch.cuda.synchronize()
    assert torch.equal(_slot_input(eng, n).view(torch.uint8), blurred.view(torch.uint8))
    m.fit_current(n)                                                # the step runs on it
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.loss).all())
