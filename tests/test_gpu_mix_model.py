"""TRAIN --mixup / --cutmix on the GPU, whole models: Engine.mix_batch on the slot a batch of grey ROIs was resized into (the u8 plane
where the engine has the u8 stem, the dense tensor elsewhere), the fused step's loss and head gradients against the two-target
reference, lam = 1 against an engine without mix, the prefetch slot against the direct form, and a captured step that sees new factors."""
import argparse

import numpy as np
import pytest
import torch

import loss_bounds as lb
import mix_cases as mc

pytestmark = pytest.mark.gpu
W7 = [0.02, 0.3, 1.0, 2.5, 7.0, 30.0, 90.0]
EPS = 0.1


def _hp(model, B, **kw):
    hp = dict(MODEL=model, classes=list('abcdefg'), pretrained=False, batch_size=B, precision='fp32', model_id='mx', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _batch(B, seed):
    """a collated batch of grey ROIs of mixed sizes and its targets"""
    from ifcb_classifier_amd.neuston_data import collate_rois
    rng = np.random.default_rng(seed)
    items = []
    for i in range(B):
        h, w = rng.integers(20, 90, 2)
        items.append(((rng.integers(0, 256, (h, w)).astype(np.uint8), 0), int(rng.integers(0, 7)), 'roi%d' % i))
    rois, targets, _ = collate_rois(items)
    return rois, targets


def _model(model, B, **kw):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp(model, B, **kw))
    if model == 'inception_v3':
        m.model.set_dropout_mask((torch.rand(B, 2048, generator=torch.Generator().manual_seed(5)) > 0.5).cuda())
    return m


def _slot_input(eng, n, slot=None):
    s = eng.in_slot if slot is None else slot
    return (eng.in_u8[s] if eng.in_kind[s] == 'u8' else eng.in_bufs[s])[:n].clone().cpu()


def _want(heads, n, t, lam, cw):
    main, aux = heads[0], (heads[1] if len(heads) > 1 else None)
    wm = mc.xent_mix(main.logits[:n].cpu(), t, lam, cw, 1.0, EPS)
    out = {'main': wm, 'loss': wm}
    if aux is not None:
        wa = mc.xent_mix(aux.logits[:n].cpu(), t, lam, cw, 0.4, EPS, old_loss=float(wm['loss'][0]))
        out['aux'], out['loss'] = wa, lb.head_sum(wm, wa)
    return out


def _check_step(tag, eng, heads, n, t, lam, cw):
    torch.cuda.synchronize()
    want = _want(heads, n, t, lam, cw)
    r = mc.check('%s eng.loss' % tag, {'loss': eng.loss.clone()}, want['loss'], family='mix model loss')
    r = max(r, mc.check('%s main dlogits' % tag, {'dlogits': heads[0].dlogits[:n]}, want['main'], family='mix model dlogits'))
    if len(heads) > 1:
        r = max(r, mc.check('%s aux dlogits' % tag, {'dlogits': heads[1].dlogits[:n]}, want['aux'], family='mix model dlogits'))
    return r


@pytest.mark.parametrize('B', [5, 4])
@pytest.mark.parametrize('model', ['inception_v3', 'resnet18'])
def test_mix_batch_and_the_step_after_it(model, B):
    from ifcb_classifier_amd.neuston_data import rois_to_device
    m = _model(model, B, mixup=0.4, cutmix=1.0, label_smoothing=EPS, class_weights=W7)
    eng, heads = m.model.engine, m.model._train_heads
    assert eng.mix and len(eng.mix_lam) == 2
    S = eng.net.S
    rois, t = _batch(B, 1)
    n = eng.load_rois(**rois_to_device(rois, eng.dev, None))
    assert n == B and eng.in_kind[eng.in_slot] == ('u8' if model == 'inception_v3' else 'nhwc')     # the u8 stem path where there is one
    eng.target[:n].copy_(t)
    before = _slot_input(eng, n)
    lam = torch.tensor([0.3183, 1.0, 0.0, 0.7071, 0.8413][:B])          # (no short fractions: few bytes near a rounding tie)
    box = (S // 4, S // 2 + 3, 0, S // 3)
    eng.mix_batch(n, lam.cuda(), box)
    torch.cuda.synchronize()
    after = _slot_input(eng, n)
    assert torch.equal(eng.mix_lam[eng.in_slot][:n].cpu(), lam)
    if before.dtype == torch.uint8:
        exact, copy, _ = mc.mix_reference(before, lam, box)
        wrong, share = mc.u8_verdict(after, exact)
        assert not bool(wrong.any()) and share <= mc.AMBIG_MAX and torch.equal(after.double()[copy], exact[copy])
    else:
        mc.check_mix_dense('%s mix_batch' % model, after, before, lam, box, 'f32')
    assert not torch.equal(after, before)
    m.model.train()
    eng.train_step(n)
    r = _check_step(model, eng, heads, n, t, lam, eng.class_weight.cpu())
    # a python float fills every entry; no box
    eng.load_rois(**rois_to_device(rois, eng.dev, None))
    eng.mix_batch(n, 0.25)
    eng.train_step(n)
    r = max(r, _check_step(model + ' float', eng, heads, n, t, torch.full((n,), 0.25), eng.class_weight.cpu()))
    print('%s batch %d: worst err/bound %.3f' % (model, B, r))
    # validation stays the one-target loss of the configured kind
    import loss_smooth_bounds as sb
    eng.load_rois(**rois_to_device(rois, eng.dev, None))
    probs, vloss = m.eval_current(n, with_loss=True)
    torch.cuda.synchronize()
    sb.check('%s val_loss' % model, {'loss': vloss.reshape(1)}, sb.xent_ls(heads[0].logits[:n].cpu(), t, eng.class_weight.cpu(), 1.0, EPS))


@pytest.mark.parametrize('model', ['inception_v3', 'resnet18'])
def test_lam_1_without_a_box_is_the_forward_of_an_engine_without_mix(model):
    from ifcb_classifier_amd.neuston_data import rois_to_device
    B = 4
    rois, t = _batch(B, 2)
    logits = []
    for mix in (True, False):
        m = _model(model, B, **(dict(mixup=0.4) if mix else {}))
        eng = m.model.engine
        assert eng.mix == mix
        n = eng.load_rois(**rois_to_device(rois, eng.dev, None))
        eng.target[:n].copy_(t)
        if mix:
            eng.mix_batch(n, 1.0)
        m.model.train()
        eng.forward_train(n)
        torch.cuda.synchronize()
        logits.append([h.logits[:n].clone() for h in m.model._train_heads])
    for a, b in zip(*logits):
        assert torch.equal(a, b)


class _Draw:
    """a BatchMix stand-in that repeats one draw"""

    def __init__(self, lam, box):
        self.lam, self.box = lam, box

    def draw(self, S):
        return self.lam, self.box


def test_prefetch_slot_gives_the_loss_of_the_direct_form():
    from ifcb_classifier_amd.neuston_data import RoiTransform, rois_to_device
    B = 5
    rois, t = _batch(B, 3)
    draw = _Draw(0.35, (10, 100, 50, 224))
    losses, inputs = [], []
    for staged in (False, True):
        m = _model('resnet18', B, cutmix=1.0, label_smoothing=EPS)
        eng = m.model.engine
        if staged:
            tf = RoiTransform(224, mix=draw)
            n = m.stage_batch(rois, tf, t)
            m.use_staged()
            assert eng.in_slot == 1
            inputs.append(_slot_input(eng, n))
            m.fit_current(n)
        else:
            m.batch_mix = draw
            m.fit_batch(rois_to_device(rois, eng.dev, None), t.cuda())
            inputs.append(_slot_input(eng, B))
        torch.cuda.synchronize()
        losses.append(eng.loss.clone())
        mc.check('staged %d' % staged, {'loss': eng.loss.clone()},
                 mc.xent_mix(m.model._train_heads[0].logits[:B].cpu(), t, torch.full((B,), 0.35), None, 1.0, EPS), family='mix model loss')
    assert torch.equal(inputs[0], inputs[1]) and torch.equal(losses[0], losses[1])


def test_a_captured_step_sees_new_factors_without_a_new_capture():
    from ifcb_classifier_amd.neuston_data import rois_to_device
    B = 4
    m = _model('resnet18', B, mixup=0.4, label_smoothing=EPS)
    eng, heads = m.model.engine, m.model._train_heads
    eng.graph_train = True
    rois, t = _batch(B, 4)
    m.model.train()
    handles = []
    for lam in (0.2, 0.9):
        n = eng.load_rois(**rois_to_device(rois, eng.dev, None))
        eng.target[:n].copy_(t)
        eng.mix_batch(n, lam)
        pl = eng.train_step(n)
        _check_step('graph lam %g' % lam, eng, heads, n, t, torch.full((n,), lam), None)
        assert 'fwd_bwd' in pl.graphs
        handles.append(pl.graphs['fwd_bwd'])
    assert handles[0] is handles[1]                                # one capture, replayed
