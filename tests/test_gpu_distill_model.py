"""TRAIN --distill on the GPU, whole models: the fused step of an engine built with distill against a direct call of the loss kernel
(plain launches and the captured graph), and a teacher / student pair of NeustonModels through stage_batch / use_staged / fit_current
and through fit_batch: the teacher buffer the student's loss read, and the blob jittered once."""
import argparse
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, NC = 8, 5


def _hp(**kw):
    hp = dict(MODEL='resnet18', classes=list('abcde'), pretrained=False, batch_size=B, precision='fp32', model_id='st', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _model(seed=11, **kw):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(seed)
    return NeustonModel(_hp(**kw), max_batch=B)


def _batch(seed, jitter=False):
    """a collated batch of grey ROIs of mixed sizes with flip codes (and jitter factors), and its targets"""
    from ifcb_classifier_amd.neuston_data import collate_rois
    rng = np.random.default_rng(seed)
    items = []
    for i in range(B):
        h, w = rng.integers(20, 90, 2)
        aug = (rng.integers(0, 256, (h, w)).astype(np.uint8), int(rng.integers(0, 4)))
        if jitter:
            aug = aug + (0, float(rng.uniform(0.6, 1.4)), float(rng.uniform(0.6, 1.4)))
        items.append((aug, int(rng.integers(0, NC)), 'roi%d' % i))
    rois, targets, _ = collate_rois(items)
    return rois, targets


def _direct(eng, head, n, weight, acc_from=None):
    """ifcbk_softmax_xent_distill on the step's own logits, targets and teacher buffer -> (loss, dlogits)"""
    from ifcb_classifier_amd import _lib
    loss = torch.zeros(1, device='cuda') if acc_from is None else acc_from.clone()
    dl = torch.zeros(n, NC, device='cuda')
    cw = eng.class_weight
    eng.ctx.call('ifcbk_softmax_xent_distill', _lib.ptr(head.logits), _lib.ptr(eng.target), _lib.ptr(eng.teacher_logits), _lib.ptr(cw), n, NC,
                 weight, eng.label_smoothing, eng.distill[0], eng.distill[1], _lib.ptr(loss), 0 if acc_from is None else 1, _lib.ptr(dl),
                 _lib.cur_stream())
    torch.cuda.synchronize()
    return loss, dl


@pytest.mark.parametrize('graph', [False, True], ids=['launches', 'graph'])
@pytest.mark.parametrize('kw', [dict(), dict(label_smoothing=0.1, class_weights=[0.5, 1.0, 2.0, 1.0, 3.0])], ids=['plain', 'cw_ls'])
def test_the_fused_step_leaves_the_loss_of_a_direct_call(kw, graph):
    from ifcb_classifier_amd.neuston_data import rois_to_device
    m = _model(distill='teacher.ptl', distill_alpha=0.3, distill_temperature=4, **kw)
    eng, head = m.model.engine, m.model._train_heads[0]
    assert eng.distill == (0.3, 4.0) and tuple(eng.teacher_logits.shape) == (B, NC)
    eng.graph_train = graph
    rois, t = _batch(1)
    m.model.train()
    for step in range(2):                                   # (graph: the second step replays the capture, with new teacher logits)
        eng.teacher_logits.copy_(torch.randn(B, NC, generator=torch.Generator().manual_seed(40 + step)) * 3)
        n = eng.load_rois(**rois_to_device(rois, eng.dev, None))
        eng.target[:n].copy_(t)
        pl = eng.train_step(n)
        torch.cuda.synchronize()
        assert graph == ('fwd_bwd' in pl.graphs)
        loss, dl = _direct(eng, head, n, 1.0)
        assert bool(torch.isfinite(loss).all()) and torch.equal(eng.loss, loss)
        assert torch.equal(head.dlogits[:n], dl)
    # the validation loss stays the hard loss of the configured kind
    import loss_smooth_bounds as sb
    eng.load_rois(**rois_to_device(rois, eng.dev, None))
    probs, vloss = m.eval_current(n, with_loss=True)
    torch.cuda.synchronize()
    cw = None if eng.class_weight is None else eng.class_weight.cpu()
    sb.check('val_loss', {'loss': vloss.reshape(1)}, sb.xent_ls(head.logits[:n].cpu(), t, cw, 1.0, eng.label_smoothing))


def test_a_model_that_distils_refuses_to_train_without_its_teacher():
    from ifcb_classifier_amd.neuston_data import rois_to_device
    m = _model(distill='teacher.ptl')
    rois, t = _batch(2)
    with pytest.raises(RuntimeError, match='no teacher is attached'):
        m.fit_batch(rois_to_device(rois, m.model.engine.dev, None), t.cuda())


def _jitter_once(eng, rois):
    """the blob after ONE ifcbk_roi_jitter call, into a second buffer"""
    from ifcb_classifier_amd import _lib
    dev = eng.dev
    px = rois['pixels'].to(dev)
    out = torch.empty_like(px)
    offs, hs, ws = rois['offs'].to(dev), rois['hs'].to(dev), rois['ws'].to(dev)
    fb, fc = rois['brightness'].to(dev), rois['contrast'].to(dev)
    assert eng.ctx.lib.ifcbk_roi_jitter_workspace(B) <= eng.ctx.lib.ifcbk_ctx_workspace_bytes(eng.ctx.h)
    eng.ctx.call('ifcbk_roi_jitter', _lib.ptr(px), _lib.ptr(offs), _lib.ptr(hs), _lib.ptr(ws), B, 1, rois['max_h'], rois['max_w'],
                 _lib.ptr(fb), _lib.ptr(fc), _lib.ptr(out), _lib.cur_stream())
    torch.cuda.synchronize()
    return px, out


@pytest.mark.parametrize('staged', [True, False], ids=['staged', 'fit_batch'])
def test_teacher_and_student_see_one_batch(staged):
    """Same-size models: every backbone of the model table has one input side (224 but for inception_v3's 299, which is too slow here),
    so the pair is two resnet18s whose ROI paths differ in what the teacher's file sets instead: its img_norm and its pad."""
    from ifcb_classifier_amd import neuston_data as nd
    teacher = _model(seed=5, model_id='te', img_norm=['0.4', '0.3'], pad='border')
    student = _model(distill='teacher.ptl', distill_alpha=0.3, distill_temperature=4, label_smoothing=0.1)
    student.attach_teacher(teacher)
    eng, teng = student.model.engine, teacher.model.engine
    thead, head = teacher.model._train_heads[0], student.model._train_heads[0]
    tf = nd.RoiTransform(224)
    for step, jitter in enumerate((False, True, True)):
        rois, t = _batch(10 + step, jitter)
        seen = {}
        real = nd.rois_to_device

        def spy(*a, **k):
            seen['kw'] = real(*a, **k)
            return seen['kw']
        if staged:
            with mock.patch.object(nd, 'rois_to_device', spy):
                n = student.stage_batch(rois, tf, t, train=True)
            student.use_staged()
            assert teng.in_slot == eng.in_slot == (step + 1) % 2               # the two engines' slots move in lockstep
            student.fit_current(n)
        else:
            seen['kw'] = real(rois, eng.dev, tf)
            n = student.fit_batch(seen['kw'], t.cuda())
        torch.cuda.synchronize()
        got = eng.teacher_logits[:n].clone()
        step_loss = eng.loss.clone()
        assert torch.equal(got, thead.logits[:n])
        # the loss the step left is the kernel's on the teacher buffer it read
        loss, _ = _direct(eng, head, n, 1.0)
        assert torch.equal(step_loss, loss)
        kw = dict(seen['kw'])
        assert ('jitter' in kw) == jitter
        if jitter:
            raw, once = _jitter_once(eng, rois)
            assert torch.equal(kw['pixels'], once) and not torch.equal(raw, once)          # jittered exactly once
        # the teacher's own eval_batch of the same (jittered) ROIs with the same flip codes, its own normalisation and pad
        tkw = {k: v for k, v in kw.items() if k != 'jitter'}
        tkw.update(mean=[0.4] * 3, std=[0.3] * 3, pad='border')
        assert 'flips' in tkw
        teacher.eval_batch(tkw)
        torch.cuda.synchronize()
        assert torch.equal(got, thead.logits[:n])
        # ... which is not what the student's own normalisation and geometry would have given it
        teacher.eval_batch({k: v for k, v in kw.items() if k != 'jitter'})
        torch.cuda.synchronize()
        assert not torch.equal(got, thead.logits[:n])
    # a validation batch is not staged for the teacher
    rois, t = _batch(20)
    slot = teng.in_slot
    n = student.stage_batch(rois, tf, t)
    student.use_staged()
    assert teng.in_slot == slot and teng.prefetched is None
    student.eval_current(n, with_loss=True)
    with pytest.raises(RuntimeError, match='not staged for the teacher'):
        student.fit_current(n)
    torch.cuda.synchronize()
