"""TRAIN --resident on the GPU, whole models (resnet18, batch 8, the tiny PNG trees of tests/resident_cases.py): a batch staged through
NeustonModel.stage_resident_batch against the same batch through stage_batch(collate_rois(items)) -- the input slot's bytes, the mixing
factors and targets, the teacher's slot -- three training steps on alternating slots in fp32 and bf16 bit for bit, and the resident
blob unchanged after a jittered epoch."""
import argparse
import random

import numpy as np
import pytest
import torch

import resident_cases as rc

pytestmark = pytest.mark.gpu
B = 8


def _hp(**kw):
    hp = dict(MODEL='resnet18', classes=['ant', 'bee', 'cat'], pretrained=False, batch_size=B, precision='fp32', model_id='rs', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _model(seed=11, **kw):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(seed)
    return NeustonModel(_hp(**kw), max_batch=B)


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    """kind -> (dataset, its ResidentSet on the host), decoded once for the module and left unchanged"""
    from ifcb_classifier_amd.neuston_data import NeustonDataset, ResidentSet
    root = tmp_path_factory.mktemp('resident')
    out = {}
    for kind in ('grey', 'rgb'):
        ds = NeustonDataset(rc.write_tree(str(root / kind), kind))
        out[kind] = (ds, ResidentSet.build(ds))
    return out


def _on_device(m, res):
    eng = m.model.engine
    return res.to_device(eng.dev, eng.prefetch_stream())


def _slot_input(eng, n):
    s = eng.in_slot
    return (eng.in_u8[s] if eng.in_kind[s] == 'u8' else eng.in_bufs[s])[:n].clone()


def _stage_both(m, ds, res, idx, tf_of, seed, train=True):
    """the batch ``idx`` through the upload and through the cut, each under random.seed(seed) and a transform of its own (a BatchMix
    draws from its own generator) -> per feed a dict of what the staging left"""
    from ifcb_classifier_amd.neuston_data import collate_rois
    eng = m.model.engine
    out = []
    for resident in (False, True):
        tf = tf_of()
        ds.transforms = tf
        random.seed(seed)
        if resident:
            idx_host = np.asarray(idx, np.int64)
            with torch.cuda.stream(res.stream):
                idx_dev = torch.from_numpy(idx_host).to(eng.dev)
            n = m.stage_resident_batch(res, idx_dev, idx_host, tf, train=train)
        else:
            rois, targets, _ = collate_rois([ds[i] for i in idx])
            n = m.stage_batch(rois, tf, targets, train=train)
        state = random.getstate()
        m.use_staged()
        torch.cuda.synchronize()
        got = dict(n=n, kind=eng.in_kind[eng.in_slot], x=_slot_input(eng, n), target=eng.target[:n].clone(), state=state)
        if eng.mix:
            got['lam'] = eng.mix_lam[eng.in_slot][:n].clone()
        if m.teacher is not None and train:
            teng = m.teacher.model.engine
            got['teacher'] = _slot_input(teng, n)
        out.append(got)
    return out


def _equal(a, b):
    assert a['n'] == b['n'] and a['kind'] == b['kind'] and a['state'] == b['state']
    for k in ('x', 'target', 'lam', 'teacher'):
        assert (k in a) == (k in b)
        if k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k


IDX = [17, 3, 3, 22, 0, 9, 14, 6]                                   # (one index twice, as wrap-around padding gives)
NORM = ((0.5, 0.4, 0.3), (0.2, 0.25, 0.3))


@pytest.mark.parametrize('kind', ['grey', 'rgb'])
@pytest.mark.parametrize('name', ['plain', 'flip xy rot90', 'pad border', 'jitter', 'mixup'])
def test_one_batch_is_staged_to_the_same_bytes(trees, kind, name):
    from ifcb_classifier_amd.neuston_data import BatchMix, RoiTransform
    ds, host = trees[kind]
    tf_of = {'plain': lambda: RoiTransform(224, NORM),
             'flip xy rot90': lambda: RoiTransform(224, None, True, True, rot90=True),
             'pad border': lambda: RoiTransform(224, NORM, pad='border'),
             'jitter': lambda: RoiTransform(224, None, True, False, jitter=[0.2, 0.3]),
             'mixup': lambda: RoiTransform(224, None, False, True, mix=BatchMix(0.4, 1.0, seed=3))}[name]
    m = _model(**(dict(mixup=0.4, cutmix=1.0) if name == 'mixup' else {}))
    res = _on_device(m, host)
    blob = res.dev['pixels'].clone()
    for seed, idx in ((1, IDX), (2, IDX[:5])):
        a, b = _stage_both(m, ds, res, idx, tf_of, seed)
        _equal(a, b)
        assert a['n'] == len(idx) and a['target'].tolist() == [ds.targets[i] for i in idx]
        assert ('lam' in a) == (name == 'mixup')
    assert torch.equal(res.dev['pixels'], blob)                      # the resident blob is only read


def test_with_a_teacher_attached_its_slot_is_equal_too(trees):
    from ifcb_classifier_amd.neuston_data import RoiTransform
    ds, host = trees['grey']
    teacher = _model(seed=5, model_id='te', img_norm=['0.4', '0.3'], pad='border')
    student = _model(distill='teacher.ptl', distill_alpha=0.3, distill_temperature=4)
    student.attach_teacher(teacher)
    res = _on_device(student, host)
    blob = res.dev['pixels'].clone()
    for seed, tf_of in ((1, lambda: RoiTransform(224, None, True, True)), (2, lambda: RoiTransform(224, None, True, True, jitter=[0.3, 0.3]))):
        a, b = _stage_both(student, ds, res, IDX, tf_of, seed)
        assert 'teacher' in a
        _equal(a, b)
        assert not torch.equal(a['teacher'], a['x'])                 # its own pad and normalisation
    # a validation batch is not staged for the teacher on either feed
    a, b = _stage_both(student, ds, res, IDX[:4], lambda: RoiTransform(224), 3, train=False)
    _equal(a, b)
    assert 'teacher' not in a and teacher.model.engine.prefetched is None
    assert torch.equal(res.dev['pixels'], blob)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_three_training_steps_on_alternating_slots_leave_the_same_bits(trees, precision):
    """the look-ahead loop of Trainer.fit over three batches, fed by uploads and by cuts: P, M, V, RB and the loss"""
    from ifcb_classifier_amd.neuston_data import BatchMix, RoiTransform, collate_rois
    ds, host = trees['grey']
    batches = [IDX, [1, 2, 4, 5, 7, 8, 10, 11], [23, 20, 19, 13, 12]]
    m = _model(precision=precision, mixup=0.4)
    eng = m.model.engine
    res = _on_device(m, host)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rb0, p0 = eng.RB.clone(), eng.P.clone()
    runs = []
    for resident in (False, True):
        m.load_state_dict(sd0)
        eng.RB.copy_(rb0)
        eng.nbt.zero_(); eng.M.zero_(); eng.V.zero_(); eng.step_count = 0
        eng.params_changed()
        tf = RoiTransform(224, NORM, True, True, jitter=[0.2, 0.2], mix=BatchMix(0.4, seed=3))
        ds.transforms = tf
        random.seed(7)

        def stage(idx):
            if resident:
                idx_host = np.asarray(idx, np.int64)
                with torch.cuda.stream(res.stream):
                    idx_dev = torch.from_numpy(idx_host).to(eng.dev)
                return m.stage_resident_batch(res, idx_dev, idx_host, tf, train=True)
            rois, targets, _ = collate_rois([ds[i] for i in idx])
            return m.stage_batch(rois, tf, targets, train=True)

        losses, slots = [], []
        n_next = None
        for k, idx in enumerate(batches):
            n = stage(idx) if n_next is None else n_next
            m.use_staged()
            slots.append(eng.in_slot)
            n_next = stage(batches[k + 1]) if k + 1 < len(batches) else None
            m.fit_current(n)
            losses.append(eng.loss.clone())
        torch.cuda.synchronize()
        assert slots in ([1, 0, 1], [0, 1, 0])
        runs.append(dict(P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(), RB=eng.RB.clone(), loss=torch.stack(losses), state=random.getstate()))
    a, b = runs
    assert bool(torch.isfinite(a['loss']).all()) and not torch.equal(a['P'], p0)
    assert a['state'] == b['state']
    for k in ('loss', 'P', 'M', 'V', 'RB'):
        assert torch.equal(a[k], b[k]), k


def test_the_resident_blob_is_unchanged_after_a_jittered_epoch(trees):
    """a whole epoch of the resident loader with flips and jitter: ifcbk_roi_jitter maps each batch's copy in place, never the set"""
    from ifcb_classifier_amd import neuston_net as nn_
    from ifcb_classifier_amd.neuston_data import RoiTransform
    ds, host = trees['grey']
    m = _model()
    eng = m.model.engine
    res = _on_device(m, host)
    tf = RoiTransform(224, None, True, True, jitter=[0.5, 0.5])
    ds.transforms = tf
    loader = nn_.ResidentLoader(ds, res, B, True, 0, 1, 3)
    seen, n_next = [], None
    for (rois, targets, paths), nxt in nn_.Trainer._lookahead(loader):
        assert isinstance(rois, nn_.ResidentBatch) and targets.dtype == torch.int64
        assert paths == [ds.images[i] for i in rois.idx_host] and targets.tolist() == [ds.targets[i] for i in rois.idx_host]
        n = nn_.Trainer._stage(m, rois, tf, targets, train=True) if n_next is None else n_next
        m.use_staged()
        n_next = nn_.Trainer._stage(m, nxt[0], tf, nxt[1], train=True) if nxt is not None else None
        m.fit_current(n)
        seen += rois.idx_host.tolist()
    torch.cuda.synchronize()
    assert len(loader) == 3 and sorted(seen) == list(range(24)) and seen == loader.indices()
    assert np.array_equal(res.dev['pixels'].cpu().numpy(), host.blob)
    for k, a in (('offs', host.offs), ('hs', host.hs), ('ws', host.ws), ('targets', host.targets)):
        assert np.array_equal(res.dev[k].cpu().numpy(), a), k
    with pytest.raises(IndexError):
        m.stage_resident_batch(res, torch.tensor([24]).cuda(), np.array([24]), tf)
