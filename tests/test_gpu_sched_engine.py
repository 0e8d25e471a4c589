"""Engine(lr_schedule=...) and Engine(optimizer='adamw') on the device.  Every way a step is launched carries fp32(schedule.at(k)) in the
lr operand of every optimizer op it runs (every bucket, the split update, the data-parallel tail) and leaves P / M / V within the bound
of the float64 twin evaluated at that rate (tests/sched_cases.py); the launch modes agree bit for bit; a constant schedule is the engine
without one; AdamW alone, with the weight average, with clipping and under a schedule; a saved and reloaded optimizer state goes on down
the same curve.

Shapes: resnet18, 7 classes, batch 4, fp32 (the smallest at which the plan has its full op lists, as tests/test_gpu_clip_engine.py);
inception_v3 at batch 2 for the aux head; squeezenet at batch 2 for the channel padding inside the flat buffers."""
import argparse
import ctypes as C

import pytest
import torch

import sched_cases as sc
from option_matrix import real_mask as _real_mask, reset as _reset, same

pytestmark = pytest.mark.gpu

B, S, NC = 4, 224, 7
KEYS = ('P', 'M', 'V', 'RB', 'nbt', 'loss')
WD = 0.05


def _f32(v):
    return C.c_float(v).value


def _cosine(T=6, W=2, base=1e-3, lr_min=0.0):
    from ifcb_classifier_amd.lr_schedule import LrSchedule
    return LrSchedule('cosine', base, T, W, lr_min)


def _engine(name, b, **kw):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    eng = Engine(graph.build(name, NC, pretrained=False), device=0, max_batch=b, dtype='fp32', **kw)
    _reset(eng)
    return eng


class Rig:
    pass


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(6)]
    r.ys = [torch.randint(0, NC, (B,), generator=g) for _ in range(6)]
    r.sched = _cosine()
    r.eng = _engine('resnet18', B, lr_schedule=r.sched)
    assert len(r.eng.plan(B).step_adam_idxs) > 1                              # several buckets
    r.plain_bits = None
    yield r
    r.eng.close()


def _load(r, eng, k):
    eng.load_input_nchw(r.xs[k])
    eng.target[:B].copy_(r.ys[k])


def _step(r, eng, k, mode):
    """one step in a launch mode -> (the snapshot the twin starts from, the optimizer ops that ran)"""
    torch.cuda.synchronize()
    before = {K: getattr(eng, K).clone() for K in ('P', 'M', 'V')}
    if eng.ema_decay is not None:
        before['E'] = eng.P.clone() if eng.ema_stale else eng.E.clone()       # (a stale average restarts from P inside the step)
    _load(r, eng, k)
    pl = eng.plan(B)
    if mode == 'plain':
        eng.train_step(B)
        ran = [pl.step.arr[j] for j in pl.step_adam_idxs]
    elif mode == 'ev':
        eng.train_step(B, ev_slot=0)
        ran = [pl.step_timed_all[j] for j in pl.step_adam_idxs]
    elif mode == 'graph':
        eng.graph_train = True
        try:
            eng.train_step(B)
            assert 'fwd_bwd' in pl.graphs
        finally:
            eng.graph_train = False
        ran = [pl.adam_pack.arr[0]]
    elif mode == 'split':
        eng.forward_train(B)
        eng.run(pl.loss)
        eng.backward(B)
        eng.adam_step(B)
        ran = [pl.adam.arr[0]]
    else:
        raise KeyError(mode)
    torch.cuda.synchronize()
    before['G'] = eng.G.clone()                                               # (no optimizer op writes G: the gradient this step took)
    return before, ran


def _lr_slots(eng, ran, k, want):
    from ifcb_classifier_amd import _lib, ops
    lr, stp = ops.slot(_lib.OP_ADAM, 'lr'), ops.slot(_lib.OP_ADAM, 'step')
    for o in ran:
        assert o.kind == _lib.OP_ADAM and o.f[lr] == want and o.i[stp] == k + 1, (k, o.f[lr], want, o.i[stp])
    assert eng.lr_now == (want if eng.lr_schedule is not None else eng.lr)    # (without a schedule: the base, as given)


def _snap(eng):
    return {k: getattr(eng, k).clone() for k in KEYS}


# ------------------------------------------------------------------------------------------------------ 6. the scheduled rate
@pytest.mark.parametrize('mode', ('plain', 'ev', 'graph', 'split'))
def test_every_launch_mode_carries_the_steps_rate(rig, mode):
    eng, s = rig.eng, rig.sched
    if mode != 'plain' and rig.plain_bits is None:                            # (run on its own: the plain steps first)
        _reset(eng)
        rig.plain_bits = []
        for k in range(6):
            _step(rig, eng, k, 'plain')
            rig.plain_bits.append(_snap(eng))
    _reset(eng)
    rates, snaps = [], []
    for k in range(6):
        before, ran = _step(rig, eng, k, mode)
        want = _f32(s.at(k))
        _lr_slots(eng, ran, k, want)
        assert len(ran) == (len(eng.plan(B).step_adam_idxs) if mode in ('plain', 'ev') else 1)
        worst = sc.check_optimizer('sched %s step %d' % (mode, k + 1), eng, before, k + 1, want)
        assert worst < 1.0
        rates.append(want)
        snaps.append(_snap(eng))
    assert rates[0] == _f32(0.5e-3) and rates[1] == rates[2] == _f32(1e-3) and rates[2] > rates[3] > rates[4] > rates[5] > 0
    assert eng.lr == 1e-3                                                     # the base stays what the twins read
    if mode == 'plain':
        rig.plain_bits = snaps
        # the rate matters: the twin at the base rate is out of bounds at the first (half-rate) step
        _reset(eng)
        before, _ran = _step(rig, eng, 0, 'plain')
        want = sc.optimizer_reference(eng, before, 1, eng.lr)
        w, e = want['P']
        assert bool(((eng.P.double() - w.to(eng.P.device)).abs() > e.to(eng.P.device)).any())
    else:
        for k in range(6):
            for key in KEYS:
                assert same(snaps[k][key], rig.plain_bits[k][key]), (mode, k, key)


def test_a_constant_schedule_is_the_engine_without_one(rig):
    from ifcb_classifier_amd.lr_schedule import LrSchedule
    plain = _engine('resnet18', B)
    const = _engine('resnet18', B, lr_schedule=LrSchedule('constant', plain.lr, 6, 0))
    try:
        assert plain.lr_schedule is None and plain.lr_now == plain.lr
        for k in range(3):
            _step(rig, plain, k, 'plain')
            _before, ran = _step(rig, const, k, 'plain' if k != 1 else 'graph')
            _lr_slots(const, ran, k, _f32(1e-3))
            a, b = _snap(plain), _snap(const)
            for key in KEYS:
                assert same(a[key], b[key]), (k, key)
    finally:
        plain.close()
        const.close()


def test_two_replicas_take_the_scheduled_rate(rig):
    import dp_twin
    from ifcb_classifier_amd import _lib, ops
    s = _cosine()
    tw = dp_twin.Twin('resnet18', B, S, nc=NC, dtype='fp32', lr_schedule=s)   # (warm: one plain step, so the exchange step is step 2)
    try:
        assert all(e.step_count == 1 and e.lr_now == _f32(s.at(0)) for e in tw.engs)
        local = tw.local(0)
        torch.cuda.synchronize()
        before = [{K: getattr(e, K).clone() for K in ('P', 'M', 'V')} for e in tw.engs]
        tw.ddp_step(0, local)
        want = _f32(s.at(1))
        for r, eng in enumerate(tw.engs):
            o = eng.plan(B).adam_pack.arr[0]
            assert o.f[ops.slot(_lib.OP_ADAM, 'lr')] == want and o.i[1] == 2 and o.f[ops.slot(_lib.OP_ADAM, 'grad_scale')] == 0.5
            assert eng.lr_now == want and eng.step_count == 2
            before[r]['G'] = eng.G * 0.5                                      # the averaged gradient (a power of two: exact)
            assert sc.check_optimizer('sched dp replica %d' % r, eng, before[r], 2, want) < 1.0
        for key in ('P', 'M', 'V'):
            assert same(getattr(tw.engs[0], key), getattr(tw.engs[1], key)), key
    finally:
        tw.close()


# ------------------------------------------------------------------------------------------------------ 7. AdamW
_COMBOS = {
    'alone': dict(),
    'ema': dict(ema_decay=0.9),
    'clip': dict(clip_grad=1e-3),                                             # far below the norm of a fresh resnet18's gradient
    'cosine': 'cosine',
}


@pytest.mark.parametrize('combo', sorted(_COMBOS))
def test_adamw_against_the_twin(rig, combo):
    kw = _COMBOS[combo]
    s = _cosine() if kw == 'cosine' else None
    eng = _engine('resnet18', B, optimizer='adamw', weight_decay=WD, **(dict(lr_schedule=s) if s is not None else kw))
    try:
        pl = eng.plan(B)
        assert all(int(pl.step.arr[j].i[2]) == 1 for j in pl.step_adam_idxs) and int(pl.adam.arr[0].i[2]) == 1 == int(pl.adam_pack.arr[0].i[2])
        p0 = eng.P.clone()
        for k in range(3):
            before, ran = _step(rig, eng, k, 'plain')
            lr = _f32(s.at(k)) if s is not None else _f32(1e-3)
            _lr_slots(eng, ran, k, lr)
            assert sc.check_optimizer('adamw %s step %d' % (combo, k + 1), eng, before, k + 1, lr) < 1.0
            if combo == 'clip':
                _norm, coef, _top, clipped = eng.grad_clip_stats()
                assert coef < 1.0 and clipped == k + 1
            if k == 0:
                # the decay is decoupled: torch's L2 form of the same weight_decay is out of the twin's bounds
                l2 = sc.ob.adam(before['P'], before['G'], before['M'], before['V'], lr, eng.betas[0], eng.betas[1], eng.eps, WD, 1, 1.0)['p'][0]
                want, e = sc.optimizer_reference(eng, before, 1, lr, sc.cc.geometry(eng.ctx.lib)[0])['P']
                assert bool(((l2 - want.cpu()).abs() > 2 * e.cpu()).any()) or combo == 'clip'
        assert not same(eng.P, p0)
    finally:
        eng.close()


def test_adamw_inception_v3_with_its_aux_head():
    eng = _engine('inception_v3', 2, optimizer='adamw', weight_decay=WD)
    try:
        assert len([h for h in eng.heads if h.aux]) == 1
        g = torch.Generator().manual_seed(2)
        r = Rig()
        r.xs, r.ys = [torch.rand(2, 3, 299, 299, generator=g).cuda()], [torch.tensor([1, 5])]
        torch.cuda.synchronize()
        before = {K: getattr(eng, K).clone() for K in ('P', 'M', 'V')}
        eng.load_input_nchw(r.xs[0])
        eng.target[:2].copy_(r.ys[0])
        eng.train_step(2)
        torch.cuda.synchronize()
        before['G'] = eng.G.clone()
        assert sc.check_optimizer('adamw inception_v3', eng, before, 1, _f32(1e-3)) < 1.0
    finally:
        eng.close()


def test_adamw_leaves_the_padding_inside_the_flat_buffer_at_zero():
    """squeezenet's classifier conv pads its output channels to a 16-byte chunk: elements of P that belong to no parameter, decayed like
    the rest, must stay exactly 0 (sched_cases.check_optimizer asserts it for P, M and V)"""
    eng = _engine('squeezenet', 2, optimizer='adamw', weight_decay=WD)
    try:
        assert any(getattr(n, 'kind', '') == 'cb' and n.K != n.K_real for n in eng.net.nodes)
        pad = ~_real_mask(eng)
        assert int(pad.sum()) > 4
        g = torch.Generator().manual_seed(2)
        torch.cuda.synchronize()
        before = {K: getattr(eng, K).clone() for K in ('P', 'M', 'V')}
        eng.load_input_nchw(torch.rand(2, 3, S, S, generator=g).cuda())
        eng.target[:2].copy_(torch.tensor([0, 6]))
        eng.train_step(2)
        torch.cuda.synchronize()
        before['G'] = eng.G.clone()
        assert sc.check_optimizer('adamw squeezenet', eng, before, 1, _f32(1e-3)) < 1.0
        assert bool((eng.P.cpu()[pad] == 0).all()) and bool((before['P'].cpu()[pad] == 0).all())
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ 8. life cycle
def _hp(**kw):
    hp = dict(MODEL='resnet18', classes=['c%d' % i for i in range(NC)], pretrained=False, batch_size=B, precision='fp32', model_id='sch',
              resize=224, img_norm=None, seed=3, optimizer='AdamW', weight_decay=WD, learning_rate=1e-3, lr_schedule='cosine', warmup=1.0,
              lr_min=0.0, emax=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_a_reloaded_optimizer_state_goes_on_down_the_curve(rig, tmp_path):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp(), max_batch=B)
    m2 = None
    try:
        eng = m.model.engine
        s = m.set_lr_schedule(2)                                              # 3 epochs of 2 steps, one of them warm-up
        assert (s.total_steps, s.warmup_steps) == (6, 2) and eng.optimizer == 'adamw'
        for k in range(3):
            _step(rig, eng, k, 'plain')
        st = m.optimizer_state()
        grp = st['param_groups'][0]
        assert grp['lr'] == _f32(s.at(2)) and grp['initial_lr'] == 1e-3 and all(v['step'] == 3 for v in st['state'].values())
        path = str(tmp_path / 'mid.ckpt')
        torch.save(m.checkpoint_dict(epoch=1, global_step=3), path)
        want = []
        for k in range(3, 6):
            _step(rig, eng, k, 'plain')
            want.append(_snap(eng))
        m2 = NeustonModel.load_from_checkpoint(path, max_batch=B)
        e2 = m2.model.engine
        assert e2.step_count == 3 and e2.lr_schedule is None
        m2.set_lr_schedule(2)
        assert e2.lr_now == _f32(s.at(2))                                     # the rate follows the loaded step count, nothing else was saved
        e2.dropout_seed, e2.dropout_calls = eng.dropout_seed, 0
        for k in range(3, 6):
            _before, ran = _step(rig, e2, k, 'plain')
            _lr_slots(e2, ran, k, _f32(s.at(k)))
            got = _snap(e2)
            for key in ('P', 'M', 'V', 'RB', 'loss'):
                assert same(got[key], want[k - 3][key]), (k, key)
    finally:
        m.model.engine.close()
        if m2 is not None:
            m2.model.engine.close()
