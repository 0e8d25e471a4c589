"""Engine(ema_decay=...) on the device: the training trajectory keeps its bits, the averages E / ERB follow the oracle of
tests/ema_bounds.py step by step, every way a step is launched leaves the same E / ERB, ema_weights() shows the averaged model and
puts every bit back, and a write to P from outside restarts the average.

Shapes: those of tests/test_gpu_step_modes.py -- resnet18 at batch 8, side 224 and inception_v3 at batch 6, side 299, the smallest at
which the plans have their full op lists, several optimizer buckets included."""
import pytest
import torch

import ema_bounds as eb

pytestmark = pytest.mark.gpu

FAMILIES = {'resnet18': ('resnet18', 8, 224), 'inception_v3': ('inception_v3', 6, 299)}
DECAY = 0.9
KEYS = ('loss', 'P', 'M', 'V', 'RB', 'nbt')


class Rig:
    pass


def _engine(name, B, **kw):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    eng = Engine(graph.build(name, 7, pretrained=False), device=0, max_batch=B, **kw)
    _reset(eng)
    return eng


def _reset(eng, seed=4321):
    """the state of a fresh engine with the weights of `seed` (init_weights is a write from outside: the average restarts)"""
    eng.init_weights(seed=seed)
    eng.M.zero_()
    eng.V.zero_()
    eng.RB.zero_()
    for k, v in eng.bviews.items():
        if k.endswith('running_var'):
            v.fill_(1.0)
    eng.nbt.zero_()
    eng.loss_sum.zero_()
    eng.step_count = 0
    eng.dropout_seed, eng.dropout_calls = 5, 0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _snap(eng):
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).clone() for k in KEYS}
    if eng.E is not None:
        out['E'], out['ERB'] = eng.E.clone(), eng.ERB.clone()
    return out


def _load(r, eng, k):
    eng.load_input_nchw(r.xs[k])
    eng.target[:r.B].copy_(r.ys[k])


def _step(r, eng, k, mode='plain'):
    B = r.B
    _load(r, eng, k)
    if mode == 'plain':
        eng.train_step(B)
    elif mode == 'graph':
        assert not eng.graph_train
        eng.graph_train = True
        try:
            pl = eng.train_step(B)
            assert 'fwd_bwd' in pl.graphs
        finally:
            eng.graph_train = False
    elif mode == 'ev_all':
        eng.train_step(B, ev_slot=0)
    elif mode == 'split':
        pl = eng.forward_train(B)
        eng.run(pl.loss)
        eng.backward(B)
        eng.adam_step(B)
    elif mode == 'ddp':
        eng.train_step_ddp(B, 1, lambda t: None)
    else:
        raise KeyError(mode)
    return _snap(eng)


def _run(r, eng, mode, nsteps=3):
    _reset(eng)
    return [_step(r, eng, k, mode) for k in range(nsteps)]


@pytest.fixture(scope='module')
def rig(request):
    name, B, S = FAMILIES[request.param]
    r = Rig()
    r.family, r.name, r.B = request.param, name, B
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(4)]
    r.ys = [torch.randint(0, 7, (B,), generator=g) for _ in range(4)]
    r.base = _engine(name, B)
    r.ema = _engine(name, B, ema_decay=DECAY)
    assert r.base.E is None and r.ema.E.shape == r.ema.P.shape
    assert len(r.ema.plan(B).step_adam_idxs) > 1                    # several buckets
    r.cache = {}
    yield r
    r.base.close()
    r.ema.close()


def _plain(r):
    """(initial P, initial RB, the three plain steps of the averaging engine)"""
    if 'plain' not in r.cache:
        _reset(r.ema)
        p0, rb0 = r.ema.P.clone(), r.ema.RB.clone()
        r.cache['plain'] = (p0, rb0, [_step(r, r.ema, k) for k in range(3)])
    return r.cache['plain']


ALL = pytest.mark.parametrize('rig', sorted(FAMILIES), indirect=True)


def _check_recurrence(tag, p0, rb0, outs):
    """E after step k against the oracle applied to the device E after step k - 1 and the device P after step k; ERB likewise"""
    e_prev, erb_prev = p0, rb0                                      # step 1 starts from E = the initial P, ERB = the initial RB
    for k, o in enumerate(outs):
        w = eb.weight(DECAY, k + 1)
        assert w == eb.f32(1.0 - (2.0 + k) / (11.0 + k))            # the warm-up: 2/11, 3/12, 4/13
        eb.check('%s step %d E' % (tag, k + 1), o['E'].cpu(), e_prev.cpu(), o['P'].cpu(), w)
        eb.check('%s step %d ERB' % (tag, k + 1), o['ERB'].cpu(), erb_prev.cpu(), o['RB'].cpu(), w)
        assert not same(o['E'], o['P']) and not same(o['E'], e_prev) and not same(o['ERB'], erb_prev)
        e_prev, erb_prev = o['E'], o['ERB']


@ALL
def test_three_steps_keep_the_trajectory_and_follow_the_oracle(rig):
    r = rig
    ref = _run(r, r.base, 'plain')
    p0, rb0, outs = _plain(r)
    assert r.ema.ema_updates == 3 and not r.ema.ema_stale
    for k in range(3):
        for key in KEYS:
            assert same(outs[k][key], ref[k][key]), (r.family, 'step %d' % (k + 1), key)
    assert not same(ref[0]['P'], ref[1]['P']) and bool(torch.isfinite(ref[2]['P']).all())
    _check_recurrence(r.family, p0, rb0, outs)


@ALL
def test_sgd_with_momentum(rig):
    r = rig
    a = _engine(r.name, r.B, optimizer='sgd', momentum=0.9, lr=0.005)
    b = _engine(r.name, r.B, optimizer='sgd', momentum=0.9, lr=0.005, ema_decay=DECAY)
    try:
        ref = _run(r, a, 'plain')
        _reset(b)
        p0, rb0 = b.P.clone(), b.RB.clone()
        outs = [_step(r, b, k) for k in range(3)]
        for k in range(3):
            for key in KEYS:
                assert same(outs[k][key], ref[k][key]), (r.family, 'step %d' % (k + 1), key)
        _check_recurrence(r.family + ' sgd', p0, rb0, outs)
    finally:
        a.close()
        b.close()


@ALL
@pytest.mark.parametrize('mode', ('graph', 'ev_all', 'split', 'ddp'))
def test_every_launch_mode_leaves_the_same_average(rig, mode):
    r = rig
    _p0, _rb0, ref = _plain(r)
    outs = _run(r, r.ema, mode)
    for k in range(3):
        for key in ('P', 'RB', 'E', 'ERB'):
            assert same(outs[k][key], ref[k][key]), (r.family, mode, 'step %d' % (k + 1), key)


def _probs(r, eng, k):
    """the eval forward's probabilities with the main head's logits behind them (after a few steps on noise the softmax of these
    untrained networks saturates to one-hot rows, which two different models share; their logits they do not)"""
    _load(r, eng, k)
    pl = eng.forward_eval(r.B)
    eng.run(pl.softmax)
    torch.cuda.synchronize()
    main = [h for h in eng.heads if not h.aux][0]
    return torch.cat([eng.probs[:r.B], main.logits[:r.B]], 1).clone()


@ALL
def test_ema_weights_shows_the_averaged_model_and_leaves_no_trace(rig):
    r = rig
    eng = r.ema
    never = _run(r, eng, 'plain', nsteps=4)                         # four steps, never entered
    outs = _run(r, eng, 'plain', nsteps=3)
    raw = _probs(r, eng, 3)
    with eng.ema_weights():
        inside = _probs(r, eng, 3)
    # a second engine whose parameters and running statistics were loaded from E / ERB
    other = r.base
    other.P.copy_(outs[2]['E'])
    other.RB.copy_(outs[2]['ERB'])
    other.params_changed()
    want = _probs(r, other, 3)
    assert same(inside, want) and not same(inside, raw)
    after = _snap(eng)
    for key in ('P', 'M', 'V', 'RB', 'nbt', 'E', 'ERB'):
        assert same(after[key], outs[2][key]), key
    assert eng.step_count == 3 and eng.ema_updates == 3 and not eng.packed
    assert same(_probs(r, eng, 3), raw)
    # eval forwards do not touch what a train step reads: the fourth step is the fourth step of the engine that never entered
    fourth = _step(r, eng, 3)
    for key in KEYS + ('E', 'ERB'):
        assert same(fourth[key], never[3][key]), key
    with pytest.raises(RuntimeError, match='without ema_decay'):
        with r.base.ema_weights():
            pass


@ALL
def test_a_write_from_outside_restarts_the_average(rig):
    r = rig
    eng = r.ema
    _run(r, eng, 'plain', nsteps=2)
    assert eng.ema_updates == 2
    eng.init_weights(seed=99)
    assert eng.ema_stale
    p0, rb0 = eng.P.clone(), eng.RB.clone()
    o = _step(r, eng, 2)
    assert eng.ema_updates == 1 and not eng.ema_stale
    w = eb.weight(DECAY, 1)
    eb.check('restart E', o['E'].cpu(), p0.cpu(), o['P'].cpu(), w)
    eb.check('restart ERB', o['ERB'].cpu(), rb0.cpu(), o['RB'].cpu(), w)
