"""Engine(accumulate=K) on the device.  K = 1 is the engine without the argument, bit for bit.  A window of K > 1 is the hand-made
sequence on today's entry points -- per batch forward_train + loss + backward and a clone of G, the clones summed in fp32 in order by
torch, the sum written to G, ONE update with grad_scale = 1 / K, the repack -- bit for bit in P, M, V, RB, nbt, the packed weights (and
E, ERB with a weight average), for both ways a batch is launched, the three optimizers and a clip at half the window's norm; the update
lies within the float64 twin's bound (tests/option_matrix.py); the step count, the schedule's rate and the weight average count optimizer
steps while BatchNorm counts batches; a short window is flushed at 1 / K; the batches of a window may differ in size; init_weights drops
an open window; per-op timing is refused; and the data-parallel step exchanges nothing until the window's last batch, then every element
of the accumulator exactly once.

Shapes: resnet18, 7 classes, batch 4, fp32 (the smallest at which the plan has its full op lists, tests/test_gpu_clip_engine.py), and a
batch of 2 for the second plan of the mixed window."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_cases as cc
import option_matrix as om
from option_matrix import real_mask, reset as _reset, same

pytestmark = pytest.mark.gpu

B, S, NC = 4, 224, 7
KEYS = ('P', 'M', 'V', 'RB', 'nbt', 'Wsh')
OPTS = {'adam': dict(), 'sgd': dict(optimizer='sgd', momentum=0.9), 'adamw': dict(optimizer='adamw', weight_decay=0.05),
        'ema': dict(ema_decay=0.9)}
_ENG = {}


def _engine(tag, **kw):
    """one engine per configuration for the whole module (reset by every test that takes it)"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    if tag not in _ENG:
        _ENG[tag] = Engine(graph.build('resnet18', NC, pretrained=False), device=0, max_batch=B, dtype='fp32', **kw)
    _reset(_ENG[tag])
    return _ENG[tag]


class Rig:
    pass


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(3)]
    r.ys = [torch.randint(0, NC, (B,), generator=g) for _ in range(3)]
    r.xs.append(r.xs[1][:2].contiguous())                                     # batch 3: two images, a second plan of the same engine
    r.ys.append(r.ys[1][:2].contiguous())
    yield r
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _load(r, eng, k):
    n = eng.load_input_nchw(r.xs[k])
    eng.target[:n].copy_(r.ys[k])
    return n


def _snap(eng, keys=KEYS):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).clone() for k in keys}


def _keys(eng):
    return KEYS + (('E', 'ERB') if eng.ema_decay is not None else ())


def _acc_batches(r, eng, ks, mode='plain', flush=False):
    """the batches `ks` through the accumulating engine's train_step -> the fp32 loss of each"""
    losses = []
    eng.graph_train = mode == 'graph'
    try:
        for k in ks:
            n = _load(r, eng, k)
            pl = eng.train_step(n)
            assert mode != 'graph' or 'fwd_bwd' in pl.graphs
            losses.append(eng.loss.clone())
    finally:
        eng.graph_train = False
    if flush:
        eng.accumulate_flush()
    return losses


def _hand_window(r, eng, ks, K):
    """today's entry points on an engine without the argument: the window of batches `ks` as ONE update from the fp32 sum of their
    gradients times 1 / K -> the fp32 loss of each batch"""
    clones, losses = [], []
    for k in ks:
        n = _load(r, eng, k)
        pl = eng.forward_train(n)
        eng.run(pl.loss)
        eng.backward(n)
        clones.append(eng.G.clone())
        losses.append(eng.loss.clone())
    total = clones[0].clone()
    for c in clones[1:]:
        total = total + c                                                     # fp32, in order
    eng.G.copy_(total)
    eng.step_count += 1
    eng._ema_begin_step()
    eng._set_update(pl.adam.arr[0], 1.0 / K)
    eng.run(pl.adam)
    eng._ema_end_step()
    eng.run(pl.pack)                                                          # the repack
    eng.packed, eng.eval_stats_ready = True, False
    return losses


def _windows(n, K):
    return [list(range(i, min(i + K, n))) for i in range(0, n, K)]


def _loss_sum(losses):
    tot = torch.zeros(1, dtype=torch.float32, device=losses[0].device)
    for v in losses:
        tot = tot + v
    return tot


def _check_equal(got, want, keys, what):
    for key in keys:
        assert same(got[key], want[key]), (what, key)


# ------------------------------------------------------------------------------------------------------ K = 1
@pytest.mark.parametrize('mode', ('plain', 'graph'))
def test_k1_is_the_engine_without_the_argument(rig, mode):
    base, one = _engine('base'), _engine('one', accumulate=1)
    assert one.A is None and base.A is None and one.accumulate == 1
    assert not hasattr(one.plan(B), 'acc_update')
    for k in range(3):
        for eng in (base, one):
            _load(rig, eng, k)
            eng.graph_train = mode == 'graph'
            try:
                eng.train_step(B)
            finally:
                eng.graph_train = False
            assert eng.acc_pending == 0
        a, b = _snap(base, KEYS + ('loss', 'loss_sum')), _snap(one, KEYS + ('loss', 'loss_sum'))
        _check_equal(b, a, KEYS + ('loss', 'loss_sum'), (mode, k))
    assert one.accumulate_flush() is False


# ------------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize('mode', ('plain', 'graph'))
@pytest.mark.parametrize('K', (2, 3))
@pytest.mark.parametrize('opt', sorted(OPTS))
def test_a_window_is_the_hand_made_sequence(rig, opt, K, mode):
    acc, twin = _engine('%s K%d' % (opt, K), accumulate=K, **OPTS[opt]), _engine('%s twin' % opt, **OPTS[opt])
    assert acc.A is not None and acc.A.numel() == acc.nparam_padded and acc.A.data_ptr() % 16 == 0
    acc.A.fill_(float('nan'))                                                 # the first batch of a window overwrites it
    got_losses = _acc_batches(rig, acc, range(3), mode, flush=True)           # K = 2: a window of two and a flushed window of one
    want_losses = []
    for w in _windows(3, K):
        want_losses += _hand_window(rig, twin, w, K)
    keys = _keys(acc)
    _check_equal(_snap(acc, keys), _snap(twin, keys), keys, (opt, K, mode))
    assert acc.step_count == twin.step_count == len(_windows(3, K)) and acc.acc_pending == 0
    assert bool((acc.nbt == 3).all())
    for a, b in zip(got_losses, want_losses):
        assert same(a, b)
    assert same(acc.loss_sum, _loss_sum(want_losses))                         # train_loss stays the sum over the loader's batches


@pytest.mark.parametrize('mode', ('plain', 'graph'))
@pytest.mark.parametrize('K', (2, 3))
def test_a_window_clipped_at_half_its_norm(rig, K, mode):
    loose = _engine('loose K%d' % K, accumulate=K, clip_grad=1e30)
    _acc_batches(rig, loose, range(K))
    norm = float(loose.clip_state[0])                                         # the device's norm of the first window's A / K
    assert 0 < norm < np.inf and float(loose.clip_state[1]) == 1.0
    mx = float(np.float32(norm / 2))
    acc, twin = _engine('clip K%d' % K, accumulate=K, clip_grad=mx), _engine('clip twin K%d' % K, clip_grad=mx)
    _acc_batches(rig, acc, range(K), mode)
    _hand_window(rig, twin, range(K), K)
    torch.cuda.synchronize()
    assert same(acc.clip_state[:4], twin.clip_state[:4])                      # the norm is taken over A, the figures count one step
    n2, coef, top, clipped = acc.grad_clip_stats()
    assert n2 == norm and 0.49 < coef < 0.51 and top == norm and clipped == 1
    _check_equal(_snap(acc), _snap(twin), KEYS, ('clip', K, mode))
    _acc_batches(rig, acc, range(K, 3), mode, flush=True)                     # K = 2: one more batch, flushed
    for w in _windows(3, K)[1:]:
        _hand_window(rig, twin, w, K)
    _check_equal(_snap(acc), _snap(twin), KEYS, ('clip, flushed', K, mode))
    assert same(acc.clip_state[:4], twin.clip_state[:4])


# ------------------------------------------------------------------------------------------------------ float64
def test_the_update_against_the_float64_twin(rig):
    """check_optimizer evaluates its twin at grad_scale 1, so the snapshot's G is A times the window's 1 / K = 0.5: an exact product, and
    the fp32 value the kernel forms from A and its grad_scale operand"""
    eng = _engine('adam K2', accumulate=2)
    before, orig = {}, eng._acc_apply

    def spy(grad_scale):
        torch.cuda.synchronize()
        before.update(P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(), A=eng.A.clone(), grad_scale=grad_scale)
        return orig(grad_scale)
    eng._acc_apply = spy
    try:
        losses = _acc_batches(rig, eng, range(2))
    finally:
        del eng._acc_apply
    assert before['grad_scale'] == 0.5 and eng.step_count == 1
    before['G'] = before['A'] * 0.5
    worst = om.check_optimizer('accumulate K=2', eng, before, 1, cc.geometry(eng.ctx.lib)[0])
    print('worst err / bound %.3g' % worst)
    assert worst < 1.0
    assert same(eng.loss_sum, losses[0] + losses[1]) and float(eng.loss_sum) > 0


# ------------------------------------------------------------------------------------------------------ counting
def test_steps_rate_and_average_count_optimizer_steps(rig):
    from ifcb_classifier_amd.lr_schedule import LrSchedule
    sched = LrSchedule('cosine', 1e-3, 6, 0)
    eng = _engine('counting', accumulate=2, lr_schedule=sched, ema_decay=0.9)
    es = []
    for k in range(4):
        _acc_batches(rig, eng, [k % 3])
        es.append(_snap(eng, ('E', 'ERB', 'nbt')))
        assert eng.step_count == (k + 1) // 2 and eng.acc_pending == (k + 1) % 2
    assert eng.step_count == 2 and bool((eng.nbt == 4).all()) and eng.nbt.numel() == len(eng.bn_nodes)
    rates = [C.c_float(sched.at(t)).value for t in range(4)]
    assert len(set(rates)) == 4
    assert eng.lr_now == rates[1] != rates[3]                                 # the rate of optimizer step 2, not of batch 4
    assert eng.plan(B).acc_update.arr[0].f[eng._upd_lr] == rates[1]
    assert eng.ema_updates == 2
    assert same(es[0]['E'], _initial_p(eng)) and not same(es[1]['E'], es[0]['E'])          # E moved with the first update,
    assert same(es[2]['E'], es[1]['E']) and same(es[2]['ERB'], es[1]['ERB'])               # stood still through batch 3,
    assert not same(es[3]['E'], es[2]['E']) and not same(es[3]['ERB'], es[2]['ERB'])       # and moved with the second


def _initial_p(eng):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    tag = 'initial'
    if tag not in _ENG:
        _ENG[tag] = Engine(graph.build('resnet18', NC, pretrained=False), device=0, max_batch=B, dtype='fp32')
    _reset(_ENG[tag])
    return _ENG[tag].P


# ------------------------------------------------------------------------------------------------------ short window, mixed sizes, reset
def test_a_short_window_is_flushed_at_one_over_k(rig):
    acc, twin = _engine('adam K3', accumulate=3), _engine('adam twin')
    pending = [acc.acc_pending]
    for k in range(2):
        _acc_batches(rig, acc, [k])
        pending.append(acc.acc_pending)
    assert acc.step_count == 0
    assert acc.accumulate_flush() is True
    pending.append(acc.acc_pending)
    assert pending == [0, 1, 2, 0] and acc.step_count == 1
    _hand_window(rig, twin, range(2), 3)
    got = _snap(acc)
    _check_equal(got, _snap(twin), KEYS, 'flush')
    assert acc.accumulate_flush() is False                                    # a closed window: nothing happens
    _check_equal(_snap(acc), got, KEYS, 'second flush')
    assert acc.step_count == 1


def test_the_batches_of_a_window_may_differ_in_size(rig):
    acc, twin = _engine('adam K2', accumulate=2), _engine('adam twin')
    _acc_batches(rig, acc, [0, 3])                                            # batch 4, then batch 2: two plans of one engine
    assert acc.step_count == 1 and acc.acc_pending == 0 and len(acc._plans) == 2
    _hand_window(rig, twin, [0, 3], 2)
    _check_equal(_snap(acc), _snap(twin), KEYS, 'mixed')


def test_init_weights_drops_an_open_window(rig):
    acc, twin = _engine('adam K2', accumulate=2), _engine('adam twin')
    _acc_batches(rig, acc, [2])
    assert acc.acc_pending == 1
    _reset(acc)                                                               # init_weights: the window is closed, A keeps batch 2's gradient
    assert acc.acc_pending == 0 and acc.step_count == 0
    _acc_batches(rig, acc, [0, 1])                                            # first = 1 again: a fresh engine's window
    assert acc.step_count == 1
    _hand_window(rig, twin, [0, 1], 2)
    _check_equal(_snap(acc), _snap(twin), KEYS, 'reset')


def test_per_op_timing_is_refused(rig):
    acc = _engine('adam K2', accumulate=2)
    _load(rig, acc, 0)
    with pytest.raises(RuntimeError, match='timing'):
        acc.train_step(B, ev_slot=0)
    with pytest.raises(RuntimeError, match='timing'):
        acc.train_step(B, op_ms=(C.c_float * 4)())
    assert acc.acc_pending == 0 and acc.step_count == 0


# ------------------------------------------------------------------------------------------------------ data parallel
def test_the_data_parallel_window_exchanges_once(rig):
    """two replicas holding the same gradient, modelled on one GPU: the stand-in all-reduce doubles its slice, and 1 / (K world) of 2 A
    is 1 / K of A exactly"""
    dp, single = _engine('dp K2', accumulate=2, dp_world=2), _engine('adam K2', accumulate=2)
    assert dp.dp_world == 2
    calls = []

    def all_reduce(t):
        off = (t.data_ptr() - dp.A.data_ptr()) // 4
        assert 0 <= off and off + t.numel() <= dp.nparam_padded and t.dtype == torch.float32
        calls.append((off, off + t.numel()))
        t.mul_(2)

    _load(rig, dp, 0)
    dp.train_step_ddp(B, 2, all_reduce)
    assert calls == [] and dp.acc_pending == 1 and dp.step_count == 0         # no collective in micro-step 1
    _load(rig, dp, 1)
    dp.train_step_ddp(B, 2, all_reduce)
    assert dp.acc_pending == 0 and dp.step_count == 1
    assert len(calls) >= 2                                                    # per finished bucket, beside backward
    cover = sorted(calls)
    assert cover[0][0] == 0 and cover[-1][1] == dp.nparam_padded
    assert all(a[1] == b[0] for a, b in zip(cover, cover[1:]))                # [0, nparam_padded) exactly once
    _acc_batches(rig, single, [0, 1])
    torch.cuda.synchronize()
    real = real_mask(dp)
    for key in ('P', 'M', 'V'):
        assert same(getattr(dp, key).cpu()[real], getattr(single, key).cpu()[real]), key
    assert same(dp.RB, single.RB) and same(dp.nbt, single.nbt) and same(dp.loss_sum, single.loss_sum)
    # a short window: the whole of A in one call ahead of the update
    del calls[:]
    _load(rig, dp, 2)
    dp.train_step_ddp(B, 2, all_reduce)
    assert calls == [] and dp.acc_pending == 1
    assert dp.accumulate_flush(2, all_reduce) is True
    assert calls == [(0, dp.nparam_padded)] and dp.acc_pending == 0 and dp.step_count == 2
    _acc_batches(rig, single, [2], flush=True)
    torch.cuda.synchronize()
    for key in ('P', 'M', 'V'):
        assert same(getattr(dp, key).cpu()[real], getattr(single, key).cpu()[real]), key
