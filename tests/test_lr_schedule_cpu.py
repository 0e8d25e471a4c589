"""TRAIN --lr-schedule / --warmup / --lr-min and --optimizer AdamW on the host: the schedule's values against their defining properties and
torch.optim.lr_scheduler, the float64 AdamW twin of tests/sched_cases.py against torch.optim.AdamW, the command line with its refusals,
the hyper-parameter round trip, the optimizer op's `decoupled` operand in every program of a plan, and the declarations of
ifcbk_adamw_flat.  The kernel runs in tests/test_gpu_adamw.py, the engine in tests/test_gpu_sched_engine.py."""
import argparse
import ctypes as C
import math
import os
import re
from unittest import mock

import pytest
import torch

import sched_cases as sc
from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net, ops
from ifcb_classifier_amd.engine import Engine
from ifcb_classifier_amd.lr_schedule import LrSchedule, schedule_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE, T = 1e-3, 40


# ------------------------------------------------------------------------------------------------------ 1. the schedule's values
@pytest.mark.parametrize('lr_min', (0.0, BASE / 10))
@pytest.mark.parametrize('W', (0, 1, 2, 7))
@pytest.mark.parametrize('kind', ('constant', 'cosine', 'linear'))
def test_schedule_values(kind, W, lr_min):
    s = LrSchedule(kind, BASE, T, W, lr_min if kind != 'constant' else 0.0)
    r = [s.at(t) for t in range(T)]
    if W >= 1:
        assert r[0] == BASE / W and r[W - 1] == BASE == r[W]
        assert all(b > a for a, b in zip(r[:W - 1], r[1:W]))
    assert r[W] == BASE
    assert all(b <= a for a, b in zip(r[W:], r[W + 1:]))                       # never rises behind the warm-up
    if kind == 'constant':
        assert all(x == BASE for x in r[W:])                                  # the same bits, not a value near them
    else:
        assert r[T - 1] > s.lr_min and r[T - 1] < r[W]
        assert all(b < a for a, b in zip(r[W:], r[W + 1:]))
    assert s.at(T) == s.at(T + 1000) == r[T - 1]                              # behind the end: the last rate
    want = sc.torch_rates(kind, BASE, T, W, s.lr_min)
    worst = max(abs(a - b) for a, b in zip(r, want))
    print('%s W=%d lr_min=%g: worst |at(t) - torch| = %.3g' % (kind, W, s.lr_min, worst))
    assert worst <= 1e-9 * BASE


def test_schedule_refusals():
    for bad in (dict(kind='step'), dict(total_steps=0), dict(warmup_steps=T), dict(warmup_steps=-1), dict(lr_min=2 * BASE), dict(lr_min=-1e-9),
                dict(lr_min=float('nan')), dict(base=float('inf')), dict(total_steps=2.5)):
        kw = dict(kind='cosine', base=BASE, total_steps=T, warmup_steps=0, lr_min=0.0)
        kw.update(bad)
        with pytest.raises(ValueError, match='lr schedule'):
            LrSchedule(**kw)
    with pytest.raises(ValueError):
        LrSchedule('cosine', BASE, T).at(-1)


def test_steps_from_a_loader_length():
    assert schedule_steps(3, 1, 2) == (6, 2)
    assert schedule_steps(60, 0.5, 7) == (420, 4)                             # round(3.5) = 4: python rounds the tie to the even one
    assert schedule_steps(60, 0.3, 7) == (420, 2) and schedule_steps(5, 0, 9) == (45, 0)


# ------------------------------------------------------------------------------------------------------ 2. the twin against torch
@pytest.mark.parametrize('wd', (0.0, 1e-2))
def test_adamw_twin_against_torch(wd):
    f32 = sc.ob.f32
    n, b1, b2, eps, wd = 37, f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    g0 = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=g0, dtype=torch.float64)
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([w], lr=1e-3, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        lr = f32(1e-3 * (1.5 - 0.2 * step))                                   # a different rate each step
        g = torch.randn(n, generator=g0, dtype=torch.float64) * 10 ** (torch.rand(n, generator=g0, dtype=torch.float64) * 4 - 3)
        w.grad = g.clone()
        opt.param_groups[0]['lr'] = lr
        opt.step()
        got = sc.adamw(p, g, m, v, lr, b1, b2, eps, wd, step, 1.0, exact=True)
        p, m, v = got['p'][0], got['m'][0], got['v'][0]
        st = opt.state[w]
        for name, a, b in (('p', p, w.detach()), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
            assert torch.allclose(a, b, rtol=1e-13, atol=1e-15), (wd, step, name, float((a - b).abs().max()))
    assert not torch.equal(p, torch.randn(n, generator=torch.Generator().manual_seed(11), dtype=torch.float64))


def test_adamw_twin_bound_is_adams_plus_the_decay_product():
    g0 = torch.Generator().manual_seed(3)
    p, g = torch.randn(64, generator=g0), torch.randn(64, generator=g0)
    m, v = torch.randn(64, generator=g0) * 0.1, torch.rand(64, generator=g0) * 0.01
    a = (1e-3, 0.9, 0.999, 1e-8)
    # without decay: Adam's own twin and values, the bound wider by the product's rounding only
    w0, ad = sc.adamw(p, g, m, v, *a, 0.0, 3, 0.5), sc.ob.adam(p, g, m, v, *a, 0.0, 3, 0.5)
    for k in 'pmv':
        assert torch.equal(w0[k][0], ad[k][0])
    assert torch.equal(w0['m'][1], ad['m'][1]) and bool((w0['p'][1] > ad['p'][1]).all())
    assert bool((w0['p'][1] - ad['p'][1] <= 1.01 * sc.U * p.double().abs()).all())
    # with decay: not torch's L2 form
    w1, l2 = sc.adamw(p, g, m, v, *a, 0.05, 3, 0.5), sc.ob.adam(p, g, m, v, *a, 0.05, 3, 0.5)
    assert bool(((w1['p'][0] - l2['p'][0]).abs() > 2 * (w1['p'][1] + l2['p'][1])).any())
    assert torch.equal(w1['m'][0], w0['m'][0]) and not torch.equal(l2['m'][0], w0['m'][0])      # the moments never see the decay
    d = sc.decay_factor(1e-3, 0.05)
    assert d == float(torch.tensor(1.0 - float(torch.tensor(1e-3)) * float(torch.tensor(0.05)), dtype=torch.float32)) and d < 1.0


# ------------------------------------------------------------------------------------------------------ 3. command line, hparams
def _parse(*flags):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'resnet18', 'id', *flags])


def test_flags_parse_and_default():
    a = _parse()
    assert (a.optimizer, a.lr_schedule, a.warmup, a.lr_min) == ('Adam', 'constant', 0.0, 0.0)
    neuston_net.check_lr_flags(a)
    a = _parse('--optimizer', 'AdamW', '--weight-decay', '0.05', '--lr-schedule', 'cosine', '--warmup', '1.5', '--lr-min', '1e-5')
    assert (a.optimizer, a.weight_decay, a.lr_schedule, a.warmup, a.lr_min) == ('AdamW', 0.05, 'cosine', 1.5, 1e-5)
    neuston_net.check_lr_flags(a)
    neuston_net.check_lr_flags(_parse('--warmup', '2'))                       # warm-up into a constant rate
    neuston_net.check_lr_flags(_parse('--lr-schedule', 'linear', '--lr-min', '0.001'))      # lr_min == learning_rate
    for bad in (('--lr-schedule', 'step'), ('--warmup', '-1'), ('--warmup', 'nan'), ('--lr-min', '-0.1'), ('--lr-min', 'inf'),
                ('--optimizer', 'adamw')):
        with pytest.raises(SystemExit):
            _parse(*bad)
    text = neuston_net.argparse_nn()._subparsers._group_actions[0].choices['TRAIN'].format_help()
    for flag in ('--lr-schedule', '--warmup', '--lr-min'):
        assert flag in text
    assert text.count('(MI355X path, additive)') >= 4


@pytest.mark.parametrize('flags,message', [
    (('--lr-schedule', 'cosine', '--lr-min', '0.01'), '--lr-min 0.01 is above --learning-rate 0.001'),
    (('--lr-schedule', 'cosine', '--warmup', '3', '--emax', '3'), '--warmup 3 must be less than --emax 3'),
    (('--warmup', '60.5'), '--warmup 60.5 must be less than --emax 60'),
    (('--lr-min', '1e-4'), '--lr-min 0.0001 needs a decaying --lr-schedule'),
    (('--warmup', '1', '--lr-min', '1e-4'), '--lr-min 0.0001 needs a decaying --lr-schedule'),
])
def test_refusals_come_with_a_message(flags, message):
    with pytest.raises(SystemExit) as ei:
        neuston_net.check_lr_flags(_parse(*flags))
    assert message in str(ei.value)


class _HostEngine(Engine):
    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None, emax=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_args_yml_and_ptl_round_trip(tmp_path):
    import yaml
    a = _parse('--optimizer', 'AdamW', '--weight-decay', '0.05', '--lr-schedule', 'cosine', '--warmup', '1', '--lr-min', '1e-5', '--emax', '3')
    dumped = yaml.safe_load(yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v))
                                            for k, v in vars(a).items()}))
    assert (dumped['optimizer'], dumped['lr_schedule'], dumped['warmup'], dumped['lr_min']) == ('AdamW', 'cosine', 1.0, 1e-5)
    plain = yaml.safe_load(yaml.safe_dump(vars(_parse())))
    assert (plain['optimizer'], plain['lr_schedule'], plain['warmup'], plain['lr_min']) == ('Adam', 'constant', 0.0, 0.0)
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(argparse.Namespace(**dict(vars(a), classes=['a', 'b', 'c'], model_id='m')))
        eng = m.model.engine
        assert eng.optimizer == 'adamw' and eng.weight_decay == 0.05 and eng.lr_schedule is None and eng.lr_now == eng.lr == 0.001
        s = m.set_lr_schedule(2)
        assert s is eng.lr_schedule and (s.kind, s.base, s.total_steps, s.warmup_steps, s.lr_min) == ('cosine', 0.001, 6, 2, 1e-5)
        opt = m.configure_optimizers()
        assert isinstance(opt, torch.optim.AdamW) and opt.defaults['weight_decay'] == 0.05 and opt.defaults['lr'] == 0.001
        # ahead of the first step the groups hold the first step's rate; behind step 4 that step's, and the base as initial_lr
        grp = m.optimizer_state()['param_groups'][0]
        assert grp['initial_lr'] == 0.001 and grp['lr'] == C.c_float(s.at(0)).value == eng.lr_now and grp['weight_decay'] == 0.05
        assert set(grp) - {'initial_lr'} <= set(opt.state_dict()['param_groups'][0]) and grp['betas'] == (0.9, 0.999)
        eng.step_count = 4
        eng.M.normal_(); eng.V.uniform_()
        st = m.optimizer_state()
        assert st['param_groups'][0]['lr'] == C.c_float(s.at(3)).value == eng.lr_now < 0.001 and eng.lr == 0.001
        ck = m.checkpoint_dict(epoch=1, global_step=4)
        hp = ck['hyper_parameters']
        assert (hp['optimizer'], hp['weight_decay'], hp['lr_schedule'], hp['warmup'], hp['lr_min']) == ('AdamW', 0.05, 'cosine', 1.0, 1e-5)
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        e2 = m2.model.engine
        assert e2.optimizer == 'adamw' and e2.step_count == 4
        for i, ps in m2.optimizer_state()['state'].items():                   # load_optimizer_state accepts what optimizer_state wrote
            assert ps['step'] == 4 and torch.equal(ps['exp_avg'], st['state'][i]['exp_avg']) and torch.equal(ps['exp_avg_sq'], st['state'][i]['exp_avg_sq'])
        assert e2.lr_schedule is None and m2.set_lr_schedule(2).at(3) == s.at(3) and e2.lr_now == eng.lr_now
        # older files and plain runs: no schedule, Adam
        m3 = neuston_models.NeustonModel(_hparams())
        assert m3.model.engine.optimizer == 'adam' and m3.set_lr_schedule(5) is None and m3.model.engine.lr_schedule is None
        assert 'initial_lr' not in m3.optimizer_state()['param_groups'][0]
        m4 = neuston_models.NeustonModel(_hparams(warmup=1.0))                  # warm-up alone: a constant schedule behind it
        s4 = m4.set_lr_schedule(4)
        assert (s4.kind, s4.total_steps, s4.warmup_steps) == ('constant', 12, 4) and s4.at(0) == 0.001 / 4 and s4.at(4) == 0.001


def test_engine_arguments():
    net = graph.build('resnet18', 3, pretrained=False)
    with pytest.raises(ValueError, match='optimizer'):
        Engine(net, max_batch=2, plan_only=True, optimizer='adamax')
    with pytest.raises(ValueError, match='lr_schedule'):
        Engine(net, max_batch=2, plan_only=True, lr_schedule=0.5)
    with pytest.raises(ValueError, match='weight_decay'):
        Engine(net, max_batch=2, plan_only=True, optimizer='adamw', weight_decay=-0.1)


# ------------------------------------------------------------------------------------------------------ 4. layout
def test_the_decoupled_operand_is_i2_and_every_optimizer_op_of_a_plan_carries_it():
    assert ops.slot(_lib.OP_ADAM, 'decoupled') == 2 and ops.OPERANDS[_lib.OP_ADAM]['i'] == ('n', 'step', 'decoupled')
    assert ops.OPERANDS[_lib.OP_SGD]['i'] == ('n', 'step')                    # SGD has no decoupled form
    net = graph.build('resnet18', 3, pretrained=False)
    seen = {}
    for optimizer in ('adam', 'adamw'):
        eng = Engine(net, max_batch=2, plan_only=True, dtype='fp32', optimizer=optimizer, weight_decay=0.05, ema_decay=0.9)
        pl = eng.plan(2)
        flags = []
        for name in ('step', 'adam', 'adam_pack'):
            got = sc.opt_ops(eng, getattr(pl, name))
            assert got and all(o.f[ops.slot(_lib.OP_ADAM, 'weight_decay')] == C.c_float(0.05).value for o in got)
            flags += [int(o.i[2]) for o in got]
        assert len(sc.opt_ops(eng, pl.step)) > 1                              # buckets: each op inherits the flag by name
        assert set(flags) == {1 if optimizer == 'adamw' else 0}
        names = set()
        for o in sc.opt_ops(eng, pl.step):
            buf = C.create_string_buffer(64)
            assert eng.ctx.lib.ifcbk_op_kernel(C.byref(o), buf, 64) == 0
            names.add(buf.value.decode())
        assert names == {'adam_kernel<true>' if optimizer == 'adamw' else 'adam_kernel'}
        fl, by = C.c_double(), C.c_double()
        o = pl.adam.arr[0]
        eng.ctx.lib.ifcbk_op_cost(C.byref(o), C.byref(fl), C.byref(by))
        seen[optimizer] = (fl.value, by.value)
    assert seen['adam'] == seen['adamw'] and seen['adam'][1] > 0              # Adam's cost: the same bytes


def test_the_scheduled_rate_is_stamped_from_the_step_count_alone():
    net = graph.build('resnet18', 3, pretrained=False)
    s = LrSchedule('cosine', 1e-3, 6, 2)
    eng = Engine(net, max_batch=4, plan_only=True, dtype='fp32', lr_schedule=s)
    lr = ops.slot(_lib.OP_ADAM, 'lr')
    for N in (4, 3):                                                          # another batch size's plan carries the same rate
        pl = eng.plan(N)
        for k in (1, 4, 6, 9):
            eng.step_count = k
            for o in sc.opt_ops(eng, pl.step) + [pl.adam.arr[0], pl.adam_pack.arr[0]]:
                eng._set_update(o)
                assert o.f[lr] == C.c_float(s.at(k - 1)).value == eng.lr_now and o.i[1] == k
    assert eng.lr == 1e-3
    plain = Engine(net, max_batch=4, plan_only=True, dtype='fp32')
    o = plain.plan(4).adam.arr[0]
    plain.step_count = 5
    plain._set_update(o)
    assert o.f[lr] == C.c_float(1e-3).value and plain.lr_now == 1e-3 and int(o.i[2]) == 0


def test_declarations_of_the_entry_point():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    flat = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(',')]
              for m in re.finditer(r'IFCBK_API\s+int\s+(ifcbk_\w+)\s*\(([^;]*?)\)\s*;', flat)}
    assert protos['ifcbk_adamw_flat'] == protos['ifcbk_adam_clip_flat']       # the operand list of the clipped Adam call
    assert 'i[2] = decoupled' in hdr and 'ifcbk_adamw_flat' in hdr.split('IFCBK_OP_ADAM,')[0].split('IFCBK_OP_ADAM:')[1]
    assert 'ifcbk_adamw_flat' in _lib.EXPORTS and _lib._PROTOS['ifcbk_adamw_flat'] == _lib._PROTOS['ifcbk_adam_clip_flat']
    emap = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    assert 'global: ifcbk_*;' in emap                                         # the map passes every ifcbk_ symbol: this one too
    assert getattr(_lib.load(), 'ifcbk_adamw_flat').argtypes is not None
    ctx = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    assert re.search(r'\n\s*ADAM_N = 0, ADAM_STEP, ADAM_DECOUPLED,\s', ctx)
    # one kernel body, instantiated once each way, one launch site each
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'pool_head.hip')).read()
    assert src.count('template <bool DECOUPLED>') == 1 and src.count('adam_kernel<false>') == 1 and src.count('adam_kernel<true>') == 1
    assert math.isfinite(sc.decay_factor(1e-3, 0.05))
