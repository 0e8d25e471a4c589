"""TRAIN --accumulate without a GPU: the declarations of ifcbk_grad_accum_flat agree (header, export map, ctypes table, the built
library), the flag parses, refuses and reaches the hyper-parameters and args.yml, the schedule counts optimizer steps, and the plans of
an engine built with accumulate=1 are those of an engine built without the argument."""
import argparse
import math
import os
import re
from unittest import mock

import pytest
import torch

from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net, ops
from ifcb_classifier_amd.engine import Engine
from ifcb_classifier_amd.plan import Program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ 1. declarations
def test_declarations_of_the_entry_point():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    flat = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(',')]
              for m in re.finditer(r'IFCBK_API\s+int\s+(ifcbk_\w+)\s*\(([^;]*?)\)\s*;', flat)}
    assert protos['ifcbk_grad_accum_flat'] == ['ifcbk_ctx*', 'float* a', 'const float* g', 'int64_t n', 'int first', 'void* stream']
    assert 'ifcbk_grad_accum_flat' in _lib.EXPORTS
    res, args = _lib._PROTOS['ifcbk_grad_accum_flat']
    import ctypes as C
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p] and len(args) == 6
    emap = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    assert 'global: ifcbk_*;' in emap                                         # the map passes every ifcbk_ symbol: this one too
    assert getattr(_lib.load(), 'ifcbk_grad_accum_flat').argtypes is not None
    mk = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'Makefile')).read()
    assert ' grad_accum.hip' in mk
    # no op kind was added and the optimizer kinds keep their operand rows: the accumulator rides in their G operand
    assert max(_lib.OP_NAMES) == 40
    assert ops.OPERANDS[_lib.OP_ADAM]['p'][:2] == ('P', 'G') and ops.OPERANDS[_lib.OP_SGD]['p'][:2] == ('P', 'G')


# ------------------------------------------------------------------------------------------------------ 2. command line
def _parse(*flags):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'resnet18', 'id', *flags])


def test_flag_parses_defaults_and_refuses():
    assert _parse().accumulate == 1
    a = _parse('--accumulate', '4')
    assert a.accumulate == 4 and isinstance(a.accumulate, int)
    for bad in ('0', '-1', 'x', '1.5', ''):
        with pytest.raises(SystemExit):
            _parse('--accumulate', bad)
    text = neuston_net.argparse_nn()._subparsers._group_actions[0].choices['TRAIN'].format_help()
    assert '--accumulate K' in text and 'accumulate_grad_batches' in text
    assert '(MI355X path, additive) Gradient accumulation' in ' '.join(text.split())
    with pytest.raises(SystemExit):                                           # RUN has no such flag
        neuston_net.argparse_nn().parse_args(['RUN', 'src', 'm.ptl', 'rid', '--accumulate', '2'])


def test_a_k_beyond_the_batches_of_an_epoch_is_a_usage_error(capsys):
    for k, batches in ((1, 1), (7, 7), (2, 7)):
        neuston_net.check_accumulate(k, batches)
    for k, batches in ((8, 7), (2, 1)):
        with pytest.raises(SystemExit) as ei:
            neuston_net.check_accumulate(k, batches)
        assert ei.value.code == 2                                             # parser.error
        err = capsys.readouterr().err
        assert '--accumulate %d is more than the %d training batch' % (k, batches) in err


def test_train_refuses_it_before_a_model_is_built(tmp_path):
    """8 images at the default split and --batch 2: fewer training batches than K = 50, refused by do_training ahead of the model"""
    import numpy as np
    from PIL import Image
    for cls in ('a', 'b'):
        os.makedirs(tmp_path / 'src' / cls)
        for i in range(4):
            Image.fromarray(np.full((20, 30), 40 * i, np.uint8)).save(str(tmp_path / 'src' / cls / ('%s%d.png' % (cls, i))))
    a = neuston_net.argparse_nn().parse_args(['--loaders', '0', '--batch', '2', 'TRAIN', str(tmp_path / 'src'), 'resnet18', 'x', '--untrain',
                                              '--accumulate', '50', '--outdir', str(tmp_path / 'out')])
    neuston_net.argparse_nn_runtimeparams(a)
    with mock.patch.object(neuston_net, 'NeustonModel', side_effect=AssertionError('built a model')):
        with pytest.raises(SystemExit) as ei:
            neuston_net.do_training(a)
    assert ei.value.code == 2


# ------------------------------------------------------------------------------------------------------ 3. hparams, args.yml, schedule
class _HostEngine(Engine):
    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None, emax=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_args_yml_and_ptl_carry_the_value(tmp_path):
    import yaml
    a = _parse('--accumulate', '2', '--lr-schedule', 'cosine', '--emax', '3')
    dump = lambda ns: yaml.safe_load(yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v))
                                                     for k, v in vars(ns).items()}))
    assert dump(a)['accumulate'] == 2 and dump(_parse())['accumulate'] == 1
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(argparse.Namespace(**dict(vars(a), classes=['a', 'b', 'c'], model_id='m')))
        eng = m.model.engine
        assert m.accumulate == 2 and eng.accumulate == 2 and eng.acc_pending == 0
        assert eng.A is not None and eng.A.shape == eng.G.shape and eng.A.dtype == torch.float32 and eng.A.data_ptr() % 16 == 0
        ck = m.checkpoint_dict(epoch=1, global_step=4)
        assert ck['hyper_parameters']['accumulate'] == 2
        assert not [k for k in ck['state_dict'] if 'acc' in k.lower()]        # the accumulator is no part of a checkpoint
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.hparams.accumulate == 2 and m2.model.engine.accumulate == 2
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path, inference=True)       # RUN: the value is carried and ignored
        assert m3.hparams.accumulate == 2 and m3.model.engine.accumulate == 1 and m3.model.engine.A is None
        old = neuston_models.NeustonModel(_hparams())                         # older files and plain runs: no entry, one batch per step
        assert old.accumulate == 1 and old.model.engine.accumulate == 1 and old.model.engine.A is None
        one = neuston_models.NeustonModel(_hparams(accumulate=1))
        assert one.model.engine.accumulate == 1 and one.model.engine.A is None
        for bad in (0, -1, 2.0, '2', True):
            with pytest.raises(ValueError, match='accumulate'):
                neuston_models.NeustonModel(_hparams(accumulate=bad))


@pytest.mark.parametrize('K', (1, 2, 3, 7))
def test_the_schedule_counts_optimizer_steps(K):
    """7 training batches per epoch: ceil(7 / K) optimizer steps, the short last window included, times emax"""
    batches, emax = 7, 3
    steps = math.ceil(batches / K)
    assert steps == {1: 7, 2: 4, 3: 3, 7: 1}[K]
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(accumulate=K, lr_schedule='cosine', warmup=1.0, emax=emax))
        assert m.optimizer_steps(batches) == steps
        s = m.set_lr_schedule(m.optimizer_steps(batches))
        assert s is m.model.engine.lr_schedule and s.total_steps == emax * steps and s.warmup_steps == steps


def test_engine_argument():
    net = graph.build('resnet18', 3, pretrained=False)
    for bad in (0, -2, 1.0, 2.5, '2', None, True):
        with pytest.raises(ValueError, match='accumulate'):
            Engine(net, max_batch=2, plan_only=True, accumulate=bad)
    eng = Engine(net, max_batch=2, plan_only=True, accumulate=3)
    assert eng.accumulate == 3 and eng.acc_pending == 0 and eng.A.numel() == eng.nparam_padded
    eng.acc_pending = 2
    eng.init_weights(seed=1)                                                  # a window open at init_weights is dropped
    assert eng.acc_pending == 0
    with pytest.raises(RuntimeError, match='timing'):
        eng.train_step(2, ev_slot=0)
    with pytest.raises(RuntimeError, match='timing'):
        eng.train_step(2, op_ms=[])
    assert 'accumulate' in _window_message(eng)


def _window_message(eng):
    eng.window_batch = 1                                                      # (a plan-only engine: only the message is wanted)
    with pytest.raises(RuntimeError) as ei:
        eng._check_train_batch(2)
    msg = str(ei.value)
    assert 'use a smaller --batch per GPU (more GPUs)' in msg                 # the text as it was, appended to
    return msg


# ------------------------------------------------------------------------------------------------------ 4. plans
def _programs(pl):
    return {k: v for k, v in vars(pl).items() if isinstance(v, Program)}


def _table(prog, bases):
    """the op table with every pointer replaced by (buffer name, byte offset) where it points into one of the engine's flat buffers and by
    a non-NULL mark elsewhere (two engines allocate at different addresses): -> [(bytes of the op without pointers, its pointers)]"""
    out = []
    for k in range(prog.n):
        o = _lib.Op.from_buffer_copy(prog.arr[k])
        ptrs = []
        for j in range(12):
            v = o.p[j] or 0
            where = [(name, v - b) for name, (b, nbytes) in bases.items() if b <= v < b + nbytes]
            ptrs.append(where[0] if where else bool(v))
            o.p[j] = None
        out.append((bytes(o), tuple(ptrs)))
    return out


def _bases(eng):
    return {name: (getattr(eng, name).data_ptr(), getattr(eng, name).numel() * 4) for name in ('P', 'G', 'M', 'V', 'A', 'E')
            if getattr(eng, name, None) is not None}


@pytest.mark.parametrize('kw', (dict(), dict(optimizer='sgd', momentum=0.9, clip_grad=1.0), dict(optimizer='adamw', weight_decay=0.05, ema_decay=0.9)))
def test_accumulate_1_builds_the_plans_of_an_engine_without_the_argument(kw):
    net = lambda: graph.build('resnet18', 7, pretrained=False)                 # (a graph per engine: an engine keeps its layout on the nodes)
    base = Engine(net(), max_batch=4, plan_only=True, dtype='fp32', **kw)
    one = Engine(net(), max_batch=4, plan_only=True, dtype='fp32', accumulate=1, **kw)
    two = Engine(net(), max_batch=4, plan_only=True, dtype='fp32', accumulate=2, **kw)
    assert one.A is None and base.A is None and two.A is not None
    for N in (4, 3):
        pb, p1, p2 = (_programs(e.plan(N)) for e in (base, one, two))
        assert len(pb) == 13 and set(p1) == set(pb) and set(p2) == set(pb) | {'acc_update', 'acc_count'}
        for name in pb:
            want = _table(pb[name], _bases(base))
            assert _table(p1[name], _bases(one)) == want, name
            assert _table(p2[name], _bases(two)) == want, name                # K > 1 adds programs and changes none
            assert p1[name].tags == pb[name].tags and p1[name].lanes == pb[name].lanes
        # the window's update: the plan's optimizer op reading A where it read G, then the whole repack; the counters alone
        upd, cnt = _table(p2['acc_update'], _bases(two)), _table(p2['acc_count'], _bases(two))
        adam_pack = _table(pb['adam_pack'], _bases(base))
        assert len(upd) == len(adam_pack) - 1 and cnt == adam_pack[-1:] and p2['acc_count'].arr[0].kind == _lib.OP_STEP_COUNTERS
        assert upd[1:] == adam_pack[1:-1] and upd[0][0] == adam_pack[0][0]
        g = ops.slot(p2['acc_update'].arr[0].kind, 'G')
        assert adam_pack[0][1][g] == ('G', 0) and upd[0][1][g] == ('A', 0)
        assert upd[0][1][:g] + upd[0][1][g + 1:] == adam_pack[0][1][:g] + adam_pack[0][1][g + 1:]
