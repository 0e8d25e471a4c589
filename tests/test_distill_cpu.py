"""TRAIN --distill on the host: the reference, bound and float32 emulation of tests/distill_cases.py, the header and the binding, the op
table Engine(plan_only=True) builds with and without distill, the kernel name of an op with p[6], the flags, the class-list check
and the hyper-parameter round trip.  The kernel runs in tests/test_gpu_distill_*.py."""
import argparse
import ctypes as C
import math
import os
import sys
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

import distill_cases as dc  # noqa: E402
import loss_smooth_bounds as sb  # noqa: E402
from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine, check_distill  # noqa: E402


# ------------------------------------------------------------------------------------------------------ reference, bound, emulation
def _torch64(l, t, z, cw, weight, eps, alpha, T):
    """Hinton's loss with torch's own functions in float64, and its gradient by autograd"""
    a, eps, alpha, T = (dc.f32(v) for v in (weight, eps, alpha, T))
    s = l.double().requires_grad_(True)
    ce = torch.nn.CrossEntropyLoss(weight=None if cw is None else cw.double(), label_smoothing=eps)(s, t)
    kl = F.kl_div(F.log_softmax(s / T, 1), F.softmax(z.double() / T, 1), reduction='batchmean')
    loss = a * ((1 - alpha) * ce + alpha * T * T * kl)
    loss.backward()
    return loss.detach(), s.grad


@pytest.mark.parametrize('N,NC', [(1, 1), (3, 2), (3, 5), (257, 3), (256, 101)])
def test_reference_is_hintons_loss_in_torch(N, NC):
    for case in dc.CASES:
        alpha, T, eps, weight, wm, offset = case[:6]
        if wm == 'zero' and NC == 1:
            continue                                        # 0 / 0 on both sides
        l, t, z, cw = dc.inputs(N, NC, wm, offset)
        loss, dl = dc.reference(l, t, z, cw, weight, eps, alpha, T)
        want_loss, want_dl = _torch64(l, t, z, cw, weight, eps, alpha, T)
        # two float64 forms of one value: they cancel differently (the comparison test_mix_cpu.py uses for its reference)
        assert torch.allclose(dl, want_dl, rtol=1e-12, atol=1e-13), dc.case_name(N, NC, case)
        assert abs(float(loss) - float(want_loss)) <= 1e-12 * (abs(float(want_loss)) + 5), dc.case_name(N, NC, case)
        # ... and the bound's own 'want' is the reference
        b = dc.bounds(l, t, z, cw, weight, eps, alpha, T)
        assert torch.allclose(b['dlogits'][0], dl, rtol=1e-12, atol=1e-13) and abs(float(b['loss'][0]) - float(loss)) <= 1e-12 * (abs(float(loss)) + 5)


@pytest.mark.parametrize('N,NC', dc.SHAPES)
def test_float32_emulation_of_the_kernel_stays_within_the_bound(N, NC):
    worst = 0.0
    for case in dc.CASES:
        alpha, T, eps, weight, wm, offset, acc, with_dl = case
        l, t, z, cw = dc.inputs(N, NC, wm, offset)
        old = dc.OLD_LOSS if acc else None
        got = dc.emulate(l, t, z, cw, weight, eps, alpha, T, old_loss=old)
        if wm == 'zero' and NC == 1:
            # the only class weighs nothing: W == 0 and 0 / 0 in the kernel's arithmetic as in torch's
            assert bool(torch.isnan(got['loss']).all()) and bool(torch.isnan(got['dlogits']).all())
            assert math.isnan(float(dc.reference(l, t, z, cw, weight, eps, alpha, T)[0]))
            continue
        want = dc.bounds(l, t, z, cw, weight, eps, alpha, T, old_loss=old)
        assert bool(torch.isfinite(want['dlogits'][1]).all()) and bool(torch.isfinite(want['loss'][1]).all())
        worst = max(worst, dc.check('emulation ' + dc.case_name(N, NC, case), got, want))
    print('emulation (%d, %d): worst err/bound %.3f' % (N, NC, worst))
    assert 0.0 <= worst <= 1.0


def test_every_parameter_value_is_in_the_case_list():
    for k, vals in enumerate((dc.ALPHAS, dc.TS, dc.EPSS, dc.SCALES, dc.WEIGHTS, (False, True), (0, 1), (0, 1))):
        assert {c[k] for c in dc.CASES} == set(vals), k
    assert len(dc.SHAPES) == 36


def test_offset_variant_underflows_q_and_not_r():
    for N, NC in ((1, 5), (3, 5), (257, 100)):
        l, t, z, cw = dc.inputs(N, NC, 'none', True)
        for T in dc.TS:
            q = torch.softmax(z / T, 1)
            r = torch.softmax(l / T, 1)
            row = (N // 2 + 1) % N
            assert int((q[row] == 0).sum()) == NC - 1 and bool((r > 0).all())
            got = dc.emulate(l, t, z, cw, 1.0, 0.0, 1.0, T)
            # the row's dlogits are alpha T / N * r away from the one surviving class
            zero = q[row] == 0
            want = (torch.tensor(T, dtype=torch.float32) / N * r[row])[zero]
            assert torch.allclose(got['dlogits'][row][zero], want, rtol=1e-5, atol=0) and bool(torch.isfinite(got['loss']).all())


def test_special_cases_of_the_reference():
    N, NC = 7, 5
    l, t, z, cw = dc.inputs(N, NC, 'random')
    # alpha == 0: the smoothed hard loss, reference and bound side by side
    a, b = dc.reference(l, t, z, cw, 0.4, 0.1, 0.0, 4.0), sb.reference(l, t, cw, 0.4, 0.1)
    assert torch.allclose(a[0], b[0], rtol=1e-13) and torch.allclose(a[1], b[1], rtol=1e-13, atol=1e-300)
    # alpha == 1 without class weights: no dependence on the target
    l, t, z, _ = dc.inputs(N, NC, 'none')
    a, b = dc.reference(l, t, z, None, 1.0, 0.0, 1.0, 4.0), dc.reference(l, (t + 1) % NC, z, None, 1.0, 0.0, 1.0, 4.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ea, eb = dc.emulate(l, t, z, None, 1.0, 0.0, 1.0, 4.0), dc.emulate(l, (t + 1) % NC, z, None, 1.0, 0.0, 1.0, 4.0)
    assert torch.equal(ea['loss'], eb['loss']) and torch.equal(ea['dlogits'], eb['dlogits'])
    # teacher == student: K == 0 and the soft gradient vanishes
    a = dc.reference(l, t, l, None, 1.0, 0.0, 1.0, 4.0)
    assert abs(float(a[0])) < 1e-15 and float(a[1].abs().max()) < 1e-16


# ------------------------------------------------------------------------------------------------------ header, binding
def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'ifcbk.h')).read()
    fn = 'ifcbk_softmax_xent_distill'
    assert 'IFCBK_API int %s(' % fn in hdr
    decl = hdr[hdr.index('IFCBK_API int %s(' % fn):]
    decl = decl[:decl.index(';')]
    assert decl.count(',') + 1 == 15                        # the ctx and 14 arguments
    assert fn in _lib.EXPORTS and len(_lib._PROTOS[fn][1]) == 15
    f = getattr(_lib.load(), fn)                            # AttributeError if the library does not export it
    assert f.argtypes is not None and len(f.argtypes) == 15 and f.restype is C.c_int
    assert [a for a in f.argtypes].count(C.c_float) == 4
    assert max(_lib.OP_NAMES) == 40                         # no new op kind
    assert 'p[6] = a teacher' in hdr and 'f[3] = alpha, f[4] = temperature' in hdr


# ------------------------------------------------------------------------------------------------------ plans
def _plan(model, B, dtype='bf16', **kw):
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, keep, clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(model, 7), max_batch=B, dtype=dtype, plan_only=True, **kw)
        return eng, eng.plan(B)


def _table(pl, strip=False):
    out = []
    for prog in mpf.PROGRAMS:
        p = getattr(pl, prog)
        ops = []
        for o in (p.arr[k] for k in range(p.n)):
            f = tuple(o.f)
            if strip and o.kind in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W):
                f = f[:3] + (0.0, 0.0) + f[5:]
            ops.append((o.kind, o.flags, tuple(o.i), f, bytes(o.u)))
        out.append((prog, ops, list(p.tags)))
    return out


@pytest.mark.parametrize('kw', [dict(), dict(class_weights=[0.5, 1.0, 2.0, 1.0, 1.0, 3.0, 0.1], label_smoothing=0.1)], ids=['plain', 'cw_ls'])
def test_distill_engine_points_the_train_loss_ops_at_its_teacher_buffer(kw):
    eng, pl = _plan('inception_v3', 2, distill=(0.3, 4), **kw)
    assert eng.distill == (0.3, 4.0)
    tl = eng.teacher_logits
    assert tl.dtype == torch.float32 and tuple(tl.shape) == (2, 7)
    for prog in ('loss', 'step', 'fwd_loss', 'fwd_bwd'):
        p = getattr(pl, prog)
        ops = [p.arr[k] for k in range(p.n) if p.tags[k] in ('loss', 'loss_aux')]
        assert len(ops) == 2 and all(o.p[6] == tl.data_ptr() and o.p[5] is None for o in ops), prog      # both heads, one set of logits
        assert all((o.p[4] == eng.class_weight.data_ptr()) if kw else (o.p[4] is None) for o in ops)
        assert all(o.f[2] == 0.0 and abs(o.f[1] - kw.get('label_smoothing', 0.0)) < 1e-7 for o in ops)
        assert all(abs(o.f[3] - 0.3) < 1e-7 and o.f[4] == 4.0 for o in ops)
        assert [o.f[0] for o in ops] == [1.0, pytest.approx(0.4)]                                        # the aux term keeps its factor
    ev = pl.eval_loss.arr[0]
    assert pl.eval_loss.n == 1 and ev.p[6] is None and ev.f[3] == 0.0 and ev.f[4] == 0.0 and ev.kind == ops[0].kind
    # the same buffer in the other slot's plan: the teacher runs on the step's stream, not in the prefetch
    eng._select_slot(1)
    assert all(eng.plan(2).loss.arr[k].p[6] == tl.data_ptr() for k in range(2))
    # everything but p[6], f[3], f[4] is the table of an engine without distill
    eng0, pl0 = _plan('inception_v3', 2, **kw)
    assert _table(pl, strip=True) == _table(pl0)
    assert not hasattr(eng0, 'teacher_logits') and eng0.distill is None


@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 4)])
def test_distill_none_is_the_default_engine(model, B):
    eng0, pl0 = _plan(model, B)
    eng1, pl1 = _plan(model, B, distill=None)
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    for prog in mpf.PROGRAMS:
        p = getattr(pl1, prog)
        assert all(p.arr[k].p[6] is None for k in range(p.n) if p.arr[k].kind in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W))


def test_engine_refuses_distill_with_focal_or_mix_and_bad_values():
    with pytest.raises(ValueError, match='focal_gamma'):
        _plan('resnet18', 2, distill=(0.5, 4.0), focal_gamma=2.0)
    with pytest.raises(ValueError, match='mix'):
        _plan('resnet18', 2, distill=(0.5, 4.0), mix=True)
    for bad in ((-0.1, 4), (1.5, 4), (float('nan'), 4), (0.5, 0), (0.5, -1), (0.5, float('inf')), (0.5, float('nan')), (0.5,), 'x', 3):
        with pytest.raises(ValueError, match='distill'):
            check_distill(bad)
    assert check_distill(None) is None and check_distill((0, 1)) == (0.0, 1.0) and check_distill([1, 0.5]) == (1.0, 0.5)
    assert check_distill((0.5, 4), focal_gamma=0.0, mix=False) == (0.5, 4.0)


def test_op_kernel_and_cost_name_the_distill_loss_only_with_p6():
    eng, pl = _plan('resnet18', 2, distill=(0.5, 4.0))
    lib = _lib.load()
    name = C.create_string_buffer(128)
    fl, by = C.c_double(), C.c_double()
    o = pl.loss.arr[0]
    assert lib.ifcbk_op_kernel(C.byref(o), name, 128) == 0 and name.value == b'softmax_xent_distill_kernel'
    assert lib.ifcbk_op_cost(C.byref(o), C.byref(fl), C.byref(by)) == 0 and by.value == 3 * 4 * 2 * 7 + 2 * 8 and fl.value > 0
    e = pl.eval_loss.arr[0]
    name.value = b''
    assert lib.ifcbk_op_kernel(C.byref(e), name, 128) == 0 and name.value == b''
    assert lib.ifcbk_op_cost(C.byref(e), C.byref(fl), C.byref(by)) == 0 and by.value == 0 and fl.value == 0
    # an op with the factors of a mixed batch keeps its name
    _, plm = _plan('resnet18', 2, mix=True)
    assert lib.ifcbk_op_kernel(C.byref(plm.loss.arr[0]), name, 128) == 0 and name.value == b'softmax_xent_mix_kernel'
    # ... and a conv op
    conv = [pl.fwd_train.arr[k] for k in range(pl.fwd_train.n) if pl.fwd_train.arr[k].kind == _lib.OP_CONV_FWD_AFFINE
            or pl.fwd_train.arr[k].kind == _lib.OP_CONV_FWD]
    _, pl0 = _plan('resnet18', 2)
    conv0 = [pl0.fwd_train.arr[k] for k in range(pl0.fwd_train.n) if pl0.fwd_train.arr[k].kind in (_lib.OP_CONV_FWD_AFFINE, _lib.OP_CONV_FWD)]
    n0 = C.create_string_buffer(128)
    for a, b in zip(conv, conv0):
        assert lib.ifcbk_op_kernel(C.byref(a), name, 128) == 0 and lib.ifcbk_op_kernel(C.byref(b), n0, 128) == 0 and name.value == n0.value


# ------------------------------------------------------------------------------------------------------ argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'resnet18', 'id'] + list(extra))


def test_flags():
    a = _parse()
    assert a.distill is None and a.distill_alpha == 0.5 and a.distill_temperature == 4.0
    a = _parse('--distill', 't.ptl', '--distill-alpha', '0.7', '--distill-temperature', '2', '--label-smoothing', '0.1', '--class-norm',
               '--weight-decay', '1e-4', '--ema', '0.99', '--flip', 'xy', '--rot90', '--jitter', '0.2', '--optimizer', 'SGD')
    assert (a.distill, a.distill_alpha, a.distill_temperature, a.label_smoothing) == ('t.ptl', 0.7, 2.0, 0.1)
    for bad in (['--distill-alpha', '-0.1'], ['--distill-alpha', '1.5'], ['--distill-alpha', 'nan'], ['--distill-temperature', '0'],
                ['--distill-temperature', '-1'], ['--distill-temperature', 'inf'], ['--distill-temperature', 'nan'], ['--distill-alpha', 'x']):
        with pytest.raises(SystemExit):
            _parse('--distill', 't.ptl', *bad)
    assert _parse('--distill', 't.ptl', '--distill-alpha', '0').distill_alpha == 0.0
    assert _parse('--distill', 't.ptl', '--distill-alpha', '1').distill_alpha == 1.0


@pytest.mark.parametrize('argv,flag', [(['--distill', 't.ptl', '--focal-gamma', '2'], '--focal-gamma'),
                                       (['--focal-gamma', '2', '--distill', 't.ptl'], '--focal-gamma'),
                                       (['--distill', 't.ptl', '--mixup', '0.4'], '--mixup'), (['--mixup', '0.4', '--distill', 't.ptl'], '--mixup'),
                                       (['--distill', 't.ptl', '--cutmix', '1'], '--cutmix'), (['--cutmix', '1', '--distill', 't.ptl'], '--cutmix')])
def test_exclusive_combinations_are_argparse_errors(argv, flag, capsys):
    with pytest.raises(SystemExit):
        _parse(*argv)
    assert '%s and --distill do not combine' % flag in capsys.readouterr().err
    _parse('--distill', 't.ptl', '--focal-gamma', '0', '--mixup', '0', '--cutmix', '0')            # 0 is off: no clash


# ------------------------------------------------------------------------------------------------------ class lists
def test_class_list_check_names_the_first_difference():
    chk = neuston_models.check_teacher_classes
    chk(['a', 'b', 'c'], ['a', 'b', 'c'])
    with pytest.raises(ValueError, match=r"class 1: 'x' \(teacher\) != 'b'"):
        chk(['a', 'b', 'c'], ['a', 'x', 'y'])
    with pytest.raises(ValueError, match=r"class 0: 'b' \(teacher\) != 'a'"):
        chk(['a', 'b', 'c'], ['b', 'c'])
    with pytest.raises(ValueError, match='teacher knows 2 classes, the training set has 3'):
        chk(['a', 'b', 'c'], ['a', 'b'])
    with pytest.raises(ValueError, match='teacher knows 4 classes, the training set has 3'):
        chk(['a', 'b', 'c'], ['a', 'b', 'c', 'd'])


# ------------------------------------------------------------------------------------------------------ hparams, .ptl
class _HostEngine(Engine):
    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_hparams_round_trip_old_checkpoints_and_the_missing_teacher(tmp_path):
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(distill=str(tmp_path / 'gone.ptl'), distill_alpha=0.7, distill_temperature=2.0,
                                                 distill_teacher_id='big', label_smoothing=0.1))
        assert m.distill == (0.7, 2.0) and m.model.engine.distill == (0.7, 2.0) and m.teacher is None
        assert isinstance(m.criterion, torch.nn.CrossEntropyLoss) and m.criterion.label_smoothing == pytest.approx(0.1)     # the hard criterion
        ck = m.checkpoint_dict()
        hp = ck['hyper_parameters']
        assert (hp['distill'], hp['distill_alpha'], hp['distill_temperature'], hp['distill_teacher_id']) == (str(tmp_path / 'gone.ptl'), 0.7, 2.0, 'big')
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        # the teacher file does not exist: loading the student never opens it
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path, inference=True)
        assert m2.distill == (0.7, 2.0) and m2.teacher is None
        # training without a teacher attached is an error, not a silent hard loss
        with pytest.raises(RuntimeError, match='no teacher is attached'):
            m2._need_teacher()
        # defaults of alpha and temperature when a file names a teacher only
        m4 = neuston_models.NeustonModel(_hparams(distill='t.ptl'))
        assert m4.distill == (0.5, 4.0)
        # a checkpoint without the keys: no distillation, no buffer
        for k in ('distill', 'distill_alpha', 'distill_temperature', 'distill_teacher_id'):
            del ck['hyper_parameters'][k]
        torch.save(ck, path)
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m3.distill is None and m3.model.engine.distill is None and not hasattr(m3.model.engine, 'teacher_logits')
        assert m3._need_teacher() is False
        with pytest.raises(RuntimeError, match='without distillation'):
            m3.attach_teacher(m2)
        for clash in (dict(focal_gamma=2.0), dict(mixup=0.4)):
            with pytest.raises(ValueError, match='distill'):
                neuston_models.NeustonModel(_hparams(distill='t.ptl', **clash))
        # a teacher with another class list is refused when it is attached
        other = neuston_models.NeustonModel(_hparams(classes=['a', 'x', 'c']))
        with pytest.raises(ValueError, match=r"class 1: 'x' \(teacher\) != 'b'"):
            m.attach_teacher(other)
        same = neuston_models.NeustonModel(_hparams(img_norm=['0.5', '0.25'], pad='border'))
        m.attach_teacher(same)
        assert m.teacher is same and m._teacher_load == dict(pad='border', mean=[0.5] * 3, std=[0.25] * 3)
        assert not [k for k in m.state_dict() if k.startswith('teacher')] and len(list(m.parameters())) == len(list(same.parameters()))
        kw = m._teacher_kw(dict(pixels=1, offs=2, hs=3, ws=4, max_h=5, max_w=6, in_channels=1, flips=7, turn=True, mean=[0] * 3, std=[1] * 3,
                                pad=128, jitter=(8, 9)))
        assert kw == dict(pixels=1, offs=2, hs=3, ws=4, max_h=5, max_w=6, in_channels=1, flips=7, turn=True, pad='border', mean=[0.5] * 3,
                          std=[0.25] * 3)


def test_defaults_leave_the_training_arguments_without_a_teacher():
    """what do_training does to the parsed arguments ahead of building the model"""
    src = open(os.path.join(os.path.dirname(HERE), 'ifcb_classifier_amd', 'neuston_net.py')).read()
    assert 'del args.distill, args.distill_alpha, args.distill_temperature' in src
    a = _parse()
    del a.distill, a.distill_alpha, a.distill_temperature
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(argparse.Namespace(**dict(vars(a), classes=['a', 'b'], model_id='m')))
    assert m.distill is None and not any(k.startswith('distill') for k in m.checkpoint_dict()['hyper_parameters'])
