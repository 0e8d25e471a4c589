"""TRAIN --ema on the host: the decay schedule, argument validation (Engine and CLI), the op tables Engine(plan_only=True) builds with a
weight average (every optimizer op of every program carries the slice of E that matches its slice of P), the footprint audit of those
programs, the oracle of tests/ema_bounds.py against torch's own EMA function, and the averaged view (Engine.ema_weights, the module's
state_dict(ema=True), the .ptl hyper-parameter) on host tensors.  The kernels run in tests/test_gpu_ema.py."""
import argparse
import math
import os
import re
import sys
from unittest import mock

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

import ema_bounds as eb  # noqa: E402
import program_footprints as pf  # noqa: E402
from ifcb_classifier_amd import _lib, engine, graph, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------------------ the schedule
def test_schedule_warms_up_from_2_11ths_and_caps_at_decay():
    assert engine.ema_decay_at(0.999, 1) == 2.0 / 11.0 == eb.decay_at(0.999, 1)
    assert engine.ema_decay_at(0.999, 2) == 3.0 / 12.0
    prev = 0.0
    for t in range(1, 20000):
        d = engine.ema_decay_at(0.999, t)
        assert d == eb.decay_at(0.999, t) == min(0.999, (1.0 + t) / (10.0 + t)) and prev <= d <= 0.999
        prev = d
    # (1 + t) / (10 + t) >= 0.999  <=>  0.001 t >= 8.99  <=>  t >= 8990
    assert engine.ema_decay_at(0.999, 8989) < 0.999 and engine.ema_decay_at(0.999, 8991) == 0.999 == engine.ema_decay_at(0.999, 10 ** 9)
    assert engine.ema_decay_at(0.1, 1) == 0.1                       # a decay below the warm-up's first value is never raised
    for t in (1, 2, 100, 10 ** 6):
        assert engine.ema_decay_at(0.9, t, warmup=False) == 0.9 == eb.decay_at(0.9, t, False)


def test_the_weight_is_one_minus_decay_in_double_rounded_once():
    for decay in (0.5, 0.9, 0.999, 0.9999):
        for t in (1, 3, 50, 10 ** 5):
            for warm in (True, False):
                w = engine.ema_weight(decay, t, warm)
                assert w == eb.weight(decay, t, warm) == float(torch.tensor(1.0 - eb.decay_at(decay, t, warm), dtype=torch.float64).float())
    # not 1 - fl32(d): for d = 0.9999 the two differ by far more than an ulp of w
    assert engine.ema_weight(0.9999, 10 ** 6) != 1.0 - eb.f32(0.9999)
    assert abs(engine.ema_weight(0.9999, 10 ** 6) - 1e-4) < 1e-4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------ argument validation
def _plan(model, B=2, env=None, **kw):
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, dict(keep, **(env or {})), clear=True):
        eng = Engine(graph.build(model, 7), max_batch=B, plan_only=True, **kw)
        return eng, eng.plan(B)


@pytest.mark.parametrize('bad', [0.0, 1.0, -0.1, 1.5, float('nan'), float('inf')])
def test_engine_refuses_a_decay_outside_the_open_unit_interval(bad):
    with pytest.raises(ValueError, match='ema_decay'):
        Engine(graph.build('resnet18', 7), max_batch=2, plan_only=True, ema_decay=bad)


def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_cli_flag():
    assert _parse().ema is None
    assert _parse('--ema', '0.9').ema == 0.9 and _parse('--ema=0.9999').ema == 0.9999
    for bad in ('1.5', '0', '1', '-0.5', 'nan', 'inf', 'x'):
        with pytest.raises(SystemExit):
            _parse('--ema=' + bad)
    help_text = [a for a in neuston_net.argparse_nn()._subparsers._group_actions[0].choices['TRAIN']._actions if a.dest == 'ema'][0].help
    assert help_text.startswith('(MI355X path, additive)')


# ------------------------------------------------------------------------------------------------------ plans
CASES = [('inception_v3', 'adam', 0.0), ('inception_v3', 'sgd', 0.9), ('resnet18', 'adam', 0.0), ('resnet18', 'sgd', 0.9)]
_BUILT = {}


def _ema_plan(model, optimizer, momentum):
    key = (model, optimizer)
    if key not in _BUILT:
        _BUILT[key] = _plan(model, optimizer=optimizer, momentum=momentum, ema_decay=0.999)
    return _BUILT[key]


def _opt_ops(eng, prog):
    kind = _lib.OP_SGD if eng.optimizer == 'sgd' else _lib.OP_ADAM
    return [(k, prog.arr[k]) for k in prog.find(kind)]


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_every_optimizer_op_carries_the_slice_of_E_that_matches_its_slice_of_P(model, optimizer, momentum):
    eng, pl = _ema_plan(model, optimizer, momentum)
    assert eng.E.shape == eng.P.shape and eng.E.dtype == torch.float32 and eng.ERB.shape == eng.RB.shape
    slot, fslot = (3, 4) if optimizer == 'sgd' else (4, 6)
    P0, E0, n = eng.P.data_ptr(), eng.E.data_ptr(), eng.nparam_padded
    carried = 0
    for name in mpf.PROGRAMS + ('adam_pack', 'fwd_bwd'):
        prog = getattr(pl, name)
        ops = _opt_ops(eng, prog)
        if name in ('step', 'adam', 'adam_pack'):
            assert ops, name
        spans = []
        for k, o in ops:
            off = o.p[0] - P0
            assert off >= 0 and off % 16 == 0 and o.p[slot] == E0 + off, (name, k)
            assert o.p[1] == eng.G.data_ptr() + off and o.p[2] == eng.M.data_ptr() + off
            assert all(not o.p[j] for j in range(slot + 1, 12)), (name, k)
            assert o.f[fslot] == 0.0                       # stamped per step (_set_update)
            spans.append((off // 4, off // 4 + int(o.i[0])))
            carried += 1
        if ops:                                            # the slices tile E exactly once
            spans.sort()
            assert spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (name, spans)
    assert len(_opt_ops(eng, pl.step)) > 1 and carried >= len(_opt_ops(eng, pl.step)) + 2          # several buckets, adam, adam_pack
    # the lane annotation of a bucket's op names its slice of E among the writes: it sits on the weight-gradient lane
    lanes = {(o.flags >> 8) & 7 for _k, o in _opt_ops(eng, pl.step)}
    assert len(lanes) == 2 and 0 in lanes


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_op_cost_counts_8_bytes_per_element_for_the_average(model, optimizer, momentum):
    import ctypes as C
    eng, pl = _ema_plan(model, optimizer, momentum)
    slot = 3 if optimizer == 'sgd' else 4
    base = 20 if optimizer == 'sgd' else 28
    for k, o in _opt_ops(eng, pl.step):
        fl, by = C.c_double(), C.c_double()
        assert eng.ctx.lib.ifcbk_op_cost(C.byref(o), C.byref(fl), C.byref(by)) == 0
        assert by.value == float(o.i[0]) * (base + 8)
        o2 = _lib.Op.from_buffer_copy(o)
        o2.p[slot] = None
        assert eng.ctx.lib.ifcbk_op_cost(C.byref(o2), C.byref(fl), C.byref(by)) == 0
        assert by.value == float(o.i[0]) * base


def _roles_with_ema():
    """program_footprints.ROLES with the average's slot: read and written, the extent of P's"""
    n4 = pf.bytes_(lambda o, e: o.i[0] * 4)
    adam, sgd = dict(pf.ROLES[_lib.OP_ADAM]), dict(pf.ROLES[_lib.OP_SGD])
    adam[4] = sgd[3] = (pf.RW, n4)
    return {_lib.OP_ADAM: adam, _lib.OP_SGD: sgd}


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_footprint_audit_finds_no_unordered_conflict_and_names_one_when_the_waits_are_cleared(model, optimizer, momentum):
    eng, pl = _ema_plan(model, optimizer, momentum)
    with mock.patch.dict(pf.ROLES, _roles_with_ema()):
        for name in ('step', 'adam', 'adam_pack'):
            p = getattr(pl, name)
            assert not pf.unordered_conflicts(eng, p.arr, p.n, p.tags), name
            fps = [f for k, o in _opt_ops(eng, p) for f in pf.op_footprints(pf.allocations(eng), o, p.tags[k])]
            assert [f for f in fps if f[2][2] == 'E' and f[1] == pf.RW], name          # the audit did see the average
        # negative control: the waits of the optimizer ops' lane are cleared.  A bucket's op sits on the weight-gradient lane behind the
        # weight gradients that complete the bucket, and the frozen table gives it no wait bit of its own: what it has to wait for, its
        # lane already waited for (schedule_lanes skips implied waits).  So the mutation clears the wait masks of that lane's ops and of
        # the optimizer ops: the lane then runs free of the chains, and its optimizer ops write P (and E) while BatchNorm ops on the
        # chain lanes still read their slices of P
        sched = pf.frozen_sched(pl.step.arr, pl.step.n)
        opt_idx = [k for k, _o in _opt_ops(eng, pl.step)]
        lw = {sched[k][0] for k in opt_idx} - {0}
        assert len(lw) == 1
        cleared = 0
        for k in range(pl.step.n):
            if (sched[k][0] in lw or k in opt_idx) and sched[k][1]:
                sched[k] = (sched[k][0], 0)
                cleared += 1
        assert cleared
        bad = pf.unordered_conflicts(eng, pl.step.arr, pl.step.n, pl.step.tags, sched=sched)
        kind = 'sgd' if optimizer == 'sgd' else 'adam'
        assert [b for b in bad if b[2] in ('E', 'P') and kind in (b[0][1], b[1][1])], bad[:6]
    # without the slot's role the audit refuses the op instead of skipping the pointer
    with pytest.raises(AssertionError, match='has no role'):
        pf.unordered_conflicts(eng, pl.adam.arr, pl.adam.n, pl.adam.tags)


def test_the_new_operand_is_not_const_in_the_typed_entry_points():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ifcbk.h')).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'IFCBK_API\s+int\s+(ifcbk_\w+)\s*\(([^;]*?)\)\s*;', hdr)}
    old, new = protos['ifcbk_adam_flat'], protos['ifcbk_adam_ema_flat']
    assert new[:5] + new[6:14] + new[15:] == old and new[5] == 'float* ema' and new[14] == 'float ema_w'
    old, new = protos['ifcbk_sgd_flat'], protos['ifcbk_sgd_ema_flat']
    assert new[:4] + new[5:10] + new[11:] == old and new[4] == 'float* ema' and new[10] == 'float ema_w'
    assert protos['ifcbk_ema_flat'] == ['ifcbk_ctx*', 'float* e', 'const float* x', 'int64_t n', 'float w', 'void* stream']
    assert len(_lib._PROTOS['ifcbk_adam_ema_flat'][1]) == len(protos['ifcbk_adam_ema_flat'])
    assert len(_lib._PROTOS['ifcbk_sgd_ema_flat'][1]) == len(protos['ifcbk_sgd_ema_flat'])
    assert len(_lib._PROTOS['ifcbk_ema_flat'][1]) == len(protos['ifcbk_ema_flat'])
    # run_one hands the operand over: p[4] / f[6] of IFCBK_OP_ADAM, p[3] / f[4] of IFCBK_OP_SGD
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    # (by the slot names ctx.hip declares, the first enumerator of a row being slot 0; through the clipping entry point, which a NULL
    # clip state makes the _ema_flat call)
    assert re.search(r'enum \{\s*// IFCBK_OP_ADAM\n\s*ADAM_P, ADAM_G, ADAM_M, ADAM_V, ADAM_E,', src)
    assert re.search(r'\n\s*ADAM_LR = 0, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ADAM_WEIGHT_DECAY, ADAM_GRAD_SCALE, ADAM_EMA_W,', src)
    assert re.search(r'enum \{\s*// IFCBK_OP_SGD\n\s*SGD_P, SGD_G, SGD_M, SGD_E,', src)
    assert re.search(r'\n\s*SGD_LR = 0, SGD_MOMENTUM, SGD_WEIGHT_DECAY, SGD_GRAD_SCALE, SGD_EMA_W,', src)
    assert re.search(r'ifcbk_adam_clip_flat\(c,[^;]*\(float\*\)p\[ADAM_E\],[^;]*o->f\[ADAM_GRAD_SCALE\], o->f\[ADAM_EMA_W\],', src)
    assert re.search(r'ifcbk_sgd_clip_flat\(c,[^;]*\(float\*\)p\[SGD_E\],[^;]*o->f\[SGD_GRAD_SCALE\], o->f\[SGD_EMA_W\],', src)


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_without_a_decay_the_plan_is_the_default_plan(model, optimizer, momentum):
    eng0, pl0 = _plan(model, optimizer=optimizer, momentum=momentum)
    eng1, pl1 = _plan(model, optimizer=optimizer, momentum=momentum, ema_decay=None, ema_warmup=True)
    assert eng1.E is None and eng1.ERB is None and eng1.ema_decay is None
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    for name in ('step', 'adam', 'adam_pack'):
        for k, o in _opt_ops(eng1, getattr(pl1, name)):
            assert not o.p[3 if optimizer == 'sgd' else 4] and o.f[4 if optimizer == 'sgd' else 6] == 0.0
    with pytest.raises(RuntimeError, match='without ema_decay'):
        with eng1.ema_weights():
            pass


# ------------------------------------------------------------------------------------------------------ the oracle against torch
def test_oracle_agrees_with_torch_swa_utils():
    fn = getattr(torch.optim.swa_utils, 'get_ema_multi_avg_fn', None)
    if fn is None:
        return                                   # an older torch: nothing to compare with (the oracle stands on its derivation)
    g = torch.Generator().manual_seed(5)
    for decay in (0.9, 0.999, 0.9999, 2.0 / 11.0 + 0.5):
        for scale in (1e-3, 1.0, 300.0):
            e = torch.randn(4099, generator=g) * scale
            p = e + torch.randn(4099, generator=g) * scale * 0.01
            p[:7] = e[:7]                                                # fixed points
            got = e.clone()
            fn(decay)([got], [p.clone()], 10)
            w = eb.f32(1.0 - decay)
            if w < 0.5:                          # (torch.lerp takes another formula from weight 0.5 on)
                eb.check('swa_utils %g %g' % (decay, scale), got, e, p, w)
            assert torch.equal(got[:7], e[:7])


def test_the_lerp_form_has_p_as_its_fixed_point_and_the_two_scalar_form_has_not():
    """d e + (1 - d) p with fl32(d) and fl32(1 - d) settles at p fl(1 - d) / (1 - fl(d)), which is not p; e + w (p - e) stays at p"""
    d = 0.9999
    fd, fw = eb.f32(d), eb.f32(1.0 - d)
    assert abs(fw / (1.0 - fd) - 1.0) > 1e-5                    # the two-scalar form's fixed point, relative to p
    p = torch.full((1000,), 3.0) + torch.arange(1000) * 1e-3
    w = eb.weight(d, 10 ** 6)
    lerp = p + torch.tensor(w) * (p - p)
    assert torch.equal(lerp, p)
    assert eb.check('lerp', lerp, p, p, w) == 0.0
    assert math.isclose(float(eb.bound(torch.tensor([1.0]), torch.tensor([1.0]), 0.5)), eb.U, rel_tol=1e-6)
    # the bound tells a wrong weight: an update with fl32(1 - fl32(d)) in the place of w is outside it
    e = torch.zeros(1000)
    wrong = (e.double() + (1.0 - fd) * (p.double() - e.double())).float()
    assert bool(((wrong.double() - eb.update(e, p, w)).abs() > eb.bound(e, p, w)).all())


# ------------------------------------------------------------------------------------------------------ the averaged view, on the host
class _HostEngine(Engine):
    """the engine NeustonModel builds, without a device: parameters, views and optimizer state live on the host"""

    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_ema_weights_shows_the_average_and_puts_every_bit_back(tmp_path):
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(ema=0.9))
        eng = m.model.engine
        assert m.ema == 0.9 and eng.ema_decay == 0.9 and eng.ema_warmup and eng.ema_stale
        # stale (nothing averaged since init_weights): the average of the model is the model
        raw = {k: v.clone() for k, v in m.model.state_dict().items()}
        avg = m.model.state_dict(ema=True)
        assert not eng.ema_stale and eng.ema_updates == 0
        assert sorted(avg) == sorted(raw) and all(torch.equal(avg[k], raw[k]) for k in raw)
        # an average that differs
        g = torch.Generator().manual_seed(3)
        eng.E.copy_(torch.randn(eng.E.shape, generator=g))
        eng.ERB.copy_(torch.rand(eng.ERB.shape, generator=g) + 0.5)
        eng.M.copy_(torch.randn(eng.M.shape, generator=g))
        eng.nbt += 3
        eng.step_count, eng.packed, eng.eval_stats_ready = 7, True, True
        P0, RB0, M0, E0, ERB0 = eng.P.clone(), eng.RB.clone(), eng.M.clone(), eng.E.clone(), eng.ERB.clone()
        with eng.ema_weights() as inside:
            assert inside is eng and torch.equal(eng.P, E0) and torch.equal(eng.RB, ERB0)
            assert not eng.packed and not eng.eval_stats_ready
            eng.packed = eng.eval_stats_ready = True               # (what an eval forward inside leaves)
            eng.params_changed()                                    # (what the module's eval forward calls)
            with pytest.raises(RuntimeError, match='inside ema_weights'):
                eng._ema_begin_step()
            with pytest.raises(RuntimeError, match='already inside'):
                with eng.ema_weights():
                    pass
            view = {k: v.clone() for k, v in m.model.state_dict().items()}
        assert torch.equal(eng.P, P0) and torch.equal(eng.RB, RB0) and torch.equal(eng.M, M0) and eng.step_count == 7
        assert torch.equal(eng.E, E0) and torch.equal(eng.ERB, ERB0)
        assert not eng.packed and not eng.eval_stats_ready and not eng.ema_stale
        avg = m.model.state_dict(ema=True)
        assert all(torch.equal(avg[k], view[k]) for k in view)
        key = next(k for k in avg if k.endswith('conv1.weight'))
        o, n, shape, kind, node = eng.poff[key]
        assert torch.equal(avg[key], E0[o:o + n].view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2))
        assert not torch.equal(avg[key], m.model.state_dict()[key])
        rk = next(k for k in avg if k.endswith('running_var'))
        assert torch.equal(avg[rk], ERB0[eng.boff[rk][0]:eng.boff[rk][0] + eng.boff[rk][1]])
        nk = next(k for k in avg if k.endswith('num_batches_tracked'))
        assert int(avg[nk]) == 3                                    # the live count
        # the copies do not alias the engine's buffers
        avg[key].zero_()
        assert torch.equal(eng.E, E0) and torch.equal(eng.P, P0)
        # a write from outside restarts the average
        eng.init_weights(5)
        assert eng.ema_stale
        # the hyper-parameter travels in the file; a file without the key means off
        ck = m.checkpoint_dict(epoch=1, global_step=2)
        assert ck['hyper_parameters']['ema'] == 0.9
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.ema == 0.9 and m2.model.engine.ema_decay == 0.9
        plain = neuston_models.NeustonModel(_hparams())
        assert plain.ema is None and plain.model.engine.ema_decay is None and plain.model.engine.E is None
        with pytest.raises(RuntimeError, match='without ema_decay'):
            plain.model.state_dict(ema=True)
        with pytest.raises(ValueError, match='ema_decay'):
            neuston_models.NeustonModel(_hparams(ema=1.5))
