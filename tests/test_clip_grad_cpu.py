"""TRAIN --clip-grad on the host: the flag's validation (CLI and Engine), the op tables Engine(plan_only=True) builds with clipping (one
optimizer op over the whole flat buffer, behind backward, carrying the clip state and the norm), the tables without it (unchanged), the
footprint audit of the clipped step, the agreement of header, export map and ctypes table on the new entry points, and the old entry
points as wrappers of the new ones.  The kernels run in tests/test_gpu_grad_clip.py, the engine in tests/test_gpu_clip_engine.py."""
import ctypes as C
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

import clip_cases as cc  # noqa: E402
import program_footprints as pf  # noqa: E402
from ifcb_classifier_amd import _lib, graph, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402

ROOT = os.path.dirname(HERE)
NORM = 0.75


# ------------------------------------------------------------------------------------------------------ the flag
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_cli_flag():
    assert _parse().clip_grad is None
    assert _parse('--clip-grad', '1.0').clip_grad == 1.0 and _parse('--clip-grad=0.5').clip_grad == 0.5
    for bad in ('0', '-1', '-0.5', 'nan', 'inf', '-inf', 'x', ''):
        with pytest.raises(SystemExit):
            _parse('--clip-grad=' + bad)
    act = [a for a in neuston_net.argparse_nn()._subparsers._group_actions[0].choices['TRAIN']._actions if a.dest == 'clip_grad'][0]
    assert act.help.startswith('(MI355X path, additive)') and 'clip_grad_norm_' in act.help and 'gradient_clip_val' in act.help
    # it composes with the other additive options
    a = _parse('--clip-grad', '2', '--optimizer', 'SGD', '--momentum', '0.9', '--weight-decay', '1e-4', '--ema', '0.99', '--mixup', '0.2')
    assert a.clip_grad == 2.0 and a.ema == 0.99 and a.optimizer == 'SGD'


@pytest.mark.parametrize('bad', [0.0, -1.0, float('nan'), float('inf'), 1e39])
def test_engine_refuses_a_norm_that_is_not_finite_and_positive(bad):
    with pytest.raises(ValueError, match='clip_grad'):
        Engine(graph.build('resnet18', 7), max_batch=2, plan_only=True, clip_grad=bad)


# ------------------------------------------------------------------------------------------------------ plans
def _plan(model, B=2, **kw):
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, keep, clear=True):
        eng = Engine(graph.build(model, 7), max_batch=B, plan_only=True, **kw)
        return eng, eng.plan(B)


CASES = [('inception_v3', 'adam', 0.0), ('inception_v3', 'sgd', 0.9), ('resnet18', 'adam', 0.0), ('resnet18', 'sgd', 0.9)]
_BUILT = {}


def _clip_plan(model, optimizer, momentum, ema=None):
    key = (model, optimizer, ema)
    if key not in _BUILT:
        _BUILT[key] = _plan(model, optimizer=optimizer, momentum=momentum, clip_grad=NORM, **({'ema_decay': ema} if ema else {}))
    return _BUILT[key]


def _opt_ops(eng, prog):
    kind = _lib.OP_SGD if eng.optimizer == 'sgd' else _lib.OP_ADAM
    return [(k, prog.arr[k]) for k in prog.find(kind)]


def _slots(optimizer):
    """(p slot of the average, p slot of the clip state, f slot of the norm)"""
    return (3, 4, 5) if optimizer == 'sgd' else (4, 5, 7)


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_the_clipped_step_holds_one_optimizer_op_over_the_whole_buffer(model, optimizer, momentum):
    eng, pl = _clip_plan(model, optimizer, momentum)
    assert eng.clip_grad == NORM and eng.clip_state.dtype == torch.float32 and eng.clip_state.data_ptr() % 16 == 0
    assert eng.clip_state.numel() == int(eng.ctx.lib.ifcbk_grad_clip_state_floats()) == 4 + 2 * cc.geometry(eng.ctx.lib)[0]
    es, cs, fs = _slots(optimizer)
    tables = []
    for name in ('step', 'adam', 'adam_pack'):
        ops = _opt_ops(eng, getattr(pl, name))
        assert len(ops) == 1, (name, len(ops))
        k, o = ops[0]
        assert int(o.i[0]) == eng.nparam_padded and o.p[0] == eng.P.data_ptr() and o.p[1] == eng.G.data_ptr() and o.p[2] == (
            eng.M.data_ptr() if (optimizer == 'adam' or momentum) else None)
        assert o.p[cs] == eng.clip_state.data_ptr() and o.f[fs] == C.c_float(NORM).value and not o.p[es]
        assert all(not o.p[j] for j in range(cs + 1, 12)) and (o.flags >> 8) & 7 == 0
        tables.append((o.kind, list(o.p), list(o.i), list(o.f)))
    assert tables[0] == tables[1] == tables[2]                      # the same op in all three (up to the step's wait bits)
    assert pl.step_adam_idxs == [pl.step_adam_idx] == [k for k, _o in _opt_ops(eng, pl.step)]
    # it sits behind every backward op: nothing that writes G follows it
    k_opt = pl.step_adam_idx
    assert all(not eng._op_param_offsets(pl.step.arr[k]) for k in range(k_opt + 1, pl.step.n))
    assert any(eng._op_param_offsets(pl.step.arr[k]) for k in range(k_opt))
    assert not _opt_ops(eng, pl.fwd_bwd) and not _opt_ops(eng, pl.bwd)
    # the cost counts the norm's pass over G
    fl, by = C.c_double(), C.c_double()
    o = pl.step.arr[k_opt]
    assert eng.ctx.lib.ifcbk_op_cost(C.byref(o), C.byref(fl), C.byref(by)) == 0
    base = (20 if momentum else 12) if optimizer == 'sgd' else 28
    assert by.value == float(eng.nparam_padded) * (base + 4)
    o2 = _lib.Op.from_buffer_copy(o)
    o2.p[cs] = None
    assert eng.ctx.lib.ifcbk_op_cost(C.byref(o2), C.byref(fl), C.byref(by)) == 0 and by.value == float(eng.nparam_padded) * base


@pytest.mark.parametrize('model,optimizer,momentum', CASES[2:])
def test_with_an_average_both_operands_ride_on_the_one_op(model, optimizer, momentum):
    eng, pl = _clip_plan(model, optimizer, momentum, ema=0.999)
    es, cs, fs = _slots(optimizer)
    for name in ('step', 'adam', 'adam_pack'):
        (k, o), = _opt_ops(eng, getattr(pl, name))
        assert o.p[es] == eng.E.data_ptr() and o.p[cs] == eng.clip_state.data_ptr() and o.f[fs] == C.c_float(NORM).value
        assert o.f[fs - 1] == 0.0                                  # the average's weight: stamped per step


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_without_the_flag_the_plan_is_the_default_plan(model, optimizer, momentum):
    eng0, pl0 = _plan(model, optimizer=optimizer, momentum=momentum)
    eng1, pl1 = _plan(model, optimizer=optimizer, momentum=momentum, clip_grad=None)
    assert eng1.clip_grad is None and eng1.clip_state is None
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    es, cs, fs = _slots(optimizer)
    for name in ('step', 'adam', 'adam_pack'):
        for k, o in _opt_ops(eng1, getattr(pl1, name)):
            assert not o.p[cs] and o.f[fs] == 0.0
    assert len(_opt_ops(eng1, pl1.step)) > 1                       # the bucketed update beside backward stays
    with pytest.raises(RuntimeError, match='without clip_grad'):
        eng1.grad_clip_stats()
    with pytest.raises(RuntimeError, match='without clip_grad'):
        eng1.reset_grad_clip_stats()
    # ... and the clipped plan differs from it in the optimizer ops only: same forward, loss and backward ops, in the same order
    eng2, pl2 = _clip_plan(model, optimizer, momentum)
    kind = _lib.OP_SGD if optimizer == 'sgd' else _lib.OP_ADAM
    rest = lambda p: [(p.arr[k].kind, p.tags[k]) for k in range(p.n) if p.arr[k].kind not in (kind, _lib.OP_WEIGHT_PACK_MULTI)]
    assert rest(pl2.step) == rest(pl0.step) and rest(pl2.fwd_bwd) == rest(pl0.fwd_bwd)


def _roles_with_clip():
    """program_footprints.ROLES with the two new slots: the average (as tests/test_ema_cpu.py) and the clip state, read and written,
    all of it (four figures and the partial sums)"""
    n4 = pf.bytes_(lambda o, e: o.i[0] * 4)
    state = pf.bytes_(lambda o, e: int(e.lib.ifcbk_grad_clip_state_floats()) * 4)
    adam, sgd = dict(pf.ROLES[_lib.OP_ADAM]), dict(pf.ROLES[_lib.OP_SGD])
    adam[4] = sgd[3] = (pf.RW, n4)
    adam[5] = sgd[4] = (pf.RW, state)
    return {_lib.OP_ADAM: adam, _lib.OP_SGD: sgd}


@pytest.mark.parametrize('model,optimizer,momentum', CASES)
def test_footprint_audit_of_the_clipped_programs(model, optimizer, momentum):
    eng, pl = _clip_plan(model, optimizer, momentum)
    with mock.patch.dict(pf.ROLES, _roles_with_clip()):
        for name in ('step', 'adam', 'adam_pack'):
            p = getattr(pl, name)
            assert not pf.unordered_conflicts(eng, p.arr, p.n, p.tags), name
            fps = [f for k, o in _opt_ops(eng, p) for f in pf.op_footprints(pf.allocations(eng), o, p.tags[k])]
            assert [f for f in fps if f[2][2] == 'clip_state' and f[1] == pf.RW], name          # the audit did see the state
            assert [f for f in fps if f[2][2] == 'G' and f[1] == pf.R and f[4] == 4 * eng.nparam_padded], name
        # negative control: with every wait of the step cleared the optimizer op, which reads all of G and writes all of P, is no
        # longer ordered behind the weight gradients and BatchNorm ops of the other lanes
        sched = [(ln, 0) for ln, _w in pf.frozen_sched(pl.step.arr, pl.step.n)]
        bad = pf.unordered_conflicts(eng, pl.step.arr, pl.step.n, pl.step.tags, sched=sched)
        assert bad
    # without the slot's role the audit refuses the op instead of skipping the pointer
    with pytest.raises(AssertionError, match='has no role'):
        pf.unordered_conflicts(eng, pl.adam.arr, pl.adam.n, pl.adam.tags)


# ------------------------------------------------------------------------------------------------------ the C interface
def _protos():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ifcbk.h')).read(), flags=re.S)
    return {m.group(2): (m.group(1), [a.strip() for a in m.group(3).split(',')])
            for m in re.finditer(r'IFCBK_API\s+(\w+)\s+(ifcbk_\w+)\s*\(([^;]*?)\)\s*;', hdr)}


def test_header_export_map_and_ctypes_table_agree_on_the_new_entry_points():
    protos = _protos()
    assert protos['ifcbk_grad_clip_state_floats'] == ('size_t', ['void'])
    assert protos['ifcbk_grad_norm'][1] == ['ifcbk_ctx*', 'const float* g', 'int64_t n', 'float grad_scale', 'float max_norm', 'float* state',
                                            'void* stream']
    old, new = protos['ifcbk_adam_ema_flat'][1], protos['ifcbk_adam_clip_flat'][1]
    assert new[:-1] == old[:-1] + ['float max_norm', 'float* clip_state'] and new[-1] == old[-1] == 'void* stream'
    old, new = protos['ifcbk_sgd_ema_flat'][1], protos['ifcbk_sgd_clip_flat'][1]
    assert new[:-1] == old[:-1] + ['float max_norm', 'float* clip_state'] and new[-1] == old[-1] == 'void* stream'
    for name in ('ifcbk_grad_norm', 'ifcbk_adam_clip_flat', 'ifcbk_sgd_clip_flat'):
        assert name in _lib.EXPORTS and len(_lib._PROTOS[name][1]) == len(protos[name][1]), name
    assert _lib._PROTOS['ifcbk_grad_clip_state_floats'] == (C.c_size_t, [])
    # the export map lets every ifcbk_ symbol out and nothing else; the built library has the four
    emap = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    assert 'global: ifcbk_*;' in emap and 'local: *;' in emap
    lib = _lib.load()
    for name in ('ifcbk_grad_clip_state_floats', 'ifcbk_grad_norm', 'ifcbk_adam_clip_flat', 'ifcbk_sgd_clip_flat'):
        assert getattr(lib, name)
    nf = int(lib.ifcbk_grad_clip_state_floats())
    assert nf > 4 and (nf - 4) % 2 == 0
    # the kernels' file is part of the build
    assert 'grad_clip.hip' in open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'Makefile')).read()


def test_the_old_entry_points_are_this_call():
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'pool_head.hip')).read()
    body = lambda name: re.search(r'extern "C" int %s\([^)]*\)\s*\{(.*?)\n\}' % name, src, flags=re.S).group(1).strip()
    assert re.fullmatch(r'return ifcbk_adam_clip_flat\(ctx, p, g, m, v, ema, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ema_w, '
                        r'0\.f, nullptr, stream\);', body('ifcbk_adam_ema_flat'))
    assert re.fullmatch(r'return ifcbk_adam_clip_flat\(ctx, p, g, m, v, nullptr, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, 0\.f, '
                        r'0\.f, nullptr, stream\);', body('ifcbk_adam_flat'))
    assert re.fullmatch(r'return ifcbk_sgd_clip_flat\(ctx, p, g, mom, ema, n, lr, momentum, weight_decay, grad_scale, ema_w, 0\.f, nullptr, '
                        r'stream\);', body('ifcbk_sgd_ema_flat'))
    assert re.fullmatch(r'return ifcbk_sgd_clip_flat\(ctx, p, g, mom, nullptr, n, lr, momentum, weight_decay, grad_scale, 0\.f, 0\.f, nullptr, '
                        r'stream\);', body('ifcbk_sgd_flat'))
    # one launch site per optimizer kernel: there is no second copy of the update for the clipped call
    assert src.count('hipLaunchKernelGGL(adam_kernel') == 1 and src.count('hipLaunchKernelGGL(sgd_kernel') == 1
    # run_one hands the operands over: p[5] / f[7] of IFCBK_OP_ADAM, p[4] / f[5] of IFCBK_OP_SGD
    ctx = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    # (by the slot names ctx.hip declares: the first enumerator of a row is slot 0)
    assert re.search(r'enum \{\s*// IFCBK_OP_ADAM\n\s*ADAM_P, ADAM_G, ADAM_M, ADAM_V, ADAM_E, ADAM_CLIP_STATE,', ctx)
    assert re.search(r'\n\s*ADAM_LR = 0, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, ADAM_WEIGHT_DECAY, ADAM_GRAD_SCALE, ADAM_EMA_W, ADAM_MAX_NORM\s', ctx)
    assert re.search(r'enum \{\s*// IFCBK_OP_SGD\n\s*SGD_P, SGD_G, SGD_M, SGD_E, SGD_CLIP_STATE,', ctx)
    assert re.search(r'\n\s*SGD_LR = 0, SGD_MOMENTUM, SGD_WEIGHT_DECAY, SGD_GRAD_SCALE, SGD_EMA_W, SGD_MAX_NORM\s', ctx)
    assert re.search(r'ifcbk_adam_clip_flat\(c,[^;]*\(float\*\)p\[ADAM_E\],[^;]*o->f\[ADAM_GRAD_SCALE\], o->f\[ADAM_EMA_W\], o->f\[ADAM_MAX_NORM\],\s*'
                     r'\(float\*\)p\[ADAM_CLIP_STATE\], st\);', ctx)
    assert re.search(r'ifcbk_sgd_clip_flat\(c,[^;]*\(float\*\)p\[SGD_E\],[^;]*o->f\[SGD_GRAD_SCALE\], o->f\[SGD_EMA_W\], o->f\[SGD_MAX_NORM\],\s*'
                     r'\(float\*\)p\[SGD_CLIP_STATE\], st\);', ctx)


# ------------------------------------------------------------------------------------------------------ the reference and the bound
def test_host_coef_is_torchs_formula():
    g = torch.randn(4099, generator=torch.Generator().manual_seed(2))
    for mx in (0.1, 1.0, 50.0, 1e4):
        total, (gc,) = cc.torch_clip([g], mx)
        coef = cc.host_coef(total, mx)
        assert torch.equal(gc, g * torch.tensor(coef)) and (float(coef) == 1.0) == (mx > total + 1e-6)
    assert float(cc.host_coef(float('inf'), 1.0)) == 0.0 and math.isnan(float(cc.host_coef(float('nan'), 1.0)))
    assert float(cc.host_coef(0.0, 1.0)) == 1.0


def test_the_bound_follows_the_chain_length():
    blocks = 1024
    per = blocks * cc.THREADS * 4
    assert [cc.chain(n, blocks) for n in (0, 3, 4, per - 4, per, per + 1, per + 4, 2 * per + 7)] == [0, 0, 1, 1, 1, 1, 2, 3]
    assert cc.norm_bound(per, blocks, 1.0) == pytest.approx((3.5 + 2) * cc.U, rel=1e-6)
    assert cc.norm_bound(0, blocks, 0.0) == 2.0 ** -149
