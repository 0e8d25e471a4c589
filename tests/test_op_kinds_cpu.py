"""The op-kind table, end to end (CPU): _lib numbers the kinds positionally, so the order of its tuple is tied here to the enum of
include/ifcbk.h; every kind but the retired one has a case in ctx.hip::run_one; and every kind is either emitted by a plan of one of the
model families or listed in EXEMPT_KINDS with the reason no plan carries it -- each of those that run_one still dispatches has a GPU
case in tests/test_gpu_program_runner.py (EXEMPT_CASES there), run alone through ifcbk_run_program against its typed entry point."""
import os
import re
from unittest import mock

import pytest
import torch

from ifcb_classifier_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED = 'IFCBK_OP_RETIRED_31'
PROGRAMS = ('step', 'fwd_eval', 'evalprep', 'pack', 'adam', 'adam_pack')
MODELS = ('inception_v3', 'resnet18', 'densenet121', 'vgg13_bn', 'alexnet', 'squeezenet')

# kind -> why none of the programs above, of any configuration below, carries it
EXEMPT_KINDS = {
    _lib.OP_WEIGHT_PACK: 'the plan builder\'s intermediate form: Engine._pack_multi folds the per-conv ops into one OP_WEIGHT_PACK_MULTI before a '
                         'program is frozen',
    _lib.OP_SOFTMAX: 'the one op of pl.softmax (probabilities behind an eval forward), which is none of the train / eval / pack programs',
    _lib.OP_MEMSET: 'a runner primitive for callers\' own programs (the delay op of tests/lane_order.py); the plans zero nothing by memset',
    _lib.OP_COPY2D: 'a runner primitive for callers\' own programs; the plans write concatenations in place and copy nothing',
    _lib.OP_DROPOUT_MASK: 'the masks are drawn by Engine.make_dropout_mask through the typed entry point, in front of the step: seed and call '
                          'count change every step and would have to be stamped into the table',
    _lib.OP_RETIRED_31: 'retired: the slot keeps the numbering, run_one has no case for it',
    _lib.OP_SOFTMAX_XENT_W: 'the loss kind of an engine with class weights (TRAIN --class-norm; tests/test_class_norm_cpu.py), which none of '
                            'the configurations here is',
}


def _sources():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    enum = re.sub(r'/\*.*?\*/', '', hdr[hdr.index('IFCBK_OP_CONV_FWD = 1'):hdr.index('typedef struct {\n    ifcbk_conv_desc d;')], flags=re.S)
    names = re.findall(r'IFCBK_OP_\w+', enum)
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    body = src[src.index('static int run_one('):src.index('// ---------------------------------------------------------------- program runner')]
    return names, body


def test_lib_numbers_the_kinds_as_the_header_does():
    names, _body = _sources()
    assert len(names) == len(set(names)) == 40 and names[0] == 'IFCBK_OP_CONV_FWD'
    # nothing in the enum but the first name carries an initialiser: position + 1 is the value
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    enum = hdr[hdr.index('IFCBK_OP_CONV_FWD = 1'):hdr.index('typedef struct {\n    ifcbk_conv_desc d;')]
    assert re.sub(r'/\*.*?\*/', '', enum, flags=re.S).count('=') == 1
    py = {v: k for k, v in vars(_lib).items() if k.startswith('OP_') and k != 'OP_NAMES' and isinstance(v, int)}
    assert sorted(py) == list(range(1, len(names) + 1)), 'an OP_* constant of _lib has no enum entry, or two share a number'
    for pos, name in enumerate(names):
        assert py[pos + 1] == name[len('IFCBK_'):], (pos + 1, name, py[pos + 1])          # the retired slot included: OP_RETIRED_31
    assert names.index(RETIRED) + 1 == _lib.OP_RETIRED_31 == 31
    assert len(_lib.OP_NAMES) == len(names) and sorted(_lib.OP_NAMES) == list(range(1, len(names) + 1))


def test_run_one_has_a_case_for_every_kind_but_the_retired_one():
    names, body = _sources()
    cases = re.findall(r'case (IFCBK_OP_\w+)\s*:', body)
    assert len(cases) == len(set(cases)), 'a kind with two cases'
    assert sorted(cases) == sorted(n for n in names if n != RETIRED), (sorted(set(names) - set(cases)), sorted(set(cases) - set(names)))
    assert RETIRED not in body
    assert re.search(r'default:\s*IFCBK_FAIL\(c, IFCBK_EINVAL, "run_program: unknown op kind %d", o->kind\);', body)


def _configs():
    for model in MODELS:
        for opt in ('adam', 'sgd'):
            yield model, opt, 2
    yield 'inception_v3', 'adam', 64          # grouped weight gradients start at batch 64 (tests/test_program_footprints_cpu.py)


@pytest.fixture(scope='module')
def emitted():
    """kind -> {(model, optimizer, input kind, program)} over every configuration"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    seen, u8 = {}, []
    with mock.patch.dict(os.environ, keep, clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):          # planning reads no tensor contents
        for model, opt, B in _configs():
            eng = Engine(graph.build(model, 7), max_batch=B, plan_only=True, optimizer=opt, momentum=0.9 if opt == 'sgd' else 0.0)
            kinds = ['nhwc'] + (['u8'] if eng.stem_u8 is not None else [])          # the plan depends on the input kind with a u8 stem only
            for kind in kinds:
                eng.in_kind[eng.in_slot] = kind
                pl = eng.plan(B)
                for prog in PROGRAMS:
                    p = getattr(pl, prog)
                    for k in range(p.n):
                        seen.setdefault(p.arr[k].kind, set()).add((model, opt, kind, prog))
            if len(kinds) == 2:
                u8.append(model)
    assert 'inception_v3' in u8
    return seen


def test_every_kind_is_emitted_by_a_plan_or_exempt_with_a_reason(emitted):
    names, body = _sources()
    every = set(range(1, len(names) + 1))
    assert set(emitted) <= every
    missing = sorted(every - set(emitted) - set(EXEMPT_KINDS))
    assert not missing, 'no plan emits %s and EXEMPT_KINDS does not say why' % [_lib.OP_NAMES[k] for k in missing]
    stale = sorted(set(EXEMPT_KINDS) & set(emitted))
    assert not stale, 'exempt, yet emitted: %s' % {k: sorted(emitted[k])[:1] for k in stale}
    assert all(isinstance(r, str) and len(r) > 20 for r in EXEMPT_KINDS.values())
    # both optimizers and both input kinds really were planned
    assert {c[1] for c in emitted[_lib.OP_SGD]} == {'sgd'} and {c[1] for c in emitted[_lib.OP_ADAM]} == {'adam'}
    assert {c[0] for c in emitted[_lib.OP_SGD]} == set(MODELS) == {c[0] for c in emitted[_lib.OP_ADAM]}
    assert emitted[_lib.OP_CONV_WGRAD_GROUP] and {c[3] for c in emitted[_lib.OP_CONV_WGRAD_GROUP]} == {'step'}
    assert {c[2] for c in emitted[_lib.OP_STEM_U8_FWD]} == {'u8'} and {c[2] for c in emitted[_lib.OP_STEM_U8_WGRAD]} == {'u8'}


def test_every_exempt_kind_that_run_one_dispatches_has_a_gpu_case():
    import importlib
    names, body = _sources()
    dispatched = {names.index(n) + 1 for n in re.findall(r'case (IFCBK_OP_\w+)\s*:', body)}
    runner = importlib.import_module('test_gpu_program_runner')
    # (the eval conv + max-pool fusion was exempt until the CPU planner emitted it; its stand-alone GPU case stays where it is)
    kept = {_lib.OP_CONV_FWD_AFFINE_MAXPOOL}
    assert kept <= set(runner.EXEMPT_CASES) and not kept & set(EXEMPT_KINDS)
    assert sorted(set(runner.EXEMPT_CASES) - kept) == sorted(set(EXEMPT_KINDS) & dispatched)
    assert _lib.OP_RETIRED_31 not in runner.EXEMPT_CASES
