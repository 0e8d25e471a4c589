"""The plan of a batch N does not depend on the capacity of the engine that builds it (CPU, Engine(plan_only=True)).

tests/test_gpu_engine_life.py holds a long-lived engine of capacity B that runs a partial batch N to the raw bits of a fresh engine of
capacity N.  That bound is only right if both run the same program: the same op kinds, flags with lane and wait bits, descriptors,
scalars, kernel names and symbolic pointers.  In plan.PlanBuilder, max_batch and train_batch enter buffer sizes only, and the library
compares the reserved workspace with what a launch needs, never picks a kernel from it; here that is checked, not assumed."""
import os
from unittest import mock

import pytest

import engine_life as el

CASES = [(f, el.FAMILIES[f][1], n, dt) for f in el.FAMILIES for n in el.PARTIAL[f] for dt in el.DTYPES]


def test_the_cases_are_the_ones_the_gpu_file_uses():
    assert sorted({'%s-%d' % (f, n) for f, _b, n, _dt in CASES}) == sorted(el.PAIRS)
    assert {dt for _f, _b, _n, dt in CASES} == {'bf16', 'fp32'}
    for f, (_name, B, _S) in el.FAMILIES.items():
        assert B - 1 in el.PARTIAL[f] and 2 in el.PARTIAL[f] and 1 in el.PARTIAL[f] and max(el.PARTIAL[f]) < B
    assert 3 in el.PARTIAL['inception_v3'] and el.FAMILIES['resnet18'][1] - 1 & 1


@pytest.mark.parametrize('family,B,N,dtype', CASES)
def test_plan_text_is_the_same_at_every_capacity(family, B, N, dtype):
    """make_plan_fingerprints.plan_text of plan(N) on a max_batch=B engine equals that on a max_batch=N engine.

    One field is normalised, and only that one: a d(raw) tensor carved from the engine's pooled allocation appears as
    '_draw_pool+<byte offset>', and the offset is the sum of the earlier carves' sizes, which hold train_batch (Engine._carve).
    engine_life.capacity_free rewrites it as '<carved tensor>+<offset inside the carve>'.  The raw texts are required to differ in
    nothing but lines that name the pool, and squeezenet1_1 (no BatchNorm, no pool) must be equal without any rewriting."""
    name = el.FAMILIES[family][0]
    raw_b, free_b = el.plan_only_text(name, B, N, dtype)
    raw_n, free_n = el.plan_only_text(name, N, N, dtype)
    assert free_b == free_n, [(x, y) for x, y in zip(free_b.splitlines(), free_n.splitlines()) if x != y][:3]
    lb, ln = raw_b.splitlines(), raw_n.splitlines()
    assert len(lb) == len(ln) > 100
    differ = [(x, y) for x, y in zip(lb, ln) if x != y]
    assert all('_draw_pool+' in x and '_draw_pool+' in y for x, y in differ), differ[:3]
    assert '_draw_pool+' not in free_b                       # every pool pointer was resolved to a carve
    if family == 'squeezenet1_1':
        assert raw_b == raw_n
    else:
        assert differ                                        # the normalisation is not vacuous


@pytest.mark.parametrize('name,B', [('resnet18', 8), ('resnet18', 6), ('inception_v3', 6), ('squeezenet', 4)])
def test_scratch_of_a_capacity_holds_every_smaller_batch(name, B):
    """The scratch an engine allocates once must hold what the plan of EVERY batch up to its capacity asks for, read back here from
    the op tables with the library's own sizing functions.  Neither size is monotonic in the batch (the kernel, and with it the
    number of partial rows and the split-K depth, follows the batch): sized for the capacity alone, resnet18 at capacity 8 had
    100,352 floats of partial sums for the 125,440 a step at batch 5 writes, and 12,142,592 bytes of workspace for the 12,544,000
    a step at batch 7 asks for -- the first an out-of-bounds write, the second a refused step (found by
    tests/test_gpu_engine_life.py on the partial batch 7)."""
    import ctypes as C
    import torch
    from ifcb_classifier_amd import _lib, graph
    from ifcb_classifier_amd.engine import Engine
    reserved = []
    with mock.patch.object(torch, 'zeros', torch.empty), mock.patch.object(torch, 'zeros_like', torch.empty_like), \
            mock.patch.object(_lib.PlanOnlyContext, 'reserve', lambda self, nbytes: reserved.append(int(nbytes))):
        eng = Engine(graph.build(name, el.NC, pretrained=False), max_batch=B, plan_only=True)
        plans = {N: eng.plan(N) for N in range(1, B + 1)}
    assert len(reserved) == 1
    lib, part = eng.ctx.lib, eng.bn_part[0].numel()
    spans = [(t.data_ptr(), t.data_ptr() + 4 * part) for t in eng.bn_part]
    seen = set()
    for N, pl in plans.items():
        for k in range(pl.step.n):
            o = pl.step.arr[k]
            d = o.u.conv
            if o.kind in (_lib.OP_CONV_WGRAD, _lib.OP_CONV_WGRAD_SEG):
                assert lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)) <= reserved[0], (N, pl.step.tags[k])
            elif not any(o.p[j] and a <= o.p[j] < b for j in range(12) for a, b in spans):
                continue                                     # no operand in a partial-sum buffer
            elif o.kind == _lib.OP_CONV_FWD:
                assert lib.ifcbk_conv2d_fwd_mblocks(C.byref(d)) * 2 * d.K <= part, (N, pl.step.tags[k])
            elif o.kind == _lib.OP_CONV_DGRAD_BNSTAT:
                assert lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(d)) * 2 * d.C <= part, (N, pl.step.tags[k])
            elif o.kind == _lib.OP_BN_STATS:
                assert lib.ifcbk_bn_stats_rows(o.u.bn.M) * 2 * o.u.bn.C <= part, (N, pl.step.tags[k])
            else:
                continue
            seen.add(o.kind)
    if name != 'squeezenet':                                 # (no BatchNorm: no partial sums, and its weight gradients ask for no workspace)
        assert {_lib.OP_CONV_FWD, _lib.OP_CONV_WGRAD, _lib.OP_CONV_DGRAD_BNSTAT} <= seen


def test_the_eval_graph_switch_is_read_once_at_construction():
    """IFCBK_GRAPH decides graph_eval when the engine is built and is not read again: the GPU scenarios that run 'with IFCBK_GRAPH=0'
    flip that attribute on the long-lived engine instead of building another one"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    env = {k: v for k, v in os.environ.items() if k != 'IFCBK_GRAPH'}
    with mock.patch.dict(os.environ, env, clear=True):
        on = Engine(graph.build('resnet18', el.NC, pretrained=False), max_batch=1, plan_only=True)
    with mock.patch.dict(os.environ, dict(env, IFCBK_GRAPH='0'), clear=True):
        off = Engine(graph.build('resnet18', el.NC, pretrained=False), max_batch=1, plan_only=True)
        assert on.graph_eval and not off.graph_eval and not on.graph_train and not off.graph_train
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ifcb_classifier_amd', 'engine.py')).read()
    assert src.count("os.environ.get('IFCBK_GRAPH'") == 1
