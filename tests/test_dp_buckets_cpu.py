"""The data-parallel bucket plan against the memory the backward ops really write (tests/dp_twin.py; Engine(plan_only=True), no GPU).

Engine.train_step_ddp hands the tail bucket [lo, hi) of the flat gradient buffer G to the all-reduce right behind the backward segment
that Engine._op_param_offsets -- a hand-kept table over the op kinds -- says finishes it.  With one rank the exchange changes nothing
and a bucket handed over early still ends with the right bits, so the GPU runs at world 1 cannot see an error in that table, and
tests/test_dp_gloo.py fills the buffer with the same table it plans with.  Here the writes come from the op table alone
(program_footprints.op_footprints: pointers, descriptors and the accumulate bits), for every family, both lane counts and both
storage types:

* the segments partition the backward list in order and their buckets tile [0, nparam_padded) from the tail;
* no op of a later segment writes or accumulates into an element that was handed over (what the overlap rests on);
* every element of every parameter tensor of a bucket is written by the segments up to its own -- except the conv biases in front of a
  BatchNorm (Engine.cbias_after), which nothing writes: their gradient is identically zero;
* no op writes the alignment padding between two tensors (zero from allocation; the exchange and the optimizer's flat launch read it);
* the first write to an element within a step is a plain write, not an accumulating one (else a step adds to the last step's SUMMED
  gradient);
* the table names, for every op, exactly the tensors that op writes.

Negative controls mutate a copy of the segment list / of the table and must be reported by op and bucket."""
import contextlib
import os
from unittest import mock

import pytest

import dp_twin as dt
from ifcb_classifier_amd import _lib

NC = 7
#  family x world, bf16; fp32 for one residual and one conv-bias + BatchNorm family
MATRIX = [(name, w, 'bf16', 2) for name in dt.FAMILIES for w in (1, 2)] + [(name, w, 'fp32', 2) for name in ('resnet18', 'vgg13_bn') for w in (1, 2)]
# grouped weight gradients (OP_CONV_WGRAD_GROUP: another row of the table) exist from batch 64 on
MATRIX.append(('inception_v3', 2, 'bf16', 64))
_PLANS = {}


def _plan(name, w, dtype, B):
    key = (name, w, dtype, B)
    if key not in _PLANS:
        import torch
        from ifcb_classifier_amd import graph
        from ifcb_classifier_amd.engine import Engine
        keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
        # (batch 64: planning reads no tensor contents; empty() keeps the host buffers untouched, as tests/test_program_footprints_cpu.py)
        cheap = [mock.patch.object(torch, 'zeros', torch.empty), mock.patch.object(torch, 'zeros_like', torch.empty_like)] if B >= 64 else []
        with mock.patch.dict(os.environ, keep, clear=True), contextlib.ExitStack() as stack:
            for c in cheap:
                stack.enter_context(c)
            eng = Engine(graph.build(name, NC), max_batch=B, plan_only=True, dp_world=w, dtype=dtype)
            pl = eng.plan(B)
        assert eng.dp_world == w and eng.NL == (2 if w > 1 else 4)
        segs = dt.plain_segments(eng.ddp_segments(pl))
        _PLANS[key] = (eng, pl, segs, dt.g_writes(eng, pl.bwd_list))
    return _PLANS[key]


@pytest.mark.parametrize('name,w,dtype,B', MATRIX, ids=lambda v: str(v))
def test_the_bucket_plan_holds_against_the_ops_own_writes(name, w, dtype, B):
    eng, pl, segs, writes = _plan(name, w, dtype, B)
    bwd = pl.bwd_list
    bad = dt.audit(eng, bwd, segs, dt.table_offsets(eng, bwd), writes)
    assert not bad, (name, w, dtype, len(bad), bad[:6])
    # the audit saw something: several buckets, every parameter tensor written, and ops of every kind the table knows that this plan has
    assert len(segs) >= 4 and sum(1 for wr in writes if wr) >= len(segs)
    nwritten = len({a for wr in writes for a, _b, _acc in wr})
    dead = sorted(o for lst in eng.cbias_after.values() for o in lst)
    assert nwritten == len(eng.poff) - len(dead), (nwritten, len(eng.poff), len(dead))
    # the conv biases in front of a BatchNorm: there for vgg*_bn, nowhere else
    assert bool(dead) == (name == 'vgg13_bn'), (name, dead)
    if dead:
        assert all(eng.poff[k][3] == 'bn_cbias' for k in eng.poff if eng.poff[k][0] in dead) and len(dead) == 10
    if B >= 64:
        assert any(o.kind == _lib.OP_CONV_WGRAD_GROUP for o in bwd.ops)


def test_the_segments_do_not_depend_on_the_lane_count():
    """world 2 builds another program (2 lanes, not 4); the order of the backward list, and with it the buckets, is the same"""
    for name in dt.FAMILIES:
        a, b = _plan(name, 1, 'bf16', 2), _plan(name, 2, 'bf16', 2)
        assert a[2] == b[2] and a[1].bwd_list.tags == b[1].bwd_list.tags, name
        lanes = lambda pl: {(pl.step.arr[k].flags >> 8) & 7 for k in range(pl.step.n)}
        assert max(lanes(b[1])) <= 1 and (name in ('alexnet', 'vgg11', 'vgg13_bn') or max(lanes(a[1])) >= 2), name


@pytest.mark.parametrize('name', ['inception_v3', 'resnet18', 'vgg13_bn'])
def test_control_a_cut_moved_one_op_early_is_named(name):
    """the cut behind a segment whose last op writes G moves one op earlier: that op now runs behind the bucket's hand-over"""
    eng, pl, segs, writes = _plan(name, 2, 'bf16', 2)
    bwd = pl.bwd_list
    moved, i, k = dt.move_cut_early(segs, writes)
    bad = dt.audit(eng, bwd, moved, dt.table_offsets(eng, bwd), writes)
    late = [b for b in bad if b[0] == 'late write']
    assert late and {(b[1], b[2], b[3]) for b in late} == {(bwd.tags[k], _lib.OP_NAMES[bwd.ops[k].kind], segs[i][2:])}, bad
    # ... and the tensor that segment i no longer finishes is reported as uncovered, in the same bucket
    unc = [b for b in bad if b[0] == 'uncovered']
    assert unc and all(b[3] == segs[i][2:] and b[1] == bwd.tags[k] for b in unc), bad
    assert {b[4] for b in unc} == {b[4] for b in late} or {b[4] for b in late} <= {b[4] for b in unc}, bad
    assert {b[0] for b in bad} == {'late write', 'uncovered'}, bad
    print('control a %s: %s' % (name, late[0]))


@pytest.mark.parametrize('name', ['inception_v3', 'resnet18', 'vgg13_bn', 'densenet121'])
def test_control_b_dropped_batchnorm_offset_is_named(name):
    """a BatchNorm-backward op is said to finish its weight gradient only: the audit names the op, the bucket and the bias it writes
    all the same -- and dp.segment_plan, planning from that table, no longer finds the buffer covered"""
    from ifcb_classifier_amd.dp import segment_plan
    eng, pl, segs, writes = _plan(name, 2, 'bf16', 2)
    bwd = pl.bwd_list
    bn = (_lib.OP_BN_BWD, _lib.OP_BN_BWD_MAXPOOL, _lib.OP_BN_BWD_PARTIALS)
    ks = [k for k, o in enumerate(bwd.ops) if o.kind in bn]
    assert len(ks) >= 10
    k = ks[len(ks) // 2]
    offs = dt.table_offsets(eng, bwd)
    dropped = offs[k][1]                                   # d(beta)
    offs[k] = [o for o in offs[k] if o != dropped]
    bad = dt.audit(eng, bwd, segs, offs, writes)
    key = [kk for kk, v in eng.poff.items() if v[0] == dropped][0]
    bucket = [s[2:] for s in segs if s[2] <= dropped < s[3]][0]
    assert [(b[0], b[1], b[2], b[3], b[4]) for b in bad] == [('table', bwd.tags[k], _lib.OP_NAMES[bwd.ops[k].kind], bucket, key)], bad
    assert key.endswith('.bias') and eng.poff[key][3] == 'bn_b'
    with pytest.raises(RuntimeError, match='does not cover'):
        segment_plan(offs, eng.palloc, eng.nparam_padded, 8)
    print('control b %s: %s' % (name, bad[0]))


def test_control_c_an_accumulating_first_write_and_a_write_into_the_padding_are_named():
    """the accumulate bit of a weight gradient set (flags bit 0, what program_footprints._acc reads); a weight gradient one element long"""
    eng, pl, segs, writes = _plan('resnet18', 2, 'bf16', 2)
    bwd = pl.bwd_list
    k = next(k for k, o in enumerate(bwd.ops) if o.kind == _lib.OP_CONV_WGRAD and not o.flags & 1)
    o = _lib.Op.from_buffer_copy(bwd.ops[k])
    o.flags |= 1
    mutated = type(bwd)()
    mutated.ops, mutated.tags, mutated.meta = list(bwd.ops), list(bwd.tags), list(bwd.meta)
    mutated.ops[k] = o
    bad = dt.audit(eng, mutated, segs, dt.table_offsets(eng, bwd))
    assert [(b[0], b[1], b[2]) for b in bad] == [('accumulates first', bwd.tags[k], 'conv_wgrad')], bad
    # the head's bias gradient (7 classes in an 8-element slot) made one element longer reaches the padding behind it
    wr = [list(w) for w in writes]
    off, n = eng.poff['fc.bias'][:2]
    assert n == NC and eng.palloc[off] == 8
    j, i = next((j, i) for j, w in enumerate(wr) for i, (a, b, _acc) in enumerate(w) if (a, b) == (off, off + n))
    wr[j][i] = (off, off + n + 1, wr[j][i][2])
    bad = dt.audit(eng, bwd, segs, dt.table_offsets(eng, bwd), wr)
    assert [(b[0], b[1], b[4]) for b in bad] == [('padding', bwd.tags[j], 'fc.bias')], bad


def test_control_d_a_dead_bias_without_its_batchnorm():
    """vgg13_bn: the conv bias in front of a BatchNorm rides with that BatchNorm's backward op.  Said of another op, the audit names it"""
    eng, pl, segs, writes = _plan('vgg13_bn', 2, 'bf16', 2)
    bwd = pl.bwd_list
    offs = dt.table_offsets(eng, bwd)
    ks = [k for k in range(len(offs)) if any(o in offs[k] for lst in eng.cbias_after.values() for o in lst)]
    assert len(ks) == 10 and all(bwd.ops[k].kind in (_lib.OP_BN_BWD, _lib.OP_BN_BWD_MAXPOOL, _lib.OP_BN_BWD_PARTIALS) for k in ks)
    k = ks[3]
    rider = [o for o in offs[k] if o in eng.cbias_after[offs[k][0]]]
    offs[k] = [o for o in offs[k] if o not in rider]
    j = next(j for j in range(k + 1, len(offs)) if offs[j] and j not in ks)          # a later op that writes some other tensor
    offs[j] = offs[j] + rider
    bad = dt.audit(eng, bwd, segs, offs, writes)
    assert [(b[0], b[1]) for b in bad] == [('table', bwd.tags[j])] and 'rides with' in bad[0][5], bad
