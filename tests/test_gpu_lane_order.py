"""A missing dependency between program lanes, made deterministic (helpers and the poison list: tests/lane_order.py).

The engine's own frozen programs run with delay ops in front of chosen ops -- every op of one lane, or a seeded random quarter --
on buffers whose every product was overwritten with NaN, and must leave exactly the bits of the single-lane program, which is plain
stream order.  A consumer that does not wait for a slowed producer reads NaN; a writer that does not wait for a slowed reader
changes what that reader sees.  tests/test_program_footprints_cpu.py checks the same property statically, from the pointers."""
import os
from unittest import mock

import pytest
import torch

import lane_order as lo
from ifcb_classifier_amd import _lib

pytestmark = pytest.mark.gpu

# the smallest shapes at which each plan has its full op list (as test_gpu_model.py / test_gpu_families.py use them)
FAMILIES = {
    'inception_v3': ('inception_v3', 6, 299, {}),
    'inception_v3-lanes2': ('inception_v3', 6, 299, {'IFCBK_LANES': '2'}),       # the data-parallel default
    'resnet18': ('resnet18', 8, 224, {}),                                       # downsample branches
    'densenet121': ('densenet121', 4, 224, {}),                                 # dx accumulating into concatenation slices
    'squeezenet1_1': ('squeezenet', 4, 224, {}),                                # fire modules, ceil-mode pools
}


class Rig:
    pass


@pytest.fixture(scope='module')
def rig(request):
    from conftest import MEASURED
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    name, B, S, env = FAMILIES[request.param]
    r = Rig()
    r.family, r.B = request.param, B
    with mock.patch.dict(os.environ, env):
        eng = r.eng = Engine(graph.build(name, 7, pretrained=False), device=0, max_batch=B)
        eng.init_weights(seed=4321)
        eng.dropout_seed = 5
        pl = r.pl = eng.plan(B)
    assert eng.NL == int(env.get('IFCBK_LANES', 4))
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(3)]
    r.ys = [torch.randint(0, 7, (B,), generator=g) for _ in range(3)]
    # the plan really spreads over lanes at this size
    assert len(lo.lanes_of(pl.step.arr, pl.step.n)) >= 2 and len(lo.lanes_of(pl.fwd_eval.arr, pl.fwd_eval.n)) >= 2, request.param
    one = lambda arr, n: (lo.single_lane(arr, n), n)
    # a warm-up step: Adam moments, running statistics and step count of a run in progress
    lo.run_step(eng, pl, B, r.xs[2], r.ys[2], one)
    r.snap = lo.snapshot(eng)
    # ---- the single-lane reference on poisoned buffers, two steps; the first one timed per op to size the delay
    lo.restore(eng, r.snap)
    lo.poison(eng)
    ms = lo.run_step(eng, pl, B, r.xs[0], r.ys[0], one, op_ms=True)
    r.ref = [lo.outcome(eng)]
    lo.run_step(eng, pl, B, r.xs[1], r.ys[1], one)
    r.ref.append(lo.outcome(eng))
    r.longest_ms = max(ms)
    r.longest_tag = pl.step.tags[ms.index(r.longest_ms)]
    r.scratch, r.delay_bytes, r.delay_reps, r.delay_ms = lo.size_delay(eng, r.longest_ms)
    MEASURED.append('lane order %-20s longest op %.3f ms (%s), delay %.3f ms (%d x %d MiB memset), step ops %d on lanes %s, eval ops %d on lanes %s'
                    % (request.param, r.longest_ms, r.longest_tag, r.delay_ms, r.delay_reps, r.delay_bytes >> 20, pl.step.n,
                       lo.lanes_of(pl.step.arr, pl.step.n), pl.fwd_eval.n, lo.lanes_of(pl.fwd_eval.arr, pl.fwd_eval.n)))
    print(MEASURED[-1])
    yield r
    eng.close()


def _two_steps(r, make_arr):
    eng = r.eng
    lo.restore(eng, r.snap)
    lo.poison(eng)
    outs = []
    for k in range(2):
        lo.run_step(eng, r.pl, r.B, r.xs[k], r.ys[k], make_arr)
        outs.append(lo.outcome(eng))
    return outs


ALL = pytest.mark.parametrize('rig', sorted(FAMILIES), indirect=True)


@ALL
def test_the_delay_outlasts_the_longest_op(rig):
    """the power of every test below: one delay op alone takes at least as long as the longest single op of the undelayed step, so a
    consumer that does not wait has time to run past its slowed producer"""
    assert rig.delay_ms >= rig.longest_ms, (rig.family, rig.delay_ms, rig.longest_ms, rig.longest_tag, rig.delay_bytes, rig.delay_reps)


@ALL
def test_poisoned_single_lane_step_equals_clean_single_lane_step(rig):
    """on buffers full of NaN the single-lane step leaves the bits it leaves on buffers as allocation leaves them (zeros): the poison
    list of lane_order.py is valid, and no op reads anything the step did not itself produce first"""
    eng = rig.eng
    lo.restore(eng, rig.snap)
    lo.poison(eng, clean=True)
    lo.run_step(eng, rig.pl, rig.B, rig.xs[0], rig.ys[0], lambda arr, n: (lo.single_lane(arr, n), n))
    clean = lo.outcome(eng)
    assert not lo.differing(clean, rig.ref[0]), (rig.family, lo.differing(clean, rig.ref[0]))
    assert bool(torch.isfinite(clean['loss']).all()) and bool(torch.isfinite(clean['G']).all()) and bool(torch.isfinite(clean['P']).all())
    for k, v in clean.items():
        if k.endswith('.logits'):
            assert bool(torch.isfinite(v[:rig.B]).all()), k


@ALL
def test_slowed_lanes_do_not_change_a_bit(rig):
    """every op of one lane delayed, for each lane; three random quarters of all ops: two consecutive steps (the second from the first
    one's leftovers) leave loss, G, P, RB, Adam m / v and the logits of the single-lane run"""
    pl = rig.pl
    pats = lo.patterns(pl.step.arr, pl.step.n)
    assert len(pats) == len(lo.lanes_of(pl.step.arr, pl.step.n)) + 3
    plain = _two_steps(rig, lambda arr, n: ((_lib.Op * n)(*arr), n))
    for k in range(2):
        assert not lo.differing(plain[k], rig.ref[k]), (rig.family, 'undelayed', k, lo.differing(plain[k], rig.ref[k]))
    for name, where in pats.items():
        assert where, name
        outs = _two_steps(rig, lambda arr, n: lo.delayed(arr, n, where, rig.scratch, rig.delay_bytes, rig.delay_reps))
        for k in range(2):
            assert not lo.differing(outs[k], rig.ref[k]), (rig.family, name, 'step %d' % k, lo.differing(outs[k], rig.ref[k]))


@ALL
def test_eval_forward_slowed_lanes(rig):
    eng, pl = rig.eng, rig.pl
    main = [h for h in eng.heads if not h.aux][0]
    lo.restore(eng, rig.snap)
    lo.poison(eng)
    lo.run_eval(eng, pl, rig.B, rig.xs[0], lambda arr, n: (lo.single_lane(arr, n), n))
    ref = main.logits.clone()
    assert bool(torch.isfinite(ref[:rig.B]).all())
    for name, where in lo.patterns(pl.fwd_eval.arr, pl.fwd_eval.n).items():
        lo.restore(eng, rig.snap)
        lo.poison(eng)
        lo.run_eval(eng, pl, rig.B, rig.xs[0], lambda arr, n: lo.delayed(arr, n, where, rig.scratch, rig.delay_bytes, rig.delay_reps))
        assert lo.same_bits(main.logits, ref), (rig.family, name)


def _drop_wait(r, j, lane):
    """the step with op j no longer waiting for `lane`, every op of `lane` delayed -> outcome of one step on poisoned buffers"""
    pl = r.pl
    assert (pl.step.arr[j].flags >> 12) >> lane & 1 and (pl.step.arr[j].flags >> 8) & 7 != lane

    def make(arr, n):
        cp = (_lib.Op * n)(*arr)
        cp[j].flags &= ~(1 << (12 + lane))
        return lo.delayed(cp, n, [k for k in range(n) if (cp[k].flags >> 8) & 7 == lane], r.scratch, r.delay_bytes, r.delay_reps)
    lo.restore(r.eng, r.snap)
    lo.poison(r.eng)
    lo.run_step(r.eng, pl, r.B, r.xs[0], r.ys[0], make)
    return lo.outcome(r.eng)


@pytest.mark.parametrize('rig', ['densenet121', 'inception_v3'], indirect=True)
def test_a_dropped_wait_is_caught(rig):
    """the method has teeth: in a copy of the step one op loses the wait for the lane of its producer, that lane is slowed, and the
    outcome differs from the single-lane bits.  Both ops read floating-point data only across the dropped edge, so every address stays
    valid: a wrong number, not a fault.
    inception_v3: a single-layer weight gradient (weight-gradient lane) that waits for its layer's BatchNorm backward -- it reads the
    poisoned d(raw), G holds NaN.  densenet121: the input gradient of a growth conv (and the weight
    gradient in front of it), which read their slice of the concatenation's gradient while the later layers' BatchNorm backwards still accumulate into it."""
    pl = rig.pl
    arr, n, tags = pl.step.arr, pl.step.n, pl.step.tags
    lane = lambda k: (arr[k].flags >> 8) & 7
    if rig.family == 'inception_v3':
        # one such weight gradient per chain lane that feeds the weight-gradient lane.  How far the weight-gradient lane runs behind its
        # producers varies from run to run (one run caught both candidates, another only the lane-2 one), so the control asks for
        # at least one of the two to surface; each candidate alone is a dropped edge the audit on the CPU names deterministically.
        caught = {}
        for tag in ('Mixed_6b.branch7x7_2.conv', 'Mixed_6b.branch7x7dbl_2.conv'):
            j = next(k for k in range(n) if arr[k].kind == _lib.OP_CONV_WGRAD and tags[k] == tag)
            i = next(k for k in range(n) if arr[k].kind in (_lib.OP_BN_BWD, _lib.OP_BN_BWD_PARTIALS) and tags[k] == tag)
            assert i < j and arr[i].p[8 if arr[i].kind == _lib.OP_BN_BWD_PARTIALS else 6] == arr[j].p[1]          # its d(raw) is the weight gradient's dy
            assert lane(j) == rig.eng.NL - 1 and lane(i) not in caught
            out = _drop_wait(rig, j, lane(i))
            caught[lane(i)] = 'G' in lo.differing(out, rig.ref[0]) and bool(torch.isnan(out['G']).any())
        import conftest
        conftest.MEASURED.append('lane order inception_v3: dropped wait of a weight gradient caught, by producer lane: %s' % caught)
        print(conftest.MEASURED[-1])
        assert len(caught) == 2 and any(caught.values()), caught
    else:
        # a growth conv (no BatchNorm behind it) whose dy is a channel slice (pixel stride > channels) of a concatenation's gradient, in
        # the middle of a dense block.  Its weight gradient and its input gradient both read that slice, back to back on one lane: the
        # first of the two carries the wait for the lane whose BatchNorm backward accumulated into the slice last, the input gradient
        # right behind it is ordered by the stream alone -- dropping that one bit lets both run ahead
        cands = [k for k in range(n - 1) if arr[k].kind == _lib.OP_CONV_WGRAD and arr[k].u.conv.ldy > arr[k].u.conv.K
                 and bin((arr[k].flags >> 12) & 0xff).count('1') == 1 and 'denseblock3' in tags[k]
                 and arr[k + 1].kind == _lib.OP_CONV_DGRAD and tags[k + 1] == tags[k] and lane(k + 1) == lane(k)
                 and not (arr[k + 1].flags >> 12) & 0xff and arr[k + 1].p[0] == arr[k].p[1]]
        assert cands, 'no growth conv reads its slice of the concatenation gradient behind exactly one other lane'
        j = cands[len(cands) // 2]
        out = _drop_wait(rig, j, ((arr[j].flags >> 12) & 0xff).bit_length() - 1)
        assert 'G' in lo.differing(out, rig.ref[0]), tags[j]


@ALL
def test_the_plans_that_ran_pass_the_footprint_audit(rig):
    """tests/test_program_footprints_cpu.py audits Engine(plan_only=True), which plans the same ops as an engine with a device (the
    eval-mode conv + max-pool fusion, OP_CONV_FWD_AFFINE_MAXPOOL, included) but skips the workspace growth of the grouped weight
    gradients.  The same audit over the programs that the tests above launched."""
    import program_footprints as pf
    pl = rig.pl
    for prog in ('step', 'fwd_eval', 'fwd_train', 'bwd', 'pack', 'evalprep'):
        p = getattr(pl, prog)
        bad = pf.unordered_conflicts(rig.eng, p.arr, p.n, p.tags)
        assert not bad, (rig.family, prog, bad[:6])
    if rig.family.startswith('inception_v3'):
        assert pl.fwd_eval.find(_lib.OP_CONV_FWD_AFFINE_MAXPOOL)
