"""Every way Engine.train_step launches a step leaves the bits of plain stream order.

The benchmark times `train_step(B, ev_slot=k, ev_arr=...)` -- ifcbk_run_program_ev on a copy of the op table made by Program.timed --
and surveys per-kernel times with `timed(single_lane=True)`; graph mode replays forward + backward as a hipGraph and runs Adam from
pl.adam_pack.  Each of these stamps the per-step Adam scalars (step count, gradient scale) into an array of its own.  Here one rig
per family (the sizes of tests/test_gpu_lane_order.py) takes, from one restored snapshot and on poisoned buffers, two steps through the
public method in each mode; after each step loss, G, P, M, V, RB, every head's logits, num_batches_tracked and loss_sum must equal, bit
for bit, the two steps of tests/lane_order.run_step on the single-lane copy of pl.step.arr.  The second step's bias correction differs
from the first's: a table whose step count was not refreshed diverges in P, M and V (test_a_stale_step_count_is_caught does exactly
that).  The per-op times of the event modes are read back through ifcbk_program_times and checked against what was bracketed."""
import ctypes as C
import math
import os
from unittest import mock

import pytest
import torch

import lane_order as lo
from ifcb_classifier_amd import _lib

pytestmark = pytest.mark.gpu

# (model, batch, input side, environment): tests/test_gpu_lane_order.py, the smallest shapes at which each plan has its full op list
FAMILIES = {
    'inception_v3': ('inception_v3', 6, 299, {}),
    'inception_v3-lanes2': ('inception_v3', 6, 299, {'IFCBK_LANES': '2'}),
    'resnet18': ('resnet18', 8, 224, {}),
}
MODES = ('plain', 'op_ms', 'ev_all', 'ev_conv', 'ev_single_lane', 'graph')


class Rig:
    pass


outcome = lo.step_outcome                                                    # lo.outcome plus nbt and loss_sum (shared with tests/engine_life.py)


@pytest.fixture(scope='module')
def rig(request):
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
    assert eng.NL == int(env.get('IFCBK_LANES', 4)) and not eng.graph_train
    assert len(lo.lanes_of(pl.step.arr, pl.step.n)) >= 2
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(3)]
    r.ys = [torch.randint(0, 7, (B,), generator=g) for _ in range(3)]
    one = lambda arr, n: (lo.single_lane(arr, n), n)
    lo.run_step(eng, pl, B, r.xs[2], r.ys[2], one)                        # warm-up: moments, running statistics, step count 1
    r.snap = lo.snapshot(eng)
    lo.restore(eng, r.snap)
    lo.poison(eng)
    r.ref = []
    for k in range(2):
        lo.run_step(eng, pl, B, r.xs[k], r.ys[k], one)
        r.ref.append(outcome(eng))
    assert not lo.same_bits(r.ref[0]['P'], r.ref[1]['P']) and bool(torch.isfinite(r.ref[1]['P']).all())
    r.which = pl.step.find(_lib.OP_CONV_FWD)
    assert r.which and len(r.which) < pl.step.n
    r.done = {}
    yield r
    eng.close()


def _steps(r, step):
    """two steps from the snapshot on poisoned buffers; step(k) makes the train_step call -> outcome after each"""
    eng = r.eng
    lo.restore(eng, r.snap)
    lo.poison(eng)
    outs = []
    for k in range(2):
        eng.load_input_nchw(r.xs[k])
        eng.target[:r.B].copy_(r.ys[k])
        step(k)
        torch.cuda.synchronize()
        outs.append(outcome(eng))
    return outs


def _times(eng, slot, n):
    ms = (C.c_float * n)(*([float('nan')] * n))
    assert eng.ctx.lib.ifcbk_program_times(eng.ctx.h, slot, n, ms) == _lib.OK, eng.ctx.lib.ifcbk_last_error(eng.ctx.h)
    return list(ms)


def _run_mode(r, mode):
    """-> (outcomes of the two steps, what the mode left behind for the checks of its times)"""
    eng, pl, B, n = r.eng, r.pl, r.B, r.pl.step.n
    extra = {}
    if mode == 'plain':
        outs = _steps(r, lambda k: eng.train_step(B))
    elif mode == 'op_ms':
        ms = (C.c_float * n)()
        outs = _steps(r, lambda k: eng.train_step(B, op_ms=ms))
        extra['ms'] = list(ms)
    elif mode == 'ev_all':
        seen = []

        def step(k):
            eng.train_step(B, ev_slot=0)
            seen.append(pl.step_timed_all)
        outs = _steps(r, step)
        assert seen[0] is seen[1] is pl.step_timed_all                    # the second step reuses the cached copy
        extra['arr'] = pl.step_timed_all
    elif mode == 'ev_conv':
        arr = pl.step.timed(r.which)                                      # once, before the first step
        outs = _steps(r, lambda k: eng.train_step(B, ev_slot=1, ev_arr=arr))
        extra['arr'] = arr
    elif mode == 'ev_single_lane':
        arr = pl.step.timed(single_lane=True)                             # the benchmark's survey mode
        assert lo.lanes_of(arr, n) == [0]
        outer = []

        def step(k):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(torch.cuda.current_stream())
            eng.train_step(B, ev_slot=2, ev_arr=arr)
            b.record(torch.cuda.current_stream())
            outer.append((a, b))
        outs = _steps(r, step)
        extra['arr'], extra['outer'] = arr, outer[-1][0].elapsed_time(outer[-1][1])
    elif mode == 'graph':
        assert not eng.graph_train
        eng.graph_train = True
        try:
            outs = _steps(r, lambda k: eng.train_step(B))
            assert 'fwd_bwd' in pl.graphs
        finally:
            eng.graph_train = False
    else:
        raise KeyError(mode)
    if 'arr' in extra:
        slot = {'ev_all': 0, 'ev_conv': 1, 'ev_single_lane': 2}[mode]
        extra['ms'] = _times(eng, slot, n)                                # (after the synchronize of the second step)
        for j in pl.step_adam_idxs:
            assert extra['arr'][j].i[1] == eng.step_count == r.snap['step_count'] + 2
    return outs, extra


def _mode(r, mode):
    if mode not in r.done:
        r.done[mode] = _run_mode(r, mode)
    return r.done[mode]


ALL = pytest.mark.parametrize('rig', sorted(FAMILIES), indirect=True)


@ALL
@pytest.mark.parametrize('mode', MODES)
def test_a_launch_mode_leaves_the_reference_bits(rig, mode):
    outs, _extra = _mode(rig, mode)
    for k in range(2):
        assert sorted(outs[k]) == sorted(rig.ref[k]) and {'loss', 'G', 'P', 'M', 'V', 'RB', 'nbt', 'loss_sum'} <= set(outs[k])
        assert any(key.endswith('.logits') for key in outs[k])
        bad = lo.differing(outs[k], rig.ref[k])
        assert not bad, (rig.family, mode, 'step %d' % k, bad)


@ALL
def test_a_stale_step_count_is_caught(rig):
    """the comparison has teeth: the conv-timed copy takes step 1 through train_step, which stamps it; step 2 launches a copy that kept
    step 1's count (what a mode that forgot _set_update on its own array would run) straight through ifcbk_run_program_ev.  Everything
    else of step 2 is what train_step does.  P, M and V then carry the wrong bias correction."""
    eng, pl, B = rig.eng, rig.pl, rig.B
    arr = pl.step.timed(rig.which)
    stale = []

    def step(k):
        if k == 0:
            eng.train_step(B, ev_slot=1, ev_arr=arr)
            stale.append((_lib.Op * pl.step.n)(*arr))
            return
        eng.ensure_packed(pl)
        eng.make_dropout_mask(B)
        eng.step_count += 1
        for j in pl.step_adam_idxs:
            eng._set_update(pl.step.arr[j])                               # the plan's own table is current; the copy below is not
            assert stale[0][j].i[1] == eng.step_count - 1
        eng.ctx.call('ifcbk_run_program_ev', stale[0], pl.step.n, eng.stream(), 1)
    outs = _steps(rig, step)
    assert not lo.differing(outs[0], rig.ref[0])
    bad = lo.differing(outs[1], rig.ref[1])
    assert 'P' in bad, (rig.family, bad)
    assert 'G' not in bad and 'loss' not in bad                           # forward and backward do not read the step count


@ALL
def test_times_of_the_event_modes(rig):
    from conftest import MEASURED
    eng, pl, n = rig.eng, rig.pl, rig.pl.step.n
    for mode in ('op_ms', 'ev_all', 'ev_conv', 'ev_single_lane'):
        ms = _mode(rig, mode)[1]['ms']
        assert len(ms) == n and all(math.isfinite(m) and m >= 0 for m in ms), (rig.family, mode, [m for m in ms if not (math.isfinite(m) and m >= 0)][:5])
    # conv-timed: exactly the bracketed ops have a time
    ms = _mode(rig, 'ev_conv')[1]['ms']
    which = set(rig.which)
    assert all(ms[k] > 0 for k in which), [k for k in which if not ms[k] > 0][:5]
    assert all(ms[k] == 0.0 for k in range(n) if k not in which)
    # single lane, all ops: every op that launches a named kernel took time ...
    ms, extra = _mode(rig, 'ev_single_lane')[1]['ms'], _mode(rig, 'ev_single_lane')[1]
    name = C.create_string_buffer(256)
    named = []
    for k in range(n):
        assert eng.ctx.lib.ifcbk_op_kernel(C.byref(pl.step.arr[k]), name, 256) == _lib.OK
        if name.value:
            named.append(k)
    assert len(named) > n // 2
    assert all(ms[k] > 0 for k in named), [(k, pl.step.tags[k]) for k in named if not ms[k] > 0][:5]
    # ... and, back to back on one stream, the ops' disjoint intervals lie inside the one around the whole call: their sum is at most
    # the outer time plus one event granularity per op.  g: the largest time between two events recorded with nothing between them
    pairs = []
    s = torch.cuda.current_stream()
    for _ in range(100):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        b.record(s)
        pairs.append((a, b))
    torch.cuda.synchronize()
    g = max(a.elapsed_time(b) for a, b in pairs)
    total, outer = sum(ms), extra['outer']
    MEASURED.append('step modes %-20s single-lane timed step: %d ops, sum(ms) %.4f, outer %.4f ms, event granularity g %.5f ms (bound %.4f)'
                    % (rig.family, n, total, outer, g, outer + n * g))
    assert math.isfinite(g) and g >= 0
    assert total <= outer + n * g, (rig.family, total, outer, g, n)
