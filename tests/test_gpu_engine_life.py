"""One engine through the life of a TRAIN run, held to the raw bits of a fresh engine (helpers and the hostile set-up: tests/engine_life.py).

Per family one long-lived engine of capacity B is warmed up with a full batch and then dirtied again and again; per (family, N) one
fresh engine of capacity N serves as the reference and is closed when its cases are done (at most three engines are alive: the
long-lived one, the fresh one and the fp32 engine of the oracle anchor).  Everything is compared with lane_order.same_bits; that the
two engines run the same program is pinned by tests/test_engine_life_cpu.py.  What each scenario would catch:

  1 partial batch on dirty buffers   a kernel that reads a tile row, a target, a mask row or an input image behind N
  2 nothing behind N is written      a kernel that writes one (activations, gradients, raws, heads, probs, arg-max, per-lane scratch)
  3 eval between two steps           an eval forward that touches training state: nbt, loss_sum, step_count, dropout_calls, RB, a shadow
  4 eval after a step                a stale `packed` or `eval_stats_ready`, a graph replayed over stale shadows; evalprep skipped for a
                                     second plan while the engine-global flag is set
  5 writes from outside              load_state_dict / params_changed not reaching packed and eval_stats_ready
  6 input kinds and slots            the plan key (N, slot, kind) changing under shared buffers; the u8 stem reading the dense tensor
  7 the workspace moves              a graph replayed after its arena moved; pl.graphs not emptied
  8 refusals                         a refused call that already counted a step, drew a mask or built a plan

The anchor outside the code under test: the partial-batch train step and the eval behind it in fp32 mode against oracle/tv_models
(fp32 storage), at the tolerances of tests/test_gpu_model.py::test_fp32_mode_meets_the_north_star_tolerance."""
import ctypes as C
import os
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import engine_life as el
import lane_order as lo
from local_parity import rel

pytestmark = pytest.mark.gpu

# Scenario 2's exemptions: a buffer that is legitimately written behind image N goes here BY NAME, with the source line that writes it
# quoted (checked against the file, as tests/test_op_inventory_cpu.py does with dispatch conditions).  No buffer is exempt by default,
# and more than three entries mean something is wrong that has to be understood first.
#   buffer name -> (file under ifcb_classifier_amd/, quoted line, why the write is legitimate)
WRITES_BEHIND_N = {}


class Life:
    """the long-lived engine of one family, behind the module surface (scenario 5 writes through it), warmed up with one full batch"""

    def __init__(self, family):
        from ifcb_classifier_amd.neuston_models import get_namebrand_model
        self.family = family
        self.name, self.B, self.S = el.FAMILIES[family]
        B, S = self.B, self.S
        self.hip = get_namebrand_model(self.name, el.NC, max_batch=B)
        eng = self.eng = self.hip.engine
        eng.init_weights(seed=4321)
        eng.dropout_seed = 5
        assert eng.graph_eval and not eng.graph_train and eng.train_batch == eng.max_batch == B
        g = torch.Generator().manual_seed(9)
        self.xs_cpu = [torch.rand(B, 3, S, S, generator=g) for _ in range(4)]           # x0, x1, the eval batch, the warm-up
        self.xs = [x.cuda() for x in self.xs_cpu]
        self.ys = [el.labels(B, g) for _ in range(4)]
        self.rois = [el.make_rois(B, 21 + k) for k in range(3)] if family == 'inception_v3' else None
        el.stage_dense(eng, B, self.xs[3], self.ys[3])
        eng.train_step(B)                                                               # moments, running statistics, step count 1
        torch.cuda.synchronize()
        self.snap = lo.snapshot(eng)
        self._two = self._anchor = None

    def two_steps(self):
        """T(B, x0), T(B, x1) from the snapshot on poisoned buffers -> what scenario 3 must find after its detour through eval"""
        if self._two is None:
            eng, B = self.eng, self.B
            lo.restore(eng, self.snap)
            el.poison(eng, B)
            for k in range(2):
                el.stage_dense(eng, B, self.xs[k], self.ys[k])
                out = el.train(eng, B)
            self._two = (out, eng.step_count, eng.dropout_calls)
        return self._two

    def anchor(self):
        """-> (fp32 module of capacity B, dirtied by one full step; its post-warm-up snapshot; the fp32 oracle)"""
        if self._anchor is None:
            from ifcb_classifier_amd.neuston_models import get_namebrand_model
            from oracle import tv_models
            hip = get_namebrand_model(self.name, el.NC, max_batch=self.B, dtype='fp32')
            eng = hip.engine
            eng.init_weights(seed=4321)
            eng.dropout_seed = 5
            el.stage_dense(eng, self.B, self.xs[3], self.ys[3])
            eng.train_step(self.B)
            torch.cuda.synchronize()
            self._anchor = (hip, lo.snapshot(eng), tv_models.get_namebrand_model(self.name, el.NC, storage='fp32'))
        return self._anchor

    def close(self):
        if self._anchor is not None:
            self._anchor[0].engine.close()
        self.eng.close()
        self._anchor = self._two = None
        torch.cuda.empty_cache()


class Pair:
    """the long-lived engine and the fresh engine of capacity N, with the references every scenario of that N shares"""

    def __init__(self, life, N):
        from ifcb_classifier_amd import graph
        from ifcb_classifier_amd.engine import Engine
        self.life, self.N = life, N
        self.eng = life.eng
        self.fresh = Engine(graph.build(life.name, el.NC, pretrained=False), device=0, max_batch=N)
        assert self.fresh.train_batch == self.fresh.max_batch == N
        self._ref, self._dirty = {}, {}

    # ---- the fresh engine
    def fresh_train(self, snap, stage):
        lo.restore(self.fresh, snap)
        stage(self.fresh)
        return el.train(self.fresh, self.N)

    def fresh_eval(self, snap, stage):
        lo.restore(self.fresh, snap)
        stage(self.fresh)
        return el.evaluate(self.fresh, self.N)

    def ref(self, what):
        """the fresh engine, given the snapshot and only this batch: 'train' on (x0, y0), 'eval' on the eval batch"""
        if what not in self._ref:
            life, N = self.life, self.N
            if what == 'train':
                self._ref[what] = self.fresh_train(life.snap, lambda e: el.stage_dense(e, N, life.xs[0], life.ys[0]))
            else:
                self._ref[what] = self.fresh_eval(life.snap, lambda e: el.stage_dense(e, N, life.xs[2], life.ys[2]))
        return self._ref[what]

    # ---- the long-lived engine at N, from the snapshot
    def dirty(self, what, clean):
        """-> (outcome, buffers written behind N -- poisoned run only, mask rows >= N still as set)"""
        key = (what, clean)
        if key not in self._dirty:
            life, N, eng = self.life, self.N, self.eng
            tail = 0 if clean else 1
            lo.restore(eng, life.snap)
            el.poison(eng, N, clean)
            if what == 'train':
                el.stage_dense(eng, N, life.xs[0], life.ys[0], tail)
                out = el.train(eng, N)
            else:
                el.stage_dense(eng, N, life.xs[2], life.ys[2], tail)
                out = el.evaluate(eng, N)
            behind = None if clean else el.written_behind(eng, self.fresh, N)
            masks = [m.mask for m in list(eng.heads) + list(eng.drops) if getattr(m, 'mask', None) is not None]
            masks_ok = all(bool((m[N:] == tail).all()) for m in masks)
            tgt_ok = bool((eng.target[N:] == el.JUNK).all())
            self._dirty[key] = (out, behind, masks_ok and tgt_ok)
        return self._dirty[key]

    def close(self):
        self.fresh.close()
        self._ref.clear()
        self._dirty.clear()


_LIVE = {}


def _release(keep=None):
    for f in list(_LIVE):
        if f != keep:
            _LIVE.pop(f).close()


@pytest.fixture(scope='module', autouse=True)
def _close_everything():
    yield
    _release()


@pytest.fixture(scope='module')
def pair(request):
    family, N = request.param.rsplit('-', 1)
    _release(keep=family)                              # one family's engines at a time
    if family not in _LIVE:
        _LIVE[family] = Life(family)
    p = Pair(_LIVE[family], int(N))
    yield p
    p.close()


ALL = pytest.mark.parametrize('pair', el.PAIRS, indirect=True)
INCEPTION = pytest.mark.parametrize('pair', el.INCEPTION_PAIRS, indirect=True)


def _same(got, want, *ctx):
    assert sorted(got) == sorted(want), (ctx, sorted(got), sorted(want))
    bad = lo.differing(got, want)
    assert not bad, ctx + (bad,)
    assert not el.all_finite(got), ctx + ('not finite', el.all_finite(got))


def test_the_exemption_table_is_short_and_quotes_live_source():
    assert len(WRITES_BEHIND_N) <= 3
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ifcb_classifier_amd')
    for name, (fname, quote, why) in WRITES_BEHIND_N.items():
        assert why and ' '.join(quote.split()) in ' '.join(open(os.path.join(root, fname)).read().split()), name


# ------------------------------------------------------------------------------------------------ 7: the workspace moves under graphs
def test_the_workspace_moves_under_a_captured_eval_graph():
    """an inference engine (train_batch = 1, a small reservation) captures its eval graph; load_rois with small ROIs but declared bounds
    so large that ifcbk_roi_preprocess_workspace exceeds ifcbk_ctx_workspace_bytes moves the workspace: the reservation rises, the live
    graphs of the ctx fall to 0, and forward_eval on the same input has its pre-growth bits and one live graph again.  The header's
    contract for a handle kept across a direct ctx.reserve growth: ifcbk_graph_launch refuses it with IFCBK_EINVAL (the return code is
    all that is checked: nothing is launched).  Also scenario 8's first refusal: train_step(N > train_batch) raises and changes nothing."""
    from ifcb_classifier_amd import _lib, graph
    from ifcb_classifier_amd.engine import Engine
    N = 2
    eng = Engine(graph.build('inception_v3', el.NC, pretrained=False), device=0, max_batch=3, train_batch=1)
    try:
        eng.init_weights(seed=4321)
        lib, h = eng.ctx.lib, eng.ctx.h
        rois = el.make_rois(N, 5)
        y = torch.tensor([0, 1])
        el.stage_rois(eng, N, rois, y)
        first = el.evaluate(eng, N)
        plane = eng.in_u8[0][:N].clone()
        pl = eng.plan(N)
        assert eng.graph_eval and list(pl.graphs) == ['fwd_eval'] and eng.ctx.live_graphs() == 1
        # ---- refused: a train step beyond the gradient buffers of an inference engine
        before = el.host_state(eng)
        with pytest.raises(RuntimeError, match='built for inference'):
            eng.train_step(N)
        assert not el.host_state_changes(before, el.host_state(eng)) and eng.ctx.live_graphs() == 1
        # ---- the bounds (bounds only: the ROIs stay a few kilobytes) at which the resize tables outgrow the reservation
        d = _lib.RoiDesc()
        d.n_img, d.S, d.in_channels, d.out_channels, d.dtype = N, eng.net.S, 1, 8, eng.cdtype
        ws0 = lib.ifcbk_ctx_workspace_bytes(h)
        bound = max(rois['max_h'], rois['max_w'])
        while lib.ifcbk_roi_preprocess_workspace(C.byref(d), bound, bound) <= ws0:
            bound *= 2
            assert bound < 1 << 26
        el.stage_rois(eng, N, dict(rois, max_h=bound, max_w=bound), y)
        assert lib.ifcbk_ctx_workspace_bytes(h) > ws0 and eng.ctx.live_graphs() == 0 and not pl.graphs
        torch.cuda.synchronize()
        assert torch.equal(eng.in_u8[0][:N], plane)                                    # the same input as before the growth
        again = el.evaluate(eng, N)
        _same(again, first, 'after the workspace moved')
        assert eng.ctx.live_graphs() == 1 and list(pl.graphs) == ['fwd_eval']
        # ---- a handle kept across a direct growth is refused, not replayed
        g = pl.graphs['fwd_eval']
        eng.ctx.reserve(2 * lib.ifcbk_ctx_workspace_bytes(h))
        assert lib.ifcbk_graph_launch(h, g, eng.stream()) == _lib.EINVAL
        assert b'the workspace moved' in lib.ifcbk_last_error(h)
        assert lib.ifcbk_graph_destroy(h, g) == _lib.OK and eng.ctx.live_graphs() == 0
        pl.graphs.clear()
        _same(el.evaluate(eng, N), first, 'recaptured after the direct growth')
        assert eng.ctx.live_graphs() == 1
    finally:
        eng.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ 1: a partial batch on dirty buffers
@ALL
@pytest.mark.parametrize('clean', [False, True], ids=['nan', 'zeros'])
def test_partial_train_step_on_dirty_buffers(pair, clean):
    """train_step(N) on the capacity-B engine -- every product poisoned with NaN (or zeroed), the input, targets and mask rows behind N
    hostile -- leaves loss, G, P, M, V, RB, nbt, loss_sum and every head's logits[:N] of the fresh engine at N, all finite.
    inception_v3 at N = 1 has BatchNorms over a single value (the auxiliary head's 1 x 1 maps): torch refuses that case, bn.hip
    takes unbias = 1 (`d->M > 1 ? M / (M - 1.0) : 1.0`); what the engine does there is pinned the same way, finite and equal."""
    got, _behind, _ok = pair.dirty('train', clean)
    want = pair.ref('train')
    assert {'loss', 'G', 'P', 'M', 'V', 'RB', 'nbt', 'loss_sum'} <= set(want) and any(k.endswith('.logits') for k in want)
    _same(got, want, pair.life.family, pair.N, 'train', 'zeros' if clean else 'nan')
    assert pair.eng.step_count == pair.fresh.step_count == pair.life.snap['step_count'] + 1


@ALL
@pytest.mark.parametrize('clean', [False, True], ids=['nan', 'zeros'])
def test_partial_eval_on_dirty_buffers(pair, clean):
    """forward_eval(N) + pl.eval_loss + pl.softmax under the same set-up: probs[:N], loss and the logits[:N] of the fresh engine"""
    got, _behind, _ok = pair.dirty('eval', clean)
    want = pair.ref('eval')
    assert {'probs', 'loss'} <= set(want) and any(k.endswith('.logits') for k in want)
    _same(got, want, pair.life.family, pair.N, 'eval', 'zeros' if clean else 'nan')


# ------------------------------------------------------------------------------------------------ 2: nothing behind image N is written
@ALL
@pytest.mark.parametrize('what', ['train', 'eval'])
def test_nothing_behind_image_n_is_written(pair, what):
    """after the NaN run of scenario 1 every tensor with a leading batch dimension still holds the poison from image N on, the flat
    per-lane scratch behind the extent the capacity-N engine allocates for it, and the targets and mask rows behind N what was put there"""
    _out, behind, inputs_ok = pair.dirty(what, False)
    assert inputs_ok
    unknown = [b for b in behind if b not in WRITES_BEHIND_N]
    assert not unknown, (pair.life.family, pair.N, what, unknown)


# ------------------------------------------------------------------------------------------------ 3: eval leaves no trace in training
@ALL
@pytest.mark.parametrize('graph_eval', [True, False], ids=['graph', 'IFCBK_GRAPH=0'])
def test_eval_between_two_steps_leaves_no_trace(pair, graph_eval):
    """T(B, x0), E(B, xe), E(N, xe[:N]), T(B, x1) from the snapshot leaves what T(B, x0), T(B, x1) leaves: the outcome with nbt and
    loss_sum, step_count and dropout_calls.  IFCBK_GRAPH=0 is graph_eval = False (tests/test_engine_life_cpu.py: read once)."""
    life, eng, N, B = pair.life, pair.eng, pair.N, pair.life.B
    want, steps, calls = life.two_steps()
    assert eng.graph_eval
    eng.graph_eval = graph_eval
    try:
        lo.restore(eng, life.snap)
        el.poison(eng, B)
        el.stage_dense(eng, B, life.xs[0], life.ys[0])
        el.train(eng, B)
        el.stage_dense(eng, B, life.xs[2], life.ys[2])
        el.evaluate(eng, B)
        el.stage_dense(eng, N, life.xs[2], life.ys[2], 1)
        el.evaluate(eng, N)
        assert not graph_eval or 'fwd_eval' in eng.plan(N).graphs
        el.stage_dense(eng, B, life.xs[1], life.ys[1])
        got = el.train(eng, B)
    finally:
        eng.graph_eval = True
    _same(got, want, life.family, N, graph_eval)
    assert (eng.step_count, eng.dropout_calls) == (steps, calls)


# ------------------------------------------------------------------------------------------------ 4: eval sees the state a step left
@ALL
def test_eval_sees_the_state_a_step_left(pair):
    """after T(B, x0): E(N) equals the fresh engine loaded with the post-step state; after a second step, with nothing rebuilt, E(B)
    runs first and E(N) behind it -- evalprep is then skipped for the N plan (the flag is engine-global) and E(N) must still be right"""
    life, eng, N, B = pair.life, pair.eng, pair.N, pair.life.B
    stage_n = lambda e: el.stage_dense(e, N, life.xs[2], life.ys[2], 1)
    lo.restore(eng, life.snap)
    el.poison(eng, B)
    for k in range(2):
        el.stage_dense(eng, B, life.xs[k], life.ys[k])
        el.train(eng, B)
        assert eng.packed and not eng.eval_stats_ready
        after = lo.snapshot(eng)
        if k == 1:
            el.stage_dense(eng, B, life.xs[2], life.ys[2])
            el.evaluate(eng, B)
            assert eng.eval_stats_ready
        stage_n(eng)
        got = el.evaluate(eng, N)
        _same(got, pair.fresh_eval(after, stage_n), life.family, N, 'after step %d' % k)


# ------------------------------------------------------------------------------------------------ 5: writes from outside
@ALL
def test_writes_from_outside_reach_the_next_eval_and_step(pair):
    """between two evals the model changes through the public surface -- load_state_dict of another state, then an in-place write to a
    parameter and a running variance through the module's views followed by params_changed(), which is what neuston_models.py calls --
    and the next eval and the next train step equal the fresh engine with that state"""
    life, eng, N, hip = pair.life, pair.eng, pair.N, pair.life.hip
    stage_e = lambda e: el.stage_dense(e, N, life.xs[2], life.ys[2], 1)
    stage_t = lambda e: el.stage_dense(e, N, life.xs[0], life.ys[0], 1)
    lo.restore(eng, life.snap)
    stage_e(eng)
    first = el.evaluate(eng, N)
    assert eng.packed and eng.eval_stats_ready and 'fwd_eval' in eng.plan(N).graphs
    other = {k: (v.detach().clone() * 1.0625 if v.is_floating_point() else v.detach().clone()) for k, v in hip.state_dict().items()}
    hip.load_state_dict(other)
    assert not eng.packed and not eng.eval_stats_ready
    stage_e(eng)
    got = el.evaluate(eng, N)
    assert lo.differing(got, first)                                                     # the other state is another model
    _same(got, pair.fresh_eval(lo.snapshot(eng), stage_e), life.family, N, 'load_state_dict')
    with torch.no_grad():
        next(iter(hip.parameters())).mul_(1.5)
        rv = [b for k, b in hip.named_buffers() if k.endswith('running_var')]
        if rv:
            rv[0].add_(0.25)
    eng.params_changed()
    stage_e(eng)
    got2 = el.evaluate(eng, N)
    assert lo.differing(got2, got)
    _same(got2, pair.fresh_eval(lo.snapshot(eng), stage_e), life.family, N, 'in place')
    before = lo.snapshot(eng)
    stage_t(eng)
    _same(el.train(eng, N), pair.fresh_train(before, stage_t), life.family, N, 'step')


# ------------------------------------------------------------------------------------------------ 6: input kinds and slots
@INCEPTION
def test_input_kind_and_slot_switches(pair):
    """one engine, partial N: grey ROIs (the u8 plane), the dense input, ROIs through the prefetch slot -- a step each -- then an eval on
    each kind and one more through the first slot.  After every stage the outcome equals the fresh engine given the state the stage
    started from and only that stage's input.  tests/test_gpu_model.py::test_prefetched_input_slots_equal_sequential_steps covers the
    slots at full B on one kind; this is the plan key (N, slot, kind) changing under shared buffers."""
    life, eng, N, fresh = pair.life, pair.eng, pair.N, pair.fresh
    assert eng.stem_u8 is not None and eng.in_slot == 0
    rois = [{k: (v[:N] if k in ('offs', 'hs', 'ws') else v) for k, v in r.items()} for r in life.rois]
    y = life.ys
    lo.restore(eng, life.snap)
    el.poison(eng, N)
    # (tag, the stage on the long-lived engine, the same input on the fresh engine's only slot, the (slot, kind) it must lead to)
    steps = [('rois', lambda e: el.stage_rois(e, N, rois[0], y[0], 1), None, (0, 'u8')),
             ('dense', lambda e: el.stage_dense(e, N, life.xs[0], y[1], 1), None, (0, 'nhwc')),
             ('rois, prefetch slot', lambda e: el.stage_rois_prefetched(e, N, rois[1], y[2], 1),
              lambda e: el.stage_rois(e, N, rois[1], y[2], 1), (1, 'u8'))]
    evals = [('eval: rois, slot 1', lambda e: el.stage_rois(e, N, rois[2], y[0], 1), None, (1, 'u8')),
             ('eval: dense, slot 1', lambda e: el.stage_dense(e, N, life.xs[2], y[0], 1), None, (1, 'nhwc')),
             ('eval: rois, back through slot 0', lambda e: el.stage_rois_prefetched(e, N, rois[0], y[1], 1),
              lambda e: el.stage_rois(e, N, rois[0], y[1], 1), (0, 'u8'))]
    for run, ref, stages in ((el.train, pair.fresh_train, steps), (el.evaluate, pair.fresh_eval, evals)):
        for tag, stage, plain, where in stages:
            before = lo.snapshot(eng)
            stage(eng)
            assert (eng.in_slot, eng.in_kind[eng.in_slot]) == where, tag
            _same(run(eng, N), ref(before, plain or stage), life.family, N, tag)
    assert {k for k in eng._plans if k[0] == N} == {(N, 0, 'u8'), (N, 0, 'nhwc'), (N, 1, 'u8'), (N, 1, 'nhwc')}
    assert set(fresh._plans) == {(N, 0, 'u8'), (N, 0, 'nhwc')}
    eng.load_input_nchw(life.xs[0][:N].contiguous())                                   # the slot the other scenarios find: 0, dense
    assert (eng.in_slot, eng.in_kind[0]) == (0, 'nhwc')


# ------------------------------------------------------------------------------------------------ the fp32 anchor
def _oracle_loss(out, y):
    if isinstance(out, tuple):
        return F.cross_entropy(out[0], y) + 0.4 * F.cross_entropy(out[1], y)
    return F.cross_entropy(out, y)


@ALL
def test_partial_step_and_eval_meet_the_north_star_tolerances_in_fp32(pair):
    """the partial-batch train step and the eval behind it on a dirty fp32 engine of capacity B against oracle/tv_models with fp32
    storage, at exactly the tolerances of test_gpu_model.py::test_fp32_mode_meets_the_north_star_tolerance: logits (main and
    auxiliary) within 1e-3 rel, the loss within 1e-4 rel.  inception_v3 at N = 1 trains BatchNorms over a single value, for which torch
    has no answer (it raises): the anchor is skipped for that case, and only for it -- the case asserts the refusal instead."""
    life, N = pair.life, pair.N
    hip, snap, ora = life.anchor()
    eng = hip.engine
    incep = life.family == 'inception_v3'
    x0, y0, xe, ye = life.xs_cpu[0][:N], life.ys[0][:N], life.xs_cpu[2][:N], life.ys[2][:N]
    lo.restore(eng, snap)
    ora.load_state_dict({k: v.detach().cpu().clone() for k, v in hip.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(13)
    if incep:
        m = torch.rand(life.B, 2048, generator=g) > 0.5
        eng.external_mask, ora.dropout_mask = m.cuda(), m[:N]
    elif life.family == 'squeezenet1_1':
        m = torch.rand(life.B, 512, 13, 13, generator=g) > 0.5
        eng.external_mask = {'classifier.0': m.permute(0, 2, 3, 1).reshape(life.B, -1).contiguous().cuda()}
        ora.dropout_masks = {'classifier.0': m[:N]}
    ora.train()
    if incep and N == 1:
        with pytest.raises(ValueError, match='more than 1 value per channel'), torch.no_grad():
            ora(x0)
        eng.external_mask = None
        return
    with torch.no_grad():
        out_o = ora(x0)
    el.poison(eng, N)
    el.stage_dense(eng, N, life.xs[0], life.ys[0], 1)
    got = el.train(eng, N)
    eng.external_mask = None
    main = [h for h in eng.heads if not h.aux][0]
    lo_main = out_o.logits if incep else out_o
    r = rel(got[main.name + '.logits'].cpu(), lo_main)
    loss_o = float(_oracle_loss(out_o, y0))
    print(life.family, N, 'fp32 partial step: train logits rel %.2e, loss %.6f vs %.6f' % (r, float(got['loss']), loss_o))
    assert r < 1e-3
    if incep:
        aux = [h for h in eng.heads if h.aux][0]
        assert rel(got[aux.name + '.logits'].cpu(), out_o.aux_logits) < 1e-3
    assert abs(float(got['loss']) - loss_o) < 1e-4 * abs(loss_o)
    ora.load_state_dict({k: v.detach().cpu().clone() for k, v in hip.state_dict().items()}, strict=True)
    ora.eval()
    with torch.no_grad():
        eo = ora(xe)
    el.stage_dense(eng, N, life.xs[2], life.ys[2], 1)
    ev = el.evaluate(eng, N)
    r = rel(ev[main.name + '.logits'].cpu(), eo)
    loss_o = float(F.cross_entropy(eo, ye))
    print(life.family, N, 'fp32 eval behind it: logits rel %.2e, loss %.6f vs %.6f' % (r, float(ev['loss']), loss_o))
    assert r < 1e-3
    assert abs(float(ev['loss']) - loss_o) < 1e-4 * abs(loss_o)


# ------------------------------------------------------------------------------------------------ 8: refusals change nothing
@ALL
def test_refusals_change_nothing(pair):
    """plan(N > max_batch), mix_batch without mix, use_prefetched with nothing staged and a plan used after a dispatch switch changed all
    raise, and leave step_count, dropout_calls, nbt, loss_sum, in_slot, packed, eval_stats_ready and the keys of _plans alone; the next
    legal step has the reference bits.  (train_step beyond train_batch on an inference engine: the workspace test below.)"""
    from ifcb_classifier_amd import engine as engine_mod
    life, eng, N = pair.life, pair.eng, pair.N
    lo.restore(eng, life.snap)
    el.poison(eng, N)
    el.stage_dense(eng, N, life.xs[0], life.ys[0], 1)
    eng.plan(N)
    before = el.host_state(eng)
    with pytest.raises(RuntimeError, match='exceeds the engine capacity'):
        eng.plan(life.B + 1)
    with pytest.raises(RuntimeError, match='exceeds the engine capacity'):
        eng.forward_eval(life.B + 1)
    with pytest.raises(RuntimeError, match='built without mix=True'):
        eng.mix_batch(N, 0.5)
    assert eng.prefetched is None
    with pytest.raises(RuntimeError, match='nothing was prefetched'):
        eng.use_prefetched()
    switch = engine_mod._DISPATCH_SWITCHES[0]
    with mock.patch.dict(os.environ, {switch: '0' if os.environ.get(switch) != '0' else '1'}):
        with pytest.raises(RuntimeError, match='kernel-dispatch switch'):
            eng.plan(N)
        with pytest.raises(RuntimeError, match='kernel-dispatch switch'):
            eng.train_step(N)
        with pytest.raises(RuntimeError, match='kernel-dispatch switch'):
            eng.forward_eval(N)
    torch.cuda.synchronize()
    assert not el.host_state_changes(before, el.host_state(eng))
    _same(el.train(eng, N), pair.ref('train'), life.family, N, 'the next legal step')
