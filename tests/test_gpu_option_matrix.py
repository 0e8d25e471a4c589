"""Every legal combination of the TRAIN options on the device, held to the float64 twins of tests/option_matrix.py (whose docstring
has the composition of the bounds): the loss matrix teacher-forced on the engine's own logits, with the results of the three
combinations that have near neighbours also held OUT of the neighbours' bounds; the optimizer matrix from snapshots in front of the
second of two split steps; the ways a step is launched under all options at once, bit for bit; two data-parallel replicas with
clipping and an average; and the library's refusal of the four illegal pairs, op by op.

Shapes: resnet18, 7 classes, batch 4, fp32, S = 224 and inception_v3 at batch 2 (the aux head), squeezenet at batch 2 (channel
padding inside the flat buffer): the smallest at which the plans have their full op lists (tests/test_gpu_clip_engine.py)."""
import math

import numpy as np
import pytest
import torch

import clip_cases as cc
import ema_bounds as eb
import loss_bounds as lb
import op_bounds as ob
import option_matrix as om

pytestmark = pytest.mark.gpu

SHAPES = {'resnet18': (4, 224), 'inception_v3': (2, 299), 'squeezenet': (2, 224)}
GUARD = 12345.0


class Rig:
    """engines by (model, options), built on first use and closed with the module; the fixed-seed inputs of three steps per model"""

    def __init__(self):
        self.engines, self.inputs, self.memo = {}, {}, {}

    def engine(self, model, **kw):
        from ifcb_classifier_amd import graph
        from ifcb_classifier_amd.engine import Engine
        key = (model, repr(sorted(kw.items())))
        if key not in self.engines:
            self.engines[key] = Engine(graph.build(model, om.NC, pretrained=False), device=0, max_batch=SHAPES[model][0], dtype='fp32', **kw)
        eng = self.engines[key]
        if eng.in_slot != 0:
            eng._select_slot(0)
        om.reset(eng)
        return eng

    def data(self, model):
        """per step k: x, targets, lam (one row at exactly 1.0, the others inside (0, 1)), a non-empty cut box, teacher logits"""
        if model not in self.inputs:
            B, S = SHAPES[model]
            g = torch.Generator().manual_seed(9)
            steps = []
            for k in range(3):
                x = torch.rand(B, 3, S, S, generator=g).cuda()
                y = torch.randint(0, om.NC, (B,), generator=g)
                lam = torch.rand(B, generator=g) * 0.8 + 0.1
                lam[k % B] = 1.0
                z = torch.randn(B, om.NC, generator=g) * 4.0
                box = (S // 4 + k, S // 2 + k, S // 3, S // 3 + 40 + k)
                steps.append(dict(x=x, y=y, lam=lam, z=z, box=box))
            self.inputs[model] = steps
        return self.inputs[model]

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines.clear()


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    yield r
    r.close()


def _load(eng, d):
    B = d['y'].numel()
    eng.load_input_nchw(d['x'])
    eng.target[:B].copy_(d['y'])
    if eng.mix:
        eng.mix_batch(B, d['lam'].cuda(), d['box'])
    if eng.distill is not None:
        eng.teacher_logits[:B].copy_(d['z'])
    return B


def _fwd_bwd(eng, d):
    B = _load(eng, d)
    pl = eng.forward_train(B)
    eng.run(pl.loss)
    eng.backward(B)
    return B


# ------------------------------------------------------------------------------------------------------ a. loss matrix
NEAR = ('cw+ls+mix', 'cw+ls+distill', 'cw+focal')


def _loss_case(rig, model, combo):
    d = rig.data(model)[0]
    eng = rig.engine(model, **om.loss_kwargs(combo))
    B = _load(eng, d)
    pl = eng.forward_train(B)
    eng.run(pl.loss)
    torch.cuda.synchronize()
    main = [h for h in eng.heads if not h.aux][0]
    auxs = [h for h in eng.heads if h.aux]
    args = dict(target=d['y'], lam=d['lam'], teacher=d['z'])
    name = '%s %s' % (model, om.loss_id(combo))
    lm = main.logits[:B].cpu()
    want = om.loss_reference(combo, lm, weight=1.0, **args)
    got_loss = eng.loss.cpu().clone()
    worst = ob.check_dict(name + ' main', {'dlogits': main.dlogits[:B].cpu()}, want)
    wants = [(main, lm, 1.0, want)]
    if auxs:
        la = auxs[0].logits[:B].cpu()
        want_aux = om.loss_reference(combo, la, weight=0.4, old_loss=float(want['loss'][0]), **args)
        worst = max(worst, ob.check_dict(name + ' aux', {'dlogits': auxs[0].dlogits[:B].cpu()}, want_aux))
        # the aux op accumulates into the scalar the main op stored
        worst = max(worst, ob.check_dict(name + ' main + aux', {'loss': got_loss}, lb.head_sum(want, want_aux)))
        assert float(got_loss) != float(want['loss'][0][0].float())
        wants.append((auxs[0], la, 0.4, want_aux))
    else:
        worst = max(worst, ob.check_dict(name, {'loss': got_loss}, want))
    print('%s: worst err / bound %.3f' % (name, worst))
    if om.loss_id(combo) in NEAR:
        # a kernel that read a NULL or a zero in one operand's slot computes a neighbour: the two references lie further apart than
        # twice their bounds for these inputs, and the device's result is outside the neighbour's bound
        nbs = om.neighbours(combo)
        assert len(nbs) == len(om.loss_id(combo).split('+'))
        for h, lg, wgt, w_own in wants:
            for nb in nbs:
                w_nb = om.loss_reference(nb, lg, weight=wgt, **args)
                assert om.apart(w_own, w_nb), (name, om.loss_id(nb))
                r = ob.check_dict('%s as %s' % (name, om.loss_id(nb)), {'dlogits': h.dlogits[:B].cpu()}, w_nb, raise_=False)
                assert r > 1.0, (name, h.name, om.loss_id(nb), r)
    # the validation loss of the same logits: one target, no mix, no teacher, no gradient
    before = [h.dlogits.clone() for h in eng.heads]
    eng.run(pl.eval_loss)
    torch.cuda.synchronize()
    ev = om.loss_reference(om.eval_combo(combo), lm, d['y'], weight=1.0)
    ob.check_dict(name + ' eval', {'loss': eng.loss.cpu()}, ev)
    assert all(om.same(a, h.dlogits) for a, h in zip(before, eng.heads))
    if combo['mix'] or combo['distill']:
        assert om.apart(ev, want, 'loss') and float(eng.loss) != float(got_loss)


@pytest.mark.parametrize('combo', om.LEGAL_LOSS, ids=om.loss_id)
def test_loss_matrix_resnet18(rig, combo):
    _loss_case(rig, 'resnet18', combo)


@pytest.mark.parametrize('case', NEAR + ('plain',))
def test_loss_matrix_inception_v3_both_heads(rig, case):
    _loss_case(rig, 'inception_v3', om.loss_combo(case))


# ------------------------------------------------------------------------------------------------------ b. optimizer matrix
OPT_SNAP = ('P', 'G', 'M', 'V', 'E', 'clip_state')


def _snap(eng, keys):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).clone() for k in keys if getattr(eng, k, None) is not None}


def _max_norm(rig, model):
    """half the float64 norm of the unclipped engine's first gradient: the bound bites"""
    if ('max_norm', model) not in rig.memo:
        eng = rig.engine(model)
        _fwd_bwd(eng, rig.data(model)[0])
        torch.cuda.synchronize()
        total64, _ = cc.torch_clip([eng.gviews[k] for k in eng.gviews], 1.0, dtype=torch.float64)
        assert 0 < total64 < math.inf
        rig.memo['max_norm', model] = float(np.float32(total64 / 2))
    return rig.memo['max_norm', model]


def _plain_update(eng, before, coef, step):
    """the typed entry point without clipping on copies of the snapshot, the gradient scaled by the device's coefficient: what the
    clipped update must equal bit for bit (tests/test_gpu_grad_clip.py, at kernel level) -> {'P', 'M', 'V', 'E'}"""
    from ifcb_classifier_amd import _lib
    t = {k: v.clone() for k, v in before.items()}
    P, st, n = _lib.ptr, _lib.cur_stream(), eng.nparam_padded
    gs = float(np.float32(1.0) * np.float32(coef))
    if eng.optimizer == 'sgd':
        eng.ctx.call('ifcbk_sgd_ema_flat', P(t['P']), P(t['G']), P(t['M']) if eng.momentum else None, P(t.get('E')), n, eng.lr, eng.momentum,
                     eng.weight_decay, gs, eng._ema_w, st)
    else:
        eng.ctx.call('ifcbk_adam_ema_flat', P(t['P']), P(t['G']), P(t['M']), P(t['V']), P(t.get('E')), n, eng.lr, eng.betas[0], eng.betas[1],
                     eng.eps, eng.weight_decay, step, gs, eng._ema_w, st)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize('combo', om.OPT_COMBOS, ids=om.opt_id)
def test_optimizer_matrix_resnet18(rig, combo):
    model = 'resnet18'
    mx = _max_norm(rig, model)
    eng = rig.engine(model, **om.opt_kwargs(combo, mx))
    blocks = cc.geometry(eng.ctx.lib)[0]
    name = 'resnet18 ' + om.opt_id(combo)
    assert (eng.E is None) == (not combo['ema']) and (eng.clip_state is None) == (not combo['clip'])
    for k in range(2):
        B = _fwd_bwd(eng, rig.data(model)[k])
        before = _snap(eng, OPT_SNAP)
        eng.adam_step(B)
        torch.cuda.synchronize()
        assert eng.step_count == k + 1 and (not combo['ema'] or eng.ema_updates == k + 1)
        if combo['clip']:
            norm, coef = om.check_clip_state('%s step %d' % (name, k + 1), eng, before, blocks)
            assert coef < 1.0 and float(eng.clip_state[3]) == k + 1
            if k == 0:
                assert 0.49 < coef < 0.51
    # the second update, from the snapshot in front of it
    worst = om.check_optimizer(name, eng, before, 2, blocks)
    print('%s: worst err / bound %.3f' % (name, worst))
    assert not om.same(eng.P, before['P'])
    if combo['clip']:
        twin = _plain_update(eng, before, float(eng.clip_state[1]), 2)
        for key in ('P', 'M', 'V') + (('E',) if combo['ema'] else ()):
            assert om.same(getattr(eng, key), twin[key]), (name, key)


def test_squeezenet_padded_rows_keep_their_bits(rig):
    model = 'squeezenet'
    combo = dict(opt=('adam', 0.0), wd=True, ema=True, clip=True)
    eng = rig.engine(model, **om.opt_kwargs(combo, 1.0))
    assert any(getattr(n, 'kind', '') == 'cb' and n.K != n.K_real for n in eng.net.nodes)
    pad = ~om.real_mask(eng)
    assert int(pad.sum()) > 4
    B = _fwd_bwd(eng, rig.data(model)[0])
    before = _snap(eng, OPT_SNAP)
    assert bool((before['G'].cpu()[pad] == 0).all())
    eng.adam_step(B)
    torch.cuda.synchronize()
    blocks = cc.geometry(eng.ctx.lib)[0]
    om.check_clip_state('squeezenet', eng, before, blocks)
    om.check_optimizer('squeezenet ' + om.opt_id(combo), eng, before, 1, blocks)
    for key in ('P', 'E', 'M', 'V'):
        # (E restarts from P at the step's start: its padded rows are P's)
        src = before['P'] if key == 'E' else before[key]
        assert om.same(getattr(eng, key).cpu()[pad], src.cpu()[pad]), key
    assert not om.same(eng.P, before['P'])


# ------------------------------------------------------------------------------------------------------ c. launch modes
ALL_ON = {
    'cw+ls+mix/adam-wd-ema-clip': ('cw+ls+mix', dict(opt=('adam', 0.0), wd=True, ema=True, clip=True)),
    'cw+ls+distill/sgd0.9-ema-clip': ('cw+ls+distill', dict(opt=('sgd', 0.9), wd=False, ema=True, clip=True)),
    'cw+focal/adam-ema-clip': ('cw+focal', dict(opt=('adam', 0.0), wd=False, ema=True, clip=True)),
}
MODE_KEYS = ('P', 'M', 'V', 'E', 'ERB', 'RB', 'nbt', 'loss', 'clip_state')


def _mode_steps(rig, model, eng, mode):
    """three steps from the reset state; graph mode loads steps 2 and 3 into the other input slot (its mix factors are another array)
    -> the state after each step"""
    om.reset(eng)
    outs = []
    for k, d in enumerate(rig.data(model)):
        if mode == 'graph':
            eng._select_slot(0 if k == 0 else 1)
        B = d['y'].numel()
        if mode == 'split':
            _fwd_bwd(eng, d)
            eng.adam_step(B)
        else:
            _load(eng, d)
            if mode == 'plain':
                eng.train_step(B)
            elif mode == 'ev':
                eng.train_step(B, ev_slot=0)
            elif mode == 'graph':
                eng.graph_train = True
                try:
                    pl = eng.train_step(B)
                    assert 'fwd_bwd' in pl.graphs
                finally:
                    eng.graph_train = False
            else:
                raise KeyError(mode)
        outs.append(_snap(eng, MODE_KEYS))
    if eng.in_slot != 0:
        eng._select_slot(0)
    return outs


@pytest.mark.parametrize('case', sorted(ALL_ON))
@pytest.mark.parametrize('model', ('resnet18', 'inception_v3'))
def test_launch_modes_under_all_options(rig, model, case):
    loss_s, oc = ALL_ON[case]
    eng = rig.engine(model, **dict(om.loss_kwargs(om.loss_combo(loss_s)), **om.opt_kwargs(oc, _max_norm(rig, model))))
    modes = ['plain', 'ev', 'split'] + (['graph'] if (model, case) == ('resnet18', 'cw+ls+mix/adam-wd-ema-clip') else [])
    ref = _mode_steps(rig, model, eng, 'plain')
    assert set(ref[0]) == set(MODE_KEYS)
    assert not om.same(ref[0]['P'], ref[1]['P']) and not om.same(ref[1]['P'], ref[2]['P']) and bool(torch.isfinite(ref[2]['P']).all())
    assert [float(s['clip_state'][3]) for s in ref] == [1.0, 2.0, 3.0]            # every step was clipped
    for mode in modes[1:]:
        got = _mode_steps(rig, model, eng, mode)
        for k in range(3):
            bad = [key for key in MODE_KEYS if not om.same(got[k][key], ref[k][key])]
            assert not bad, (model, case, mode, 'step %d' % (k + 1), bad)


# ------------------------------------------------------------------------------------------------------ d. data parallel
DP_OPTIONS = {
    'adam-wd-ema-clip': dict(weight_decay=om.WEIGHT_DECAY, ema_decay=om.EMA_DECAY, clip_grad=1e-3),
    'sgd-momentum-ema-clip': dict(optimizer='sgd', momentum=0.9, lr=om.SGD_LR, ema_decay=om.EMA_DECAY, clip_grad=1e-3),
}


@pytest.mark.parametrize('case', sorted(DP_OPTIONS))
def test_two_replicas_clip_and_average_by_the_same_bits(case):
    import dp_twin
    B, S = SHAPES['resnet18']
    tw = dp_twin.Twin('resnet18', B, S, nc=om.NC, dtype='fp32', **DP_OPTIONS[case])
    try:
        tw.reset()
        local = tw.local(0)
        before = [dict(_snap(e, ('P', 'M', 'V', 'clip_state')), step_count=e.step_count) for e in tw.engs]
        tw.ddp_step(0, local)
        a, b = tw.engs
        for key in ('P', 'M', 'V', 'E'):
            assert om.same(getattr(a, key), getattr(b, key)), (case, key)
        assert om.same(a.clip_state[:2], b.clip_state[:2])                     # the same norm and coefficient bits, no collective
        assert not om.same(a.P, before[0]['P']) and bool(torch.isfinite(a.P).all())
        summed = (local[0]['G'] + local[1]['G']).cpu()                         # what each replica holds behind the exchange
        real = om.real_mask(a)
        assert bool((summed[~real] == 0).all())
        ref = cc.ref_norm(summed[real], 0.5)                                   # the norm of the averaged gradient
        norm, coef = a.grad_clip_stats()[:2]
        assert abs(norm - ref) <= cc.norm_bound(a.nparam_padded, cc.geometry(a.ctx.lib)[0], ref, 0.5)
        assert coef < 1.0 and cc.f32_bits(coef) == cc.f32_bits(cc.host_coef(np.float32(norm), 1e-3))
        # the update: the plain entry point on the summed gradient with grad_scale = fl(1/2 * coef), bit for bit
        t = dict(before[0], G=(local[0]['G'] + local[1]['G']))
        from ifcb_classifier_amd import _lib
        P, st, n = _lib.ptr, _lib.cur_stream(), a.nparam_padded
        gs = float(np.float32(0.5) * np.float32(coef))
        if a.optimizer == 'sgd':
            a.ctx.call('ifcbk_sgd_ema_flat', P(t['P']), P(t['G']), P(t['M']), None, n, a.lr, a.momentum, a.weight_decay, gs, 0.0, st)
        else:
            a.ctx.call('ifcbk_adam_ema_flat', P(t['P']), P(t['G']), P(t['M']), P(t['V']), None, n, a.lr, a.betas[0], a.betas[1], a.eps,
                       a.weight_decay, before[0]['step_count'] + 1, gs, 0.0, st)
        torch.cuda.synchronize()
        for key in ('P', 'M') + (() if a.optimizer == 'sgd' else ('V',)):
            assert om.same(getattr(a, key), t[key]), (case, key)
        # the average: every replica's own E from its P, the same bits in both; the running statistics stay per rank
        w = eb.weight(om.EMA_DECAY, a.ema_updates)
        assert a._ema_w == w == b._ema_w and not om.same(a.E, a.P) and not om.same(a.ERB, b.ERB)
    finally:
        tw.close()


# ------------------------------------------------------------------------------------------------------ e. refusals
REFUSED = {
    'focal x smoothing': dict(f=(1.0, 0.1, 2.0)),
    'focal x mix': dict(f=(1.0, 0.0, 2.0), mix=True),
    'distill x focal': dict(f=(1.0, 0.0, 2.0, 0.3, 4.0), teacher=True),
    'distill x mix': dict(f=(1.0, 0.1, 0.0, 0.3, 4.0), teacher=True, mix=True),
}


@pytest.mark.parametrize('weights', ('none', 'random'))
@pytest.mark.parametrize('pair', sorted(REFUSED))
def test_the_library_refuses_the_four_pairs_and_launches_nothing(ctx, pair, weights):
    import distill_cases as dc
    from ifcb_classifier_amd import _lib
    from ifcb_classifier_amd.engine import OpList, Program
    N, NC = 7, 5
    l, t, z, cw = dc.inputs(N, NC, weights)
    ld, td, zd = l.cuda(), t.cuda(), z.cuda()
    cwd = None if cw is None else cw.cuda()
    lam = torch.full((N,), 0.5, device='cuda')
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    P, st = _lib.ptr, _lib.cur_stream()
    kind = _lib.OP_SOFTMAX_XENT if cw is None else _lib.OP_SOFTMAX_XENT_W

    def prog(f, teacher=False, mix=False):
        ops = OpList()
        ops.add(kind, 'loss', p=(P(ld), P(td), P(loss), P(dl), P(cwd), P(lam) if mix else None, P(zd) if teacher else None), i=(N, NC), f=f)
        return Program(ops)
    bad = prog(**REFUSED[pair])
    with pytest.raises(RuntimeError, match=r'\(-1\)'):                         # (-1: IFCBK_EINVAL)
        ctx.run_program(bad.arr, bad.n, st)
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    # each half of the pair alone is an op the library runs
    spec = REFUSED[pair]
    f = spec['f'] + (0.0,) * (5 - len(spec['f']))
    halves = [dict(f=(f[0], 0.0, f[2], 0.0, 0.0))] if f[2] else []
    if spec.get('teacher'):
        halves.append(dict(f=(f[0], f[1], 0.0, 0.3, 4.0), teacher=True))
    if spec.get('mix'):
        halves.append(dict(f=(f[0], f[1], 0.0), mix=True))
    if pair == 'focal x smoothing':
        halves.append(dict(f=(f[0], f[1], 0.0)))
    assert len(halves) == 2
    for h in halves:
        loss.fill_(GUARD)
        dl.fill_(GUARD)
        good = prog(**h)
        ctx.run_program(good.arr, good.n, st)
        torch.cuda.synchronize()
        assert float(loss) != GUARD and bool(torch.isfinite(dl).all()) and not bool((dl == GUARD).any())
