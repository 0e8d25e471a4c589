"""Every combination of the TRAIN options on the host: Engine(plan_only=True) refuses exactly the illegal ones, and the loss and
optimizer ops of every legal one carry each operand in the slot include/ifcbk.h names for it (tests/option_matrix.py has the tables
and the decoders, written from the header and not from plan.py).

Families: resnet18 (one head), inception_v3 (an auxiliary head: two train loss ops, weights 1.0 and 0.4, the second accumulating) and
squeezenet (channel padding inside the flat buffer).  32 loss combinations (14 legal) and 24 optimizer combinations at dp_world 1 and 2,
per family.

The IFCBK_EINVAL refusals of the library for the same four pairs, op by op, need a device: tests/test_gpu_option_matrix.py holds them.
Nothing here launches anything."""
import pytest

import ema_bounds as eb
import option_matrix as om
from ifcb_classifier_amd import _lib, graph
from ifcb_classifier_amd.engine import Engine

MODELS = ('resnet18', 'inception_v3', 'squeezenet')
N = 2
MAX_NORM = 0.75
Z = om.f32_bits(0.0)


def test_the_tables_have_the_sizes_the_prose_gives():
    assert len(om.LOSS_COMBOS) == 32 and len(om.LEGAL_LOSS) == 14 and len(om.OPT_COMBOS) == 24
    assert sorted(om.loss_id(c) for c in om.LEGAL_LOSS if c['focal']) == ['cw+focal', 'focal']
    assert len({om.loss_id(c) for c in om.LOSS_COMBOS}) == 32 and len({om.opt_id(c) for c in om.OPT_COMBOS}) == 24
    # an illegal combination breaks one of the four pairs, a legal one none
    assert all(bool(om.violated(c)) != om.legal(c) for c in om.LOSS_COMBOS)
    assert {pr for c in om.LOSS_COMBOS for pr in om.violated(c)} == set(om.ILLEGAL_PAIRS)


def _expected_loss(eng, combo, h, train):
    aux = train and h.aux
    return dict(kind=_lib.OP_SOFTMAX_XENT_W if combo['cw'] else _lib.OP_SOFTMAX_XENT, accumulate=1 if aux else 0,
                logits=h.logits.data_ptr(), target=eng.target.data_ptr(), loss=eng.loss.data_ptr(), dlogits=h.dlogits.data_ptr() if train else 0,
                class_weight=eng.class_weight.data_ptr() if combo['cw'] else 0,
                lam=eng.mix_lam[eng.in_slot].data_ptr() if train and combo['mix'] else 0,
                teacher=eng.teacher_logits.data_ptr() if train and combo['distill'] else 0,
                N=N, NC=om.NC, weight=om.f32_bits(0.4 if aux else 1.0), smoothing=om.f32_bits(om.SMOOTHING) if combo['ls'] else Z,
                gamma=om.f32_bits(om.GAMMA) if combo['focal'] else Z,
                alpha=om.f32_bits(om.DISTILL[0]) if train and combo['distill'] else Z,
                temperature=om.f32_bits(om.DISTILL[1]) if train and combo['distill'] else Z)


@pytest.mark.parametrize('combo', om.LOSS_COMBOS, ids=om.loss_id)
@pytest.mark.parametrize('model', MODELS)
def test_loss_combination(model, combo):
    kw = om.loss_kwargs(combo)
    bad = om.violated(combo)
    if bad:
        with pytest.raises(ValueError) as ei:
            Engine(graph.build(model, om.NC), max_batch=N, plan_only=True, **kw)
        msg = str(ei.value)
        assert any(om.ARG_NAMES[a] in msg and om.ARG_NAMES[b] in msg for a, b in bad), (om.loss_id(combo), msg)
        return
    eng = Engine(graph.build(model, om.NC), max_batch=N, plan_only=True, **kw)
    main = [h for h in eng.heads if not h.aux]
    auxs = [h for h in eng.heads if h.aux]
    assert len(main) == 1 and len(auxs) == (1 if model == 'inception_v3' else 0)
    assert (eng.class_weight is not None) == combo['cw'] and eng.mix == combo['mix'] and (eng.distill is not None) == combo['distill']
    if combo['cw']:
        assert eng.class_weight.tolist() == list(om.CLASS_WEIGHTS)
    kind = _lib.OP_SOFTMAX_XENT_W if combo['cw'] else _lib.OP_SOFTMAX_XENT
    other = _lib.OP_SOFTMAX_XENT if combo['cw'] else _lib.OP_SOFTMAX_XENT_W
    for slot in (0, 1):                                   # (the factors of a mixed batch and the targets are per input slot)
        eng._select_slot(slot)
        pl = eng.plan(N)
        got = [om.decode_loss_op(pl.loss.arr[k]) for k in range(pl.loss.n)]
        want = [_expected_loss(eng, combo, h, True) for h in main + auxs]
        assert got == want, (model, om.loss_id(combo), slot)
        if combo['mix']:
            assert got[0]['lam'] != eng.mix_lam[1 - slot].data_ptr()
        assert pl.eval_loss.n == 1
        ev = om.decode_loss_op(pl.eval_loss.arr[0])
        assert ev == _expected_loss(eng, combo, main[0], False), (model, om.loss_id(combo), slot)
        assert ev['dlogits'] == 0 and ev['lam'] == 0 and ev['teacher'] == 0 and ev['alpha'] == Z and ev['temperature'] == Z
        # the same ops inside the fused step and the data-parallel programs
        for name in ('step', 'fwd_loss', 'fwd_bwd'):
            prog = getattr(pl, name)
            assert [om.decode_loss_op(prog.arr[k]) for k in prog.find(kind)] == want, (model, om.loss_id(combo), slot, name)
            assert prog.find(other) == []


def _expected_opt(eng, combo, lo, n, step, grad_scale, ema_w):
    sgd = eng.optimizer == 'sgd'
    at = lambda t: t.data_ptr() + 4 * lo
    d = dict(kind=_lib.OP_SGD if sgd else _lib.OP_ADAM, accumulate=0, P=at(eng.P), G=at(eng.G), E=at(eng.E) if combo['ema'] else 0,
             clip_state=eng.clip_state.data_ptr() if combo['clip'] else 0, n=n, step=step, lr=om.f32_bits(eng.lr),
             weight_decay=om.f32_bits(om.WEIGHT_DECAY) if combo['wd'] else Z, grad_scale=om.f32_bits(grad_scale),
             ema_w=om.f32_bits(ema_w) if combo['ema'] else Z, max_norm=om.f32_bits(MAX_NORM) if combo['clip'] else Z)
    if sgd:
        d.update(M=at(eng.M) if combo['opt'][1] else 0, momentum=om.f32_bits(combo['opt'][1]))
    else:
        d.update(M=at(eng.M), V=at(eng.V), beta1=om.f32_bits(0.9), beta2=om.f32_bits(0.999), eps=om.f32_bits(1e-8))
    return d


def _opt_ops(eng, pl):
    """-> {program: [its optimizer ops]}"""
    kind = _lib.OP_SGD if eng.optimizer == 'sgd' else _lib.OP_ADAM
    assert pl.step.find(kind) == list(pl.step_adam_idxs) and pl.adam.find(kind) == [0] and pl.adam.n == 1 and pl.adam_pack.find(kind) == [0]
    return {'adam': [pl.adam.arr[0]], 'adam_pack': [pl.adam_pack.arr[0]], 'step': [pl.step.arr[j] for j in pl.step_adam_idxs]}


def _check_opt(eng, combo, ops, step, grad_scale, ema_w):
    """every op decodes to the slice of the flat buffers its P names; -> the slices [(lo, hi)]"""
    cover = []
    for op in ops:
        d = om.decode_opt_op(op, eng.optimizer)
        lo = (d['P'] - eng.P.data_ptr()) // 4
        assert d['P'] == eng.P.data_ptr() + 4 * lo and 0 <= lo and lo + d['n'] <= eng.nparam_padded and d['n'] > 0
        assert d == _expected_opt(eng, combo, lo, d['n'], step, grad_scale, ema_w), (om.opt_id(combo), lo)
        cover.append((lo, lo + d['n']))
    return cover


@pytest.mark.parametrize('world', (1, 2))
@pytest.mark.parametrize('combo', om.OPT_COMBOS, ids=om.opt_id)
@pytest.mark.parametrize('model', MODELS)
def test_optimizer_combination(model, combo, world):
    eng = Engine(graph.build(model, om.NC), max_batch=N, plan_only=True, dp_world=world, **om.opt_kwargs(combo, MAX_NORM))
    assert eng.dp_world == world and (eng.E is not None) == combo['ema'] and (eng.clip_state is not None) == combo['clip']
    pl = eng.plan(N)
    progs = _opt_ops(eng, pl)
    whole = [(0, eng.nparam_padded)]
    for name, ops in progs.items():
        cover = sorted(_check_opt(eng, combo, ops, 1, 1.0, 0.0))
        if name != 'step' or combo['clip']:
            assert cover == whole, (name, cover)
        else:
            # the buckets tile the flat buffer; each carries the slice of E at the element offset of its slice of P (_check_opt)
            assert cover[0][0] == 0 and cover[-1][1] == eng.nparam_padded and all(a[1] == b[0] for a, b in zip(cover, cover[1:])), cover
            if model != 'squeezenet':
                assert len(cover) > 1
    if combo['clip']:
        assert eng.clip_state.data_ptr() % 16 == 0 and len(pl.step_adam_idxs) == 1
    # the per-step scalars: the gradient scale and the weight of the average land in their own slots, everything else keeps its bits
    eng.step_count = 3
    eng._ema_begin_step()
    w = eb.weight(om.EMA_DECAY, 1) if combo['ema'] else 0.0
    if combo['ema']:
        assert eng._ema_w == w and 0.0 < w < 1.0 and w != MAX_NORM
    for name, ops in progs.items():
        for op in ops:
            eng._set_update(op, grad_scale=0.5)
        _check_opt(eng, combo, ops, 3, 0.5, w)
