"""The TRAIN options taken together: the tables of every combination, decoders of the loss and optimizer ops, and the float64 twins
of one step under a combination.  Helpers only; tests/test_option_matrix_cpu.py (plans) and tests/test_gpu_option_matrix.py (device)
run them.

Axes.  Loss side: class weights (none / 7 weights) x label_smoothing (0 / 0.1) x focal_gamma (0 / 2.0) x mix (off / on) x distill
(none / (0.3, 4.0)): 32 combinations.  Optimizer side: (adam | sgd momentum 0.9 | sgd momentum 0) x weight_decay (0 / 1e-2) x
ema_decay (none / 0.9) x clip_grad (none / a bound): 24 combinations.

`legal` is written from the prose of include/ifcbk.h (IFCBK_OP_SOFTMAX_XENT_W: "f[1] != 0 together with f[2] != 0 is IFCBK_EINVAL",
"an array [p[5]] together with f[2] != 0 is IFCBK_EINVAL", "an array [p[6]] together with f[2] != 0 or with p[5] is IFCBK_EINVAL") and
of engine.check_distill ("Distillation combines with neither focal loss nor a mixed batch"), not from the engine's code: four
illegal pairs, focal x smoothing, focal x mix, distill x focal, distill x mix.  That leaves 14 loss combinations (2 with focal: with
or without class weights; 12 without: class weights x smoothing x {none, mix, distill}); every optimizer combination is legal.

`decode_loss_op` / `decode_opt_op` name the operands of an ifcbk_op from the op-table comments of include/ifcbk.h alone and refuse
an op in which a slot behind the last named one is not zero.

The float64 twins are assembled from the modules the kernel tests use; nothing here is a new formula or a new constant.

  loss (`loss_reference`): the kernel the header's dispatch names for the op -- p[6] -> distill_cases.bounds, p[5] -> mix_cases.xent_mix,
      f[2] -> loss_focal_bounds.xent_focal, f[1] -> loss_smooth_bounds.xent_ls, class weights -> loss_bounds.xent_w, else
      op_bounds.xent -- evaluated on the logits the engine holds (teacher-forced: the network in front of the loss is not part of
      the comparison, so its error is not part of the bound).  One stage, that module's bound.  A network with an auxiliary head
      passes two such stages into one loss scalar: loss_bounds.head_sum (the aux op's bound with old_loss = the main term, plus the
      stored main term's own error and the rounding of its store).

  optimizer (`optimizer_reference`), from snapshots of P, G, M, V, E and the clip state taken in front of the update.  The stages a
      combination passes, and the bound of each; the composed bound is their sum:
      1. clipping (if on): norm = clip_cases.ref_norm(G) within clip_cases.norm_bound; the coefficient is clip_cases.host_coef of the
         device's own norm, bit for bit; the gradient the update takes is torch.nn.utils.clip_grad_norm_ of the float64 gradient
         over the real parameter elements, rounded once (`reference_gradient`).  What the norm's bound and the roundings of the
         coefficient move the update by is `sensitivity(step, gc, scale_delta(n))`, the slack tests/test_gpu_grad_clip.py adds.
      2. the update: op_bounds.adam / op_bounds.sgd (torch's Adam / SGD with L2 weight decay) on that gradient: their bound.
      3. the average (if on): ema_bounds.update / ema_bounds.bound from E as it stood and the P the device wrote (the kernel averages
         the parameter it has just written, so stage 2's error does not enter).
      P, M, V: stage 2's bound + stage 1's slack.  E: stage 3's bound.  norm: stage 1's bound.
"""
import itertools
import math

import numpy as np
import torch

import clip_cases as cc
import distill_cases as dc
import ema_bounds as eb
import loss_bounds as lb
import loss_focal_bounds as fb
import loss_smooth_bounds as sb
import mix_cases as mc
import op_bounds as ob

NC = 7
CLASS_WEIGHTS = (0.5, 1.0, 2.0, 0.25, 1.5, 0.75, 1.25)
SMOOTHING, GAMMA, DISTILL = 0.1, 2.0, (0.3, 4.0)
WEIGHT_DECAY, EMA_DECAY = 1e-2, 0.9
SGD_LR = 0.005                                      # (tests/test_gpu_dp_world2.py's sgd rate; adam keeps the engine's default)

LOSS_KEYS = ('cw', 'ls', 'focal', 'mix', 'distill')
LOSS_COMBOS = [dict(zip(LOSS_KEYS, v)) for v in itertools.product((False, True), repeat=5)]
OPTIMIZERS = (('adam', 0.0), ('sgd', 0.9), ('sgd', 0.0))
OPT_KEYS = ('opt', 'wd', 'ema', 'clip')
OPT_COMBOS = [dict(zip(OPT_KEYS, v)) for v in itertools.product(OPTIMIZERS, (False, True), (False, True), (False, True))]

# the four pairs the header and check_distill's docstring refuse, by the names of the Engine arguments
ILLEGAL_PAIRS = (('focal', 'ls'), ('focal', 'mix'), ('distill', 'focal'), ('distill', 'mix'))
ARG_NAMES = dict(cw='class_weights', ls='label_smoothing', focal='focal_gamma', mix='mix', distill='distill')


def violated(combo):
    return [pr for pr in ILLEGAL_PAIRS if combo.get(pr[0]) and combo.get(pr[1])]


def legal(combo):
    return not violated(combo)


LEGAL_LOSS = [c for c in LOSS_COMBOS if legal(c)]
assert len(LOSS_COMBOS) == 32 and len(LEGAL_LOSS) == 14
assert len([c for c in LEGAL_LOSS if c['focal']]) == 2 and len([c for c in LEGAL_LOSS if not c['focal']]) == 12
assert len(OPT_COMBOS) == 24 and all(legal(c) for c in OPT_COMBOS)


def loss_id(c):
    return '+'.join(k for k in LOSS_KEYS if c[k]) or 'plain'


def opt_id(c):
    name = 'adam' if c['opt'][0] == 'adam' else 'sgd%g' % c['opt'][1]
    return '-'.join([name] + [k for k in ('wd', 'ema', 'clip') if c[k]])


def loss_combo(s):
    """'cw+ls+mix' -> the combination"""
    on = set() if s == 'plain' else set(s.split('+'))
    assert on <= set(LOSS_KEYS), s
    return {k: k in on for k in LOSS_KEYS}


def loss_kwargs(c):
    kw = {}
    if c['cw']:
        kw['class_weights'] = list(CLASS_WEIGHTS)
    if c['ls']:
        kw['label_smoothing'] = SMOOTHING
    if c['focal']:
        kw['focal_gamma'] = GAMMA
    if c['mix']:
        kw['mix'] = True
    if c['distill']:
        kw['distill'] = DISTILL
    return kw


def opt_kwargs(c, clip_grad=1.0):
    name, mu = c['opt']
    kw = dict(optimizer=name)
    if name == 'sgd':
        kw.update(momentum=mu, lr=SGD_LR)
    if c['wd']:
        kw['weight_decay'] = WEIGHT_DECAY
    if c['ema']:
        kw['ema_decay'] = EMA_DECAY
    if c['clip']:
        kw['clip_grad'] = clip_grad
    return kw


# ------------------------------------------------------------------------------------------------------ decoders (include/ifcbk.h)
LOSS_P = ('logits', 'target', 'loss', 'dlogits', 'class_weight', 'lam', 'teacher')
LOSS_F = ('weight', 'smoothing', 'gamma', 'alpha', 'temperature')
ADAM_P = ('P', 'G', 'M', 'V', 'E', 'clip_state')
ADAM_F = ('lr', 'beta1', 'beta2', 'eps', 'weight_decay', 'grad_scale', 'ema_w', 'max_norm')
SGD_P = ('P', 'G', 'M', 'E', 'clip_state')
SGD_F = ('lr', 'momentum', 'weight_decay', 'grad_scale', 'ema_w', 'max_norm')
NP_SLOTS, NF_SLOTS = 12, 8


def f32_bits(x):
    return cc.f32_bits(x)


def _decode(op, pnames, fnames):
    d = {'kind': int(op.kind), 'accumulate': int(op.flags) & 1}
    for k, name in enumerate(pnames):
        d[name] = int(op.p[k] or 0)
    for k, name in enumerate(fnames):
        d[name] = f32_bits(op.f[k])                   # the scalar's fp32 bits: -0.0 and 0.0, a NaN and a NaN differ
    rest = [('p[%d]' % k, op.p[k]) for k in range(len(pnames), NP_SLOTS) if op.p[k]]
    rest += [('f[%d]' % k, op.f[k]) for k in range(len(fnames), NF_SLOTS) if f32_bits(op.f[k]) != 0]
    assert not rest, 'slots behind the last named operand are not zero: %r' % (rest,)
    return d


def decode_loss_op(op):
    """an IFCBK_OP_SOFTMAX_XENT / _W op -> {kind, accumulate, the seven pointers (0 = NULL), N, NC, the five scalars as fp32 bits}"""
    d = _decode(op, LOSS_P, LOSS_F)
    d['N'], d['NC'] = int(op.i[0]), int(op.i[1])
    return d


def decode_opt_op(op, optimizer):
    """an IFCBK_OP_ADAM / IFCBK_OP_SGD op -> {kind, the pointers (0 = NULL), n, step, the scalars as fp32 bits}"""
    d = _decode(op, *((SGD_P, SGD_F) if optimizer == 'sgd' else (ADAM_P, ADAM_F)))
    d['n'], d['step'] = int(op.i[0]), int(op.i[1])
    return d


# ------------------------------------------------------------------------------------------------------ engine state
def reset(eng, seed=4321):
    """a fresh engine's state: seeded weights, zero moments, gradients, statistics, counters and clip state (the average restarts from
    P at the next step: init_weights marks it stale)"""
    eng.init_weights(seed=seed)
    eng.M.zero_()
    eng.V.zero_()
    eng.G.zero_()
    eng.RB.zero_()
    for k, v in eng.bviews.items():
        if k.endswith('running_var'):
            v.fill_(1.0)
    eng.nbt.zero_()
    eng.loss_sum.zero_()
    eng.step_count = 0
    eng.dropout_seed, eng.dropout_calls = 5, 0
    if eng.clip_state is not None:
        eng.clip_state.zero_()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def real_mask(eng):
    """True at the elements of the flat buffers that belong to a parameter tensor (False: alignment and channel padding)"""
    real = torch.zeros(eng.nparam_padded, dtype=torch.bool)
    for key, (o, n, _shape, _kind, _node) in eng.poff.items():
        real[o:o + n] = True
    return real


# ------------------------------------------------------------------------------------------------------ loss twin
def loss_reference(combo, logits, target, lam=None, teacher=None, weight=1.0, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of the kernel the header's dispatch names for `combo`, with the bound its module
    derives"""
    assert legal(combo), combo
    cw = torch.tensor(CLASS_WEIGHTS, dtype=torch.float32) if combo['cw'] else None
    eps = SMOOTHING if combo['ls'] else 0.0
    if combo['distill']:
        return dc.bounds(logits, target, teacher, cw, weight, eps, DISTILL[0], DISTILL[1], old_loss=old_loss)
    if combo['mix']:
        return mc.xent_mix(logits, target, lam, cw, weight, eps, old_loss=old_loss)
    if combo['focal']:
        return fb.xent_focal(logits, target, cw, weight, GAMMA, old_loss=old_loss)
    if combo['ls']:
        return sb.xent_ls(logits, target, cw, weight, eps, old_loss=old_loss)
    if combo['cw']:
        return lb.xent_w(logits, target, cw, weight, old_loss=old_loss)
    return ob.xent(logits, target, weight, old_loss=old_loss)


def eval_combo(combo):
    """what the validation loss op keeps of a combination: neither the mixed batch nor the teacher"""
    return dict(combo, mix=False, distill=False)


def neighbours(combo):
    """the combinations one operand short of `combo`: what a kernel reading a NULL or a zero in that operand's slot computes"""
    return [dict(combo, **{k: False}) for k in LOSS_KEYS if combo[k]]


def apart(a, b, key='dlogits'):
    """the two references of `key` differ by more than twice the two bounds somewhere"""
    (wa, ea), (wb, eb_) = a[key], b[key]
    return bool(((wa - wb).abs() > 2 * (ea + eb_)).any())


# ------------------------------------------------------------------------------------------------------ optimizer twin
def scale_delta(n, blocks):
    """how far, relatively, the device's clipped gradient g * fl(gs * coef) may lie from the reference's fl(gs * g * max / (norm + 1e-6))
    (formed in float64, rounded once): the norm's bound of tests/clip_cases.py, and one rounding each for norm + 1e-6, the reciprocal, its
    product with max_norm, the product gs * coef, the kernel's product with g and the reference's rounding"""
    return ((cc.chain(n, blocks) + 6) / 2.0 + 2.0 + 6.0) * cc.U


def reference_gradient(g, gs, mx):
    """clip_grad_norm_ on the CPU, on the float64 product grad_scale * g, rounded once to the fp32 gradient torch.optim then takes"""
    _total, (gc,) = cc.torch_clip([g.double() * float(np.float32(gs))], mx)
    return gc.float()


def sensitivity(step_fn, gc, delta, key='p'):
    """how far the float64 result moves when every gradient element moves by delta relatively, to first order, doubled: the larger of the
    two one-sided differences of the oracle, times 2"""
    w0 = step_fn(gc)[key][0]
    up = step_fn((gc.double() * (1 + delta)))[key][0]
    dn = step_fn((gc.double() * (1 - delta)))[key][0]
    return 2 * torch.maximum((up - w0).abs(), (dn - w0).abs())


def hyper(eng):
    """the scalars of the engine's update in the order of op_bounds.adam / op_bounds.sgd"""
    if eng.optimizer == 'sgd':
        return (eng.lr, eng.momentum, eng.weight_decay)
    return (eng.lr, eng.betas[0], eng.betas[1], eng.eps, eng.weight_decay)


def optimizer_reference(eng, before, step, blocks):
    """the float64 twin of one update from the snapshot `before` (P, G, M, V as fp32 tensors, on the device: evaluated there, see
    op_bounds.on_device) -> {'P' | 'M' | 'V': (want, bound)} with the composed bound of the module docstring; M only with momentum"""
    n = eng.nparam_padded
    g, dev = before['G'], before['G'].device
    real = real_mask(eng)
    assert bool((g.cpu()[~real] == 0).all())          # the norm over the flat buffer is the norm over the parameter tensors
    if eng.clip_grad is not None:
        gc = reference_gradient(g.cpu(), 1.0, eng.clip_grad).to(dev)
        delta = scale_delta(n, blocks)
    else:
        gc, delta = g, None
    if eng.optimizer == 'sgd':
        mom = before['M'] if eng.momentum else None
        fn = lambda g_: ob.sgd(before['P'], g_, mom, *hyper(eng), 1.0)
        names = {'P': 'p', 'M': 'mom'} if eng.momentum else {'P': 'p'}
    else:
        fn = lambda g_: ob.adam(before['P'], g_, before['M'], before['V'], *hyper(eng), step, 1.0)
        names = {'P': 'p', 'M': 'm', 'V': 'v'}
    with ob.on_device():
        want = fn(gc)
        out = {}
        for K, k in names.items():
            w, e = want[k]
            if delta is not None:
                e = e + sensitivity(fn, gc, delta, k)
            out[K] = (w, e)
    return out


def check_optimizer(name, eng, before, step, blocks):
    """P, M, V (and E) of `eng` after an update against the twin of the snapshot `before`; -> the worst err / bound"""
    want = optimizer_reference(eng, before, step, blocks)
    with ob.on_device():
        worst = ob.check_dict(name, {K: getattr(eng, K) for K in want}, want)
    if eng.optimizer == 'sgd' and not eng.momentum:
        assert same(eng.M, before['M'])               # no momentum buffer: the op carries NULL and M is never written
    if eng.optimizer == 'sgd':
        assert same(eng.V, before['V'])
    if eng.ema_decay is not None:
        w = eb.weight(eng.ema_decay, eng.ema_updates)
        assert eng._ema_w == w, (name, eng._ema_w, w)
        worst = max(worst, eb.check(name + ' E', eng.E.cpu(), before['E'].cpu(), eng.P.cpu(), w))
    return worst


def check_clip_state(name, eng, before, blocks):
    """norm within clip_cases' bound of the float64 norm of the snapshot's G; the coefficient torch's formula of the device's norm, bit
    for bit; the largest norm and the count of clipped steps carried on -> (norm, coef)"""
    ref = cc.ref_norm(before['G'].cpu())
    s, s0 = eng.clip_state[:4].cpu(), before['clip_state'][:4].cpu()
    norm, coef = float(s[0]), float(s[1])
    bound = cc.norm_bound(eng.nparam_padded, blocks, ref)
    print('%s: norm %.9g ref %.9g err %.3g bound %.3g coef %.6g' % (name, norm, ref, abs(norm - ref), bound, coef))
    assert math.isfinite(norm) and abs(norm - ref) <= bound, (name, norm, ref, bound)
    assert cc.f32_bits(coef) == cc.f32_bits(cc.host_coef(s[0].numpy(), eng.clip_grad)), (name, coef)
    assert float(s[2]) == max(float(s0[2]), norm) and float(s[3]) == float(s0[3]) + (1.0 if coef < 1.0 else 0.0), (name, s, s0)
    return norm, coef
