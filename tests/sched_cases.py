"""TRAIN --optimizer AdamW and --lr-schedule: the float64 twin of one decoupled-decay step with its error bound, torch's schedulers stepped
for comparison, and the engine-level reference of one optimizer step at a given rate.  Helpers only; tests/test_lr_schedule_cpu.py (host)
and tests/test_gpu_adamw.py, tests/test_gpu_sched_engine.py (device) run them.

The AdamW step (adam_kernel<true> of csrc/pool_head.hip, ifcbk_adamw_flat), in the notation of tests/op_bounds.py (u = 2^-24, gamma_n):

    host:  d = (float)(1.0 - (double)lr * (double)wd).  lr and wd are fp32, so their product is exact in double (48 bits); the
           subtraction rounds once in double and the conversion once to fp32.  The twin forms d by the same three operations, so d is
           an INPUT of the bound, bit for bit, not a term of it.
    pd = p * d             one fp32 product (a statement of its own in both the float4 body and the scalar tail, so never contracted
                           into what follows):  e_pd = u |p d|.
    gr = g * gs            one product, gamma_1; the twin takes op_bounds.adam with weight_decay = 0, whose gr = g * gs + 0 * p is charged
                           gamma_2 |g gs|: the same value, a bound one u looser and never tighter.
    m', v', denom, q       op_bounds.adam's terms, unchanged: they do not read p when weight_decay = 0.
    p' = pd - (lr / bc1) q op_bounds.adam's e_step, and its store: e_step + u (|p'| + e_step), evaluated from the EXACT pd.  The device
                           starts from its rounded pd instead: e_pd more in front of the store, which grows by u e_pd:
           e_p = e_pd (1 + u) + e_step + u (|p'| + e_step).
    weight_decay = 0: d = 1, pd = p exactly, e_pd = u |p| is kept (never tighter than op_bounds.adam, which the call then is).

With `exact=True` nothing is rounded to fp32 (d = 1 - lr wd in double): torch.optim.AdamW in float64, to double rounding.

Clipping and the weight average compose as in tests/option_matrix.py: clip_grad_norm_ of the float64 gradient rounded once, the slack
`sensitivity(..., scale_delta(n))`; ema_bounds from the P the device wrote."""
import torch

import clip_cases as cc
import ema_bounds as eb
import op_bounds as ob
import option_matrix as om

U = ob.U


def decay_factor(lr, wd, exact=False):
    """the factor p is scaled by: in double, or as ifcbk_adamw_flat forms it from the fp32 scalars"""
    if exact:
        return 1.0 - lr * wd
    return ob.f32(1.0 - ob.f32(lr) * ob.f32(wd))


def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, gs, exact=False):
    """one AdamW step from the fp32 state: {'p' | 'm' | 'v': (want, e)}.  exact: scalars as given, in double, the bound is not meant"""
    p64 = ob.f64(p)
    d = decay_factor(lr, wd, exact)
    pd = p64 * d
    if exact:
        g, m, v = ob.f64(g), ob.f64(m), ob.f64(v)
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        gr = g * gs
        m2 = b1 * m + (1 - b1) * gr
        v2 = b2 * v + (1 - b2) * gr * gr
        den = torch.sqrt(v2) / (bc2 ** 0.5) + eps
        z = torch.zeros_like(pd)
        return {'p': (pd - (lr / bc1) * (m2 / den), z), 'm': (m2, z), 'v': (v2, z)}
    out = ob.adam(pd, g, m, v, lr, b1, b2, eps, 0.0, step, gs)
    p2, e_p = out['p']
    out['p'] = (p2, e_p + U * pd.abs() * (1 + U))
    return out


# ------------------------------------------------------------------------------------------------------ torch's schedulers, stepped
def torch_rates(kind, base, T, W, lr_min):
    """the rate of each of T optimizer steps under torch.optim.lr_scheduler on a dummy CPU parameter: LinearLR(1/W .. 1 over W - 1 steps)
    for the warm-up, then CosineAnnealingLR(T - W, eta_min) / LinearLR(1 .. lr_min / base over T - W steps) / nothing, under SequentialLR"""
    from torch.optim import lr_scheduler as ls
    w = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.SGD([w], lr=base)
    parts, miles = [], []
    if W >= 2:
        parts.append(ls.LinearLR(opt, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1))
        miles.append(W)
    elif W == 1:
        parts.append(ls.ConstantLR(opt, factor=1.0, total_iters=1))
        miles.append(W)
    if kind == 'cosine':
        parts.append(ls.CosineAnnealingLR(opt, T_max=T - W, eta_min=lr_min))
    elif kind == 'linear':
        parts.append(ls.LinearLR(opt, start_factor=1.0, end_factor=lr_min / base, total_iters=T - W))
    else:
        parts.append(ls.ConstantLR(opt, factor=1.0, total_iters=1))
    sched = parts[0] if len(parts) == 1 else ls.SequentialLR(opt, parts, milestones=miles)
    rates = []
    for _ in range(T):
        rates.append(opt.param_groups[0]['lr'])
        opt.step()
        sched.step()
    return rates


# ------------------------------------------------------------------------------------------------------ one engine step
def snapshot(eng):
    """P, G, M, V (and E, the clip state) in front of an update, on the device"""
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in ('P', 'G', 'M', 'V')}
    if eng.ema_decay is not None:
        before['E'] = eng.E.clone()
    if eng.clip_state is not None:
        before['clip_state'] = eng.clip_state.clone()
    return before


def optimizer_reference(eng, before, step, lr, blocks=None):
    """option_matrix.optimizer_reference for an 'adam' / 'adamw' engine at the rate `lr` of this step -> {'P' | 'M' | 'V': (want, bound)}"""
    assert eng.optimizer in ('adam', 'adamw')
    g = before['G']
    real = om.real_mask(eng)
    assert bool((g.cpu()[~real] == 0).all())
    if eng.clip_grad is not None:
        gc = om.reference_gradient(g.cpu(), 1.0, eng.clip_grad).to(g.device)
        delta = om.scale_delta(eng.nparam_padded, blocks)
    else:
        gc, delta = g, None
    twin = adamw if eng.optimizer == 'adamw' else ob.adam
    fn = lambda g_: twin(before['P'], g_, before['M'], before['V'], lr, eng.betas[0], eng.betas[1], eng.eps, eng.weight_decay, step, 1.0)
    with ob.on_device():
        want = fn(gc)
        out = {}
        for K, k in (('P', 'p'), ('M', 'm'), ('V', 'v')):
            w, e = want[k]
            if delta is not None:
                e = e + om.sensitivity(fn, gc, delta, k)
            out[K] = (w, e)
    return out


def check_optimizer(name, eng, before, step, lr):
    """P, M, V (and E) of `eng` after the update against the twin at rate `lr`; the padding of the flat buffers stays exactly zero -> the
    worst err / bound"""
    blocks = cc.geometry(eng.ctx.lib)[0] if eng.clip_grad is not None else None
    want = optimizer_reference(eng, before, step, lr, blocks)
    with ob.on_device():
        worst = ob.check_dict(name, {K: getattr(eng, K) for K in want}, want)
    pad = ~om.real_mask(eng)
    for K in ('P', 'M', 'V'):
        assert bool((getattr(eng, K).cpu()[pad] == 0).all()), '%s: padding of %s is not zero' % (name, K)
    if eng.ema_decay is not None:
        w = eb.weight(eng.ema_decay, eng.ema_updates)
        assert eng._ema_w == w, (name, eng._ema_w, w)
        worst = max(worst, eb.check(name + ' E', eng.E.cpu(), before['E'].cpu(), eng.P.cpu(), w))
    return worst


def opt_ops(eng, prog):
    """the optimizer ops of a Program, in order"""
    from ifcb_classifier_amd import _lib
    return [prog.arr[j] for j in prog.find(_lib.OP_ADAM)]
