"""Float64 oracle and per-element bound of the weight average (TRAIN --ema): the update inside adam_kernel / sgd_kernel
(csrc/pool_head.hip), the plain ifcbk_ema_flat (csrc/ema.hip), and the decay schedule of the engine.

A plain helper module in the manner of op_bounds.py.  Nothing here is measured: everything runs on the CPU in float64, from the fp32
values the kernel read and was given.

The update.  With e the fp32 average the kernel read, p the fp32 parameter it had just written (for ifcbk_ema_flat: the x it read) and
w the fp32 weight it was given, the kernel computes, in fp32,

    t  = fl(p - e)
    e' = fl(e + w t)                  one rounding when the compiler contracts a * b + c into an fma (the library is built with
                                      -ffp-contract=on), else s = fl(w t), e' = fl(e + s): two

and the exact value is X = e + w (p - e).  With u = 2^-24 and |d1|, |d2|, |d3| <= u:

    uncontracted   e' = (e + w (p - e) (1 + d1) (1 + d2)) (1 + d3)
                   e' - X = X d3 + w (p - e) (d1 + d2 + d1 d2) (1 + d3)
                   |e' - X| <= u |X| + (2u + u^2) (1 + u) |w| |p - e|
    contracted     e' = (e + w (p - e) (1 + d1)) (1 + d3): the same with d2 = 0, so within the same bound.

Hence  |e' - X| <= u |X| + 2u |w| |p - e|  plus second-order terms, which `bound` keeps: (2u + u^2)(1 + u) in the place of 2u.  Where a
result is subnormal a rounding errs by at most 2^-150 absolutely in the place of u relatively: three roundings, 3 * 2^-150 on top.  The
float64 evaluation of X itself (a subtraction, a product, a sum of fp32 values, 2^-53 each) is charged as 3 * 2^-53 (|e| + |w| |p - e|).

Consequences the tests use: w = 0 gives e' = e (the entry points do not even launch the update then, so a -0 keeps its sign);
w = 1 gives X = p and e' within u |p| + 2u |p - e| of it; p = e is a fixed point, exactly: t = 0, e' = e.  The form
d e + (1 - d) p with two separately rounded scalars has no such fixed point (its fixed point is p (1 - d) / (1 - fl(d))).

The schedule.  d_t = min(DECAY, (1 + t) / (10 + t)) for the t-th update since the average was initialised, t = 1, 2, ... (TensorFlow's
ExponentialMovingAverage(num_updates)); without warm-up d_t = DECAY.  The kernel's w is 1 - d_t evaluated in double and rounded once
to fp32.
"""
import struct

import torch

U = 2.0 ** -24
D = 2.0 ** -53
SUB = 2.0 ** -150


def decay_at(decay, t, warmup=True):
    """d_t, in double"""
    if not warmup:
        return float(decay)
    return min(float(decay), (1.0 + t) / (10.0 + t))


def f32(v):
    """a python float rounded once to fp32 (as the C ABI passes a float argument)"""
    return struct.unpack('f', struct.pack('f', float(v)))[0]


def weight(decay, t, warmup=True):
    """the fp32 weight of the t-th update: fl32(1 - d_t)"""
    return f32(1.0 - decay_at(decay, t, warmup))


def update(e, p, w):
    """X = e + w (p - e) in float64 from fp32 tensors e, p and the fp32 scalar w"""
    e, p = e.detach().double().cpu(), p.detach().double().cpu()
    return e + float(w) * (p - e)


def bound(e, p, w):
    """the per-element bound of the docstring on |e' - X|"""
    e, p = e.detach().double().cpu(), p.detach().double().cpu()
    w = abs(float(w))
    x = e + w * (p - e) if w else e
    step = w * (p - e).abs()
    return U * x.abs() + (2 * U + U * U) * (1 + U) * step + 3 * SUB + 3 * D * (e.abs() + step)


def check(name, got, e, p, w):
    """assert the bound for every element; returns the worst err / bound (for a log line)"""
    assert got.dtype == torch.float32 and e.dtype == torch.float32 and p.dtype == torch.float32, name
    err = (got.detach().double().cpu() - update(e, p, w)).abs()
    b = bound(e, p, w)
    worst = float((err / b).max()) if err.numel() else 0.0
    assert bool((err <= b).all()), '%s: worst err / bound %.3g at element %d' % (name, worst, int((err / b).argmax()))
    return worst
