"""Per-element error bound of the class-weighted cross-entropy (csrc/loss.hip, softmax_xent_w_kernel) against a float64 reference.

A plain helper module beside op_bounds.py, whose softmax(), gamma, U, E_LIBM, elem and check_dict it reuses; op_bounds' docstring has
the notation (u = 2^-24, gamma_n, E) and the derivation of the unweighted loss, which this one extends term by term.

Reference, in float64 from the fp32 values the kernel reads (a = the scalar `weight` as the C ABI rounds it, w = class_weight):
    W = sum_n w[t_n],   dlogits[n][j] = a w[t_n] / W (p[n][j] - onehot),   loss = a / W sum_n w[t_n] l_n,   l_n = max + log s - l[t_n]

What the kernel adds to op_bounds.xent's count:
    W is a fp32 sum of N non-negative terms in a fixed order: |W^ - W| <= gamma_N W, so 1 / W^ carries r_W = gamma_N / (1 - gamma_N).
    coefficient c_n = a * (w_t / W^): one division and one product, and d = c_n * (p - onehot) one more product: with r_W,
        r_c = r_W + gamma_3.
        dlogits:  a w_t / W (e_p + u (p + onehot)) (1 + r_c) + r_c |dlogits|        (e_p, u (p + onehot): as in op_bounds.xent)
    loss: the term w_t * l_n is rounded (u |w_t l_n|; a fused multiply-add rounds once less, never more), the N terms and the slot
        partials are summed in fp32 (gamma_(N + 1), as in op_bounds.xent), each l_n carries its e_n:
        e = a / W ((gamma_(N + 1) + u) sum w_t |l_n| + (1 + gamma_(N + 1) + u) sum w_t e_n)
        then fl(1 / W^) and the two products, 3u, and r_W, all relative to |loss| + e; one add when accumulating.
With all-ones weights this is op_bounds.xent's bound plus the r_W and u terms (the kernel is then bit-equal to the unweighted one,
which the GPU test checks separately).
"""
import torch

import op_bounds as ob
from op_bounds import E_LIBM, U, f32, f64, gamma


def xent_w(logits, target, class_weight, weight, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of weight * CrossEntropyLoss(weight=class_weight)(logits, target), mean reduction"""
    l = f64(logits)
    N, NC = l.shape
    a = f32(weight)
    t = target.cpu().long()
    wt = f64(class_weight)[t][:, None]
    W = wt.sum()
    r_W = gamma(N) / (1 - gamma(N))
    r_c = r_W + gamma(3)
    p, e_p, (mx, s, e_s) = ob.softmax(l)
    oh = torch.zeros_like(p)
    oh[torch.arange(N), t] = 1.0
    k = abs(a) * wt / W
    dl = a * wt / W * (p - oh)
    e_dl = k * (e_p + U * (p + oh)) * (1 + r_c) + r_c * dl.abs()
    lt = l[torch.arange(N), t][:, None]
    li = mx + torch.log(s) - lt
    e_i = e_s / s * (1 + 2.0 ** -10) + E_LIBM * U * torch.log(s).abs() + 2 * U * (mx.abs() + torch.log(s).abs() + lt.abs())
    loss = a / W * (wt * li).sum()
    e = abs(a) / W * ((gamma(N + 1) + U) * (wt * li.abs()).sum() + (wt * e_i).sum() * (1 + gamma(N + 1) + U))
    e = e + (3 * U + r_W) * (loss.abs() + e)
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


def check(name, got, want, family=None, raise_=True):
    """op_bounds.check_dict: |got - want| <= 1/2 ulp(|want| + e) + e per element; returns the worst err / bound"""
    return ob.check_dict(name, got, want, family=family, raise_=raise_)


def head_sum(main, aux):
    """loss of a network with an auxiliary head, main + aux: `aux` is xent_w(..., old_loss=float(main['loss'][0])) -- the aux op adds its
    term onto the value the main op stored, so the stored value's own error (e_main and the rounding of its store) passes through
    the add unchanged"""
    (lm, em), (la, ea) = main['loss'], aux['loss']
    return {'loss': (la, ea + (em + U * (lm.abs() + em)) * (1 + U))}
