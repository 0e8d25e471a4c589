"""Per-element error bound of the label-smoothed cross-entropy (csrc/loss.hip, softmax_xent_ls_kernel) against a float64 reference.

A plain helper module beside loss_bounds.py and op_bounds.py, whose softmax(), gamma, U, E_LIBM and check_dict it reuses; op_bounds'
docstring has the notation (u = 2^-24, gamma_n, E) and the count of the unsmoothed loss, loss_bounds' the weighted one, which this
one extends term by term.  No tolerance is chosen anywhere: every term below is one operation of the kernel.

Reference, in float64 from the fp32 values the kernel reads (a = the scalar `weight` and eps = `label_smoothing` as the C ABI rounds
them to float, w = class_weight or all ones, C = NC, p = softmax(l)):
    W = sum_n w[t_n],  SW = sum_k w[k],  c1 = 1 - eps,  eC = eps / C,  A_n = c1 w[t_n] + eC SW
    l_n = max + log s - l[t_n]  (= -log p[n][t_n]),       q_n = sum_j w[j] ((max - l[n][j]) + log s)  (= sum_j w[j] (-log p[n][j]))
    loss = a / W sum_n (c1 w[t_n] l_n + eC q_n),          dlogits[n][j] = a / W (A_n p[n][j] - c1 w[t_n] [j = t_n] - eC w[j])
which is torch's F.cross_entropy(weight=, label_smoothing=) with mean reduction (test_label_smoothing_cpu.py holds the two together
in float64).

What the kernel does, counted:
    W^, SW^: fp32 sums of N / C non-negative terms in a fixed order (empty slots add exact zeros): relative gamma_N / gamma_C;
        1 / W^ and a / W^ carry r_W = gamma_N / (1 - gamma_N).  Without class weights the terms are ones and both sums are exact;
        the bound does not use that.
    c1^ = fl(1 - eps), eC^ = fl(eps / C): u each.
    A^ = fl(c1^ w_t + eC^ SW^): both terms non-negative, so the relative error is at most the larger of gamma_3 (c1, product, add) and
        gamma_C + 3u (eC, SW, product, add):  r_A = gamma_(C + 3).
    dlogits = g^ * (A^ p^ - T2 - T3),  g^ = fl(a / W^): r_g = r_W + u (1 + r_W)
        A^ p^: r_T = r_A + u + r_A u for the factor and the product, on A (p + e_p)        (e_p: op_bounds.softmax, the stored p's error)
        T2 = fl(c1^ w_t) on the target, T3 = fl(eC^ w_j): gamma_2 each
        two subtractions (a fused multiply-subtract rounds once less, never more): 2u of M = A p + c1 w_t [j = t] + eC w_j plus the
        errors so far -- relative to M, never to the difference, which cancels (NC = 1: the difference is 0)
        e_in = e_T1 + e_T2 + e_T3 + 2u (M + e_T1 + e_T2 + e_T3);   e = |g| e_in (1 + r_c) + r_c |dlogits|,  r_c = r_g + u + r_g u
    loss:
        l_n^: e_n as in op_bounds.xent.
        log s^: e_ls = e_s / s (1 + 2^-10) + E u |log s|      (the two terms of e_n that belong to log s)
        piece_j = w_j * fl(fl(max - l_j) + log s^): d_j = max - l_j >= 0 and log s >= 0 (s >= 1: the maximum contributes exp(0) = 1)
            e_b = u d_j + e_ls + u (d_j + log s + u d_j + e_ls),   e_piece = w_j e_b (1 + u) + u w_j (d_j + log s)
        q_n^: C non-negative pieces, a lane's chain and two butterfly adds, at most gamma_C:  e_q = gamma_C (q_n + sum e_piece) + sum e_piece
        term_n = fl(c1^ * fl(w_t l_n^) + eC^ * q_n^):  h1 = c1 w_t l_n: gamma_3 |h1| + c1 w_t e_n (1 + gamma_3);  h2 = eC q_n:
            gamma_2 h2 + eC e_q (1 + gamma_2);  the add: u (|h1| + h2 + e_h1 + e_h2)
        the N terms and the slot partials are summed in fp32, gamma_(N + 1) as in op_bounds.xent, on sum (|h1| + h2 + e_term);
        then fl(1 / W^) and the two products, 3u, and r_W, relative to |loss| + e; one add when accumulating -- as loss_bounds.xent_w.
"""
import torch

import op_bounds as ob
from op_bounds import E_LIBM, U, f32, f64, gamma


# the shapes both test files run: the 256-slot loop's first wrap (255, 256, 257, 600), every NC mod 4, lanes with no class at all (NC < 4)
NS = (1, 3, 255, 256, 257, 600)
NCS = (1, 2, 3, 5, 100, 101)
SHAPES = [(N, NC) for N in NS for NC in NCS]
WEIGHTS = ('none', 'random', 'zero')


def inputs(N, NC, weights='random', scale=4.0, offset_row=False):
    """(logits, target, class_weight or None): logits randn * scale (offset_row: + 80 on one row), weights 'none', 'random' in [0.1, 1.1],
    or 'zero': the same with the weight of one class set to 0 -- the class fewest targets name, so that W > 0 whenever NC > 1"""
    gen = torch.Generator().manual_seed(1000 * N + NC)
    l = torch.randn(N, NC, generator=gen) * scale
    t = torch.randint(0, NC, (N,), generator=gen)
    cw = torch.rand(NC, generator=gen) + 0.1
    if offset_row:
        l[N // 2] += 80.0
    if weights == 'none':
        return l, t, None
    if weights == 'zero':
        cw[int(torch.bincount(t, minlength=NC).argmin())] = 0.0
    return l, t, cw


def reference(logits, target, class_weight, weight, eps):
    """(loss, dlogits) in float64, from the definition alone"""
    l = f64(logits)
    N, NC = l.shape
    a, eps = f32(weight), f32(eps)
    t = target.cpu().long()
    w = torch.ones(NC, dtype=torch.float64) if class_weight is None else f64(class_weight)
    wt = w[t][:, None]
    W, SW = wt.sum(), w.sum()
    c1, eC = 1.0 - eps, eps / NC
    logp = torch.log_softmax(l, 1)
    p = logp.exp()
    oh = torch.zeros_like(p)
    oh[torch.arange(N), t] = 1.0
    loss = a / W * (c1 * wt[:, 0] * -logp[torch.arange(N), t] + eC * (w[None] * -logp).sum(1)).sum()
    dl = a / W * ((c1 * wt + eC * SW) * p - c1 * wt * oh - eC * w[None])
    return loss, dl


def xent_ls(logits, target, class_weight, weight, eps, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of weight * CrossEntropyLoss(weight=class_weight, label_smoothing=eps)(logits, target),
    mean reduction; class_weight None = all ones"""
    l = f64(logits)
    N, NC = l.shape
    a, eps = f32(weight), f32(eps)
    t = target.cpu().long()
    w = (torch.ones(NC, dtype=torch.float64) if class_weight is None else f64(class_weight))[None]
    wt = w[0][t][:, None]
    W, SW = wt.sum(), w.sum()
    c1, eC = 1.0 - eps, eps / NC
    r_W = gamma(N) / (1 - gamma(N))
    r_A = gamma(NC + 3)
    r_T = r_A + U + r_A * U
    r_g = r_W + U * (1 + r_W)
    r_c = r_g + U + r_g * U
    p, e_p, (mx, s, e_s) = ob.softmax(l)
    oh = torch.zeros_like(p)
    oh[torch.arange(N), t] = 1.0
    # ---- dlogits
    A = c1 * wt + eC * SW
    T1, T2, T3 = A * p, c1 * wt * oh, eC * w.expand_as(p)
    e_T = A * e_p * (1 + r_T) + r_T * T1 + gamma(2) * (T2 + T3)
    M = T1 + T2 + T3
    e_in = e_T + 2 * U * (M + e_T)
    g = a / W
    dl = g * (T1 - T2 - T3)
    e_dl = abs(g) * e_in * (1 + r_c) + r_c * dl.abs()
    # ---- loss
    ls = torch.log(s)
    lt = l[torch.arange(N), t][:, None]
    li = mx + ls - lt
    e_ls = e_s / s * (1 + 2.0 ** -10) + E_LIBM * U * ls.abs()
    e_i = e_ls + 2 * U * (mx.abs() + ls.abs() + lt.abs())
    d = mx - l
    b = d + ls
    e_b = U * d + e_ls + U * (d + ls + U * d + e_ls)
    e_piece = w * e_b * (1 + U) + U * w * b
    q = (w * b).sum(1, keepdim=True)
    e_q = gamma(NC) * (q + e_piece.sum(1, keepdim=True)) + e_piece.sum(1, keepdim=True)
    h1, h2 = c1 * wt * li, eC * q
    e_h1 = gamma(3) * h1.abs() + c1 * wt * e_i * (1 + gamma(3))
    e_h2 = gamma(2) * h2 + eC * e_q * (1 + gamma(2))
    e_term = e_h1 + e_h2 + U * (h1.abs() + h2 + e_h1 + e_h2)
    loss = a / W * (h1 + h2).sum()
    e = abs(a) / W * (gamma(N + 1) * (h1.abs() + h2 + e_term).sum() + e_term.sum())
    e = e + (3 * U + r_W) * (loss.abs() + e)
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


def check(name, got, want, family=None, raise_=True):
    """op_bounds.check_dict: |got - want| <= 1/2 ulp(|want| + e) + e per element; returns the worst err / bound"""
    return ob.check_dict(name, got, want, family=family, raise_=raise_)
