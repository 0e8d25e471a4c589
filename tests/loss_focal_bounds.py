"""Per-element error bound of the focal loss (csrc/loss.hip, softmax_xent_focal_kernel) against a float64 reference.

A plain helper module beside loss_bounds.py and loss_smooth_bounds.py, whose shapes, weights and inputs it takes over, and op_bounds.py,
whose softmax(), gamma, U, E_LIBM and check_dict it reuses; op_bounds' docstring has the notation (u = 2^-24 -- written U below, since u
is focal loss's 1 - p_t here --, gamma_n, E).  No tolerance is chosen anywhere: every term below is one operation of the kernel.  The
focusing exponent is written g (`gamma` is op_bounds' gamma_n).

Reference, in float64 from the fp32 values the kernel reads (a = the scalar `weight` and g = `gamma` as the C ABI rounds them to float,
w = class_weight or all ones, p = softmax(l), t = target):
    W = sum_n w[t_n],   so_n = sum_{j != t} exp(l_j - max),   s_n = sum_j exp(l_j - max),   u_n = so_n / s_n  (= 1 - p_t, without its cancellation)
    L_n = -log p_t:  -log1p(-u_n) where u_n < 1/2, max + log s - l_t elsewhere (the first form keeps L ~ u when float64's s rounds to 1)
    loss = a / W sum_n w[t_n] u_n^g L_n
    dlogits[n][j] = a / W w[t_n] v[n][j] B_n,   v = p[n][j] off the target, -u_n on it,   B_n = u_n^g + g p_t Q_n,   Q_n = u_n^(g-1) L_n  (0 at u_n = 0)
torch has no multi-class focal loss: test_focal_cpu.py holds dlogits against float64 autograd of the loss, and g = 0 against
F.cross_entropy(weight=w).

What the kernel does, counted:
    W^: a fp32 sum of N non-negative terms in a fixed order: 1 / W^ and w_t / W^ carry r_W = gamma_N / (1 - gamma_N)  (as loss_bounds).
    s^: op_bounds.softmax's e_s.  so^: the same chain with the target's term replaced by 0:
        e_so = sum_{j != t} exp(.) (U |l_j - max| + E U) + gamma_NC so + NC TINY       (TINY = 2^-126: an expf result that underflows)
    u^ = fl(so^ / s^):  e_u = (e_so + u e_s) / (s - e_s), then the division: U (u + e_u) + TINY.  u^ lies in [u_lo, u_hi] = [max(u - e_u, 0),
        min(u + e_u, 1)]  (so^ <= s^ term by term, rounding is monotone: u^ <= 1).
    L^ = fl(fl(max + logf(s^)) - l_t):  e_L = e_s / s (1 + 2^-10) + E U |log s| + 2U (|max| + |log s| + |l_t|), op_bounds.xent's e_i;
        L^ >= 0 (s^ >= 1), so L^ lies in [max(L - e_L, 0), L + e_L].
    pw^ = expf(fl(g * logf(u^))) for u^ > 0, else 0 (g > 0) or 1 (g = 0).  The exponent's error is g |log u^| ((E + 1) U): logf and the
        product; through exp that is a relative error, with the conditioning g |log u^| the issue names; expf adds E U:
        r_pw = g lam (E + 1) U (1 + 2^-10) + E U,   lam = max |log x| over x in [max(u_lo, 2^-149), u_hi]  (2^-149: the least positive u^)
        (1 + 2^-10 covers the second-order terms while g lam (E + 1) U + 2 E U <= 2^-10: asserted).  x^g is monotone in x:
        pw^ in [u_lo^g (1 - r_pw) - TINY, u_hi^g (1 + r_pw) + TINY]  (TINY: underflow of the result).
    loss: term_n = fl(w_t * fl(pw^ * L^)): the product of the two intervals, gamma_2 for the two roundings (a fused multiply-add into the
        running sum rounds once less, never more).  The N terms and the slot partials are summed in fp32, gamma_(N + 1) as in op_bounds.xent;
        then fl(1 / W^) and the two products, 3U, and r_W, relative to |loss| + e; one add when accumulating -- as loss_bounds.xent_w.
    dlogits:
        p_t^ = fl(expf(l_t - max) * fl(1 / s^)): op_bounds.softmax's e_p at the target.
        Q^ = fl(pw^ * fl(L^ / u^)), 0 when u^ = 0.
            u_hi < 2^-25: then u^ < 2^-25 < 1/2, so the target holds the row's maximum, its term is expf(0) = 1, everything else adds up to
                less than 2^-24 and every add onto 1 rounds back to 1: s^ = 1, logf(1) = 0 (an E-ulp error of 0 is 0), L^ = max - l_t = 0
                exactly.  Q^ = 0 and e_Q = Q, the whole term.  (This is why L^ / u^ cannot overflow.)
            else u_lo > 0 (asserted) and pw^ / u^ lies between the least and the largest of x^(g-1) (1 -+ r_pw) -+ TINY / u_lo at the two
                ends, x^(g-1) being monotone either way; times the interval of L^, gamma_2 for the division and the product.
        T2^ = fl(fl(g * p_t^) * Q^): the product of the intervals of p_t^ and Q^ times g, gamma_2.
        B^ = fl(pw^ + T2^): e_B = e_pw + e_T2 + U (B + e_pw + e_T2); both terms are non-negative, nothing cancels.
        c^ = fl(fl(a * fl(w_t / W^)) * B^) and the product with v: four roundings and r_W: r_c = (1 + r_W) (1 + gamma_4) - 1.
        v^: e_p off the target (op_bounds.softmax), e_u on it (the kernel stores -u^ there, not p_t^ - 1).
        e = |a| w_t / W ((B + e_B) (|v| + e_v) - B |v|) (1 + r_c) + r_c |dlogits| + TINY.
Where the bound is loose: for u below about 1e-4, L^ carries the absolute error of s^ (about NC U), which L^ / u^ turns into a large
relative error of Q; the bound states it (e_L / u_lo), and dlogits there is of the order u^(g + 1).
"""
import math

import torch

import loss_smooth_bounds as sb
import op_bounds as ob
from loss_smooth_bounds import NCS, NS, SHAPES, WEIGHTS      # noqa: F401  (the shapes and weights both focal test files run)
from op_bounds import E_LIBM, TINY, U, f32, f64, gamma

GAMMAS = (0.5, 1.0, 2.0, 5.0)
MODES = (None, 'row80', 'row120', 'peak120', 'low80')


def inputs(N, NC, weights='random', scale=4.0, mode=None):
    """loss_smooth_bounds.inputs, and on row N // 2:  'row80' / 'row120': the whole row 80 / 120 higher;  'peak120': the target's logit 120
    above the rest of its row (every other exponential is 0 in fp32: u == 0 exactly);  'low80': the target's logit 80 below the rest of its
    row (u -> 1)"""
    assert mode in MODES
    l, t, cw = sb.inputs(N, NC, weights, scale, offset_row=(mode == 'row80'))
    r = N // 2
    if mode == 'row120':
        l[r] += 120.0
    elif mode == 'peak120':
        l[r, t[r]] = l[r].max() + 120.0
    elif mode == 'low80':
        l[r, t[r]] = l[r].min() - 80.0
    return l, t, cw


def parts(l, t):
    """float64 pieces of a row, differentiable: (p, onehot, u, p_t, L)"""
    N, NC = l.shape
    ar = torch.arange(N)
    mx = l.max(1, keepdim=True).values
    ex = torch.exp(l - mx)
    oh = torch.zeros(N, NC, dtype=l.dtype)
    oh[ar, t] = 1.0
    s = ex.sum(1, keepdim=True)
    so = (ex * (1.0 - oh)).sum(1, keepdim=True)
    u = so / s
    p = ex / s
    L = torch.where(u < 0.5, -torch.log1p(-u.clamp(max=0.5)), mx + torch.log(s) - l[ar, t][:, None])
    return p, oh, u, p[ar, t][:, None], L


def loss64(l, t, w, a, g):
    """the definition's loss from float64 logits l (autograd may run through it)"""
    _, _, u, _, L = parts(l, t)
    wt = w[t][:, None]
    return a / wt.sum() * (wt * u ** g * L).sum()


def _scalars(logits, target, class_weight, weight, g):
    l = f64(logits)
    t = target.cpu().long()
    w = torch.ones(l.shape[1], dtype=torch.float64) if class_weight is None else f64(class_weight)
    return l, t, w, f32(weight), f32(g)


def reference(logits, target, class_weight, weight, g):
    """(loss, dlogits) in float64, from the definition alone"""
    l, t, w, a, g = _scalars(logits, target, class_weight, weight, g)
    p, oh, u, pt, L = parts(l, t)
    wt = w[t][:, None]
    W = wt.sum()
    pos = u > 0
    Q = torch.where(pos, u.clamp_min(1e-300) ** (g - 1.0) * L, torch.zeros_like(u))
    B = u ** g + g * pt * Q
    v = torch.where(oh > 0, -u, p)
    return a / W * (wt * u ** g * L).sum(), a / W * wt * v * B


def xent_focal(logits, target, class_weight, weight, g, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of weight * focal loss (exponent g, alpha = class_weight or ones, normaliser W)"""
    l, t, w, a, g = _scalars(logits, target, class_weight, weight, g)
    N, NC = l.shape
    ar = torch.arange(N)
    wt = w[t][:, None]
    W = wt.sum()
    r_W = gamma(N) / (1 - gamma(N))
    p, e_p, (mx, s, e_s) = ob.softmax(l)
    _, oh, u, pt, L = parts(l, t)
    d = l - mx
    ex = torch.exp(d)
    # ---- u
    so = (ex * (1 - oh)).sum(1, keepdim=True)
    e_so = (ex * (1 - oh) * (U * d.abs() + E_LIBM * U)).sum(1, keepdim=True) + gamma(NC) * so + NC * TINY
    e_u = (e_so + u * e_s) / (s - e_s)
    e_u = e_u + U * (u + e_u) + TINY
    u_lo, u_hi = (u - e_u).clamp_min(0), (u + e_u).clamp_max(1)
    # ---- L
    ls = torch.log(s)
    lt = l[ar, t][:, None]
    e_L = e_s / s * (1 + 2.0 ** -10) + E_LIBM * U * ls.abs() + 2 * U * (mx.abs() + ls.abs() + lt.abs())
    L_lo, L_hi = (L - e_L).clamp_min(0), L + e_L
    # ---- pw = u^g
    lam = torch.maximum(torch.log(u_hi).abs(), torch.log(u_lo.clamp_min(2.0 ** -149)).abs())
    cond = g * lam * (E_LIBM + 1) * U
    assert float(cond.max()) + 2 * E_LIBM * U <= 2.0 ** -10, 'gamma too large for the first-order count of the power'
    r_pw = cond * (1 + 2.0 ** -10) + E_LIBM * U
    pw = u ** g                                                         # (0 ** 0 = 1: the kernel's value at u = 0, g = 0)
    pw_lo, pw_hi = (u_lo ** g * (1 - r_pw) - TINY).clamp_min(0), u_hi ** g * (1 + r_pw) + TINY
    e_pw = torch.maximum(pw_hi - pw, pw - pw_lo)
    # ---- loss
    PL = pw * L
    e_PL = torch.maximum(pw_hi * L_hi - PL, PL - pw_lo * L_lo)
    term = wt * PL
    e_term = wt * (e_PL + gamma(2) * (PL + e_PL))
    loss = a / W * term.sum()
    e = abs(a) / W * (gamma(N + 1) * (term + e_term).sum() + e_term.sum())
    e = e + (3 * U + r_W) * (loss.abs() + e)
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    # ---- dlogits
    pos = u > 0
    Q = torch.where(pos, u.clamp_min(1e-300) ** (g - 1.0) * L, torch.zeros_like(u))
    small = u_hi < 2.0 ** -25
    assert bool((small | (u_lo > 0)).all())
    ul = torch.where(small, torch.ones_like(u), u_lo)                   # (placeholders in the rows the other case takes)
    uh = torch.where(small, torch.ones_like(u), u_hi)
    ends = torch.stack([ul ** (g - 1.0), uh ** (g - 1.0)])
    rho_hi = ends.max(0).values * (1 + r_pw) + TINY / ul
    rho_lo = (ends.min(0).values * (1 - r_pw) - TINY / ul).clamp_min(0)
    Qc_hi, Qc_lo = rho_hi * L_hi * (1 + gamma(2)) + TINY, (rho_lo * L_lo * (1 - gamma(2)) - TINY).clamp_min(0)
    e_Q = torch.where(small, Q, torch.maximum(Qc_hi - Q, Q - Qc_lo))
    Q_lo, Q_hi = (Q - e_Q).clamp_min(0), Q + e_Q
    e_pt = e_p[ar, t][:, None]
    T2 = g * pt * Q
    T2_hi = g * (pt + e_pt) * Q_hi * (1 + gamma(2)) + TINY
    T2_lo = (g * (pt - e_pt).clamp_min(0) * Q_lo * (1 - gamma(2)) - TINY).clamp_min(0)
    e_T2 = torch.maximum(T2_hi - T2, T2 - T2_lo)
    B = pw + T2
    e_B = e_pw + e_T2 + U * (B + e_pw + e_T2)
    r_c = (1 + r_W) * (1 + gamma(4)) - 1
    v = torch.where(oh > 0, -u, p)
    e_v = torch.where(oh > 0, e_u.expand_as(p), e_p)
    k = abs(a) * wt / W
    dl = a * wt / W * v * B
    e_dl = k * ((B + e_B) * (v.abs() + e_v) - B * v.abs()) * (1 + r_c) + r_c * dl.abs() + TINY
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


def check(name, got, want, family=None, raise_=True):
    """op_bounds.check_dict: |got - want| <= 1/2 ulp(|want| + e) + e per element; returns the worst err / bound"""
    return ob.check_dict(name, got, want, family=family, raise_=raise_)


def emulate(logits, target, class_weight, weight, g, old_loss=None):
    """the kernel's operations in float32 torch, in its order (four lanes per row, the two butterflies, slot partials summed in slot
    order): what a correct fp32 implementation gives, for the check that the reference sits inside the bound"""
    l = logits.float()
    N, NC = l.shape
    t = target.long()
    ar = torch.arange(N)
    f = torch.float32
    one = torch.ones((), dtype=f)
    w = torch.ones(NC, dtype=f) if class_weight is None else class_weight.float()
    a, g = torch.tensor(weight, dtype=f), torch.tensor(g, dtype=f)

    def slots(x):                                                       # per-slot chains, then the 256 partials in slot order
        part = torch.zeros(256, dtype=f)
        for n0 in range(0, N, 256):
            c = x[n0:n0 + 256]
            part[:len(c)] = part[:len(c)] + c
        tot = torch.zeros((), dtype=f)
        for i in range(256):
            tot = tot + part[i]
        return tot
    wt = w[t]
    W = slots(wt)
    mx = l.max(1).values
    ex = torch.exp(l - mx[:, None])
    oh = torch.zeros(N, NC, dtype=torch.bool)
    oh[ar, t] = True
    exo = torch.where(oh, torch.zeros((), dtype=f), ex)

    def lanes(x):                                                       # lane sub sums j = sub, sub + 4, ...; then xor 1, xor 2
        pad = torch.zeros(N, (-NC) % 4, dtype=f)
        x4 = torch.cat([x, pad], 1).reshape(N, -1, 4)
        acc = torch.zeros(N, 4, dtype=f)
        for k in range(x4.shape[1]):
            acc = acc + x4[:, k]
        return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    s, so = lanes(ex), lanes(exo)
    lt = l[ar, t]
    li = mx + torch.log(s) - lt
    u = so / s
    pw = torch.where(u > 0, torch.exp(g * torch.log(u.clamp_min(2.0 ** -149))), one if float(g) == 0 else 0 * one)
    loss = slots(wt * (pw * li)) * (one / W) * a
    if old_loss is not None:
        loss = torch.tensor(old_loss, dtype=f) + loss
    is_ = one / s
    pt = torch.exp(lt - mx) * is_
    r = torch.where(u > 0, li / u.clamp_min(2.0 ** -149), 0 * one)
    br = pw + (g * pt) * (pw * r)
    cb = a * (wt / W) * br
    dl = cb[:, None] * torch.where(oh, -u[:, None], ex * is_[:, None])
    return {'loss': loss.reshape(1), 'dlogits': dl}


assert math.isclose(U, 2.0 ** -24)
