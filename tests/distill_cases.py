"""TRAIN --distill: float64 reference, per-element bound and float32 emulation of ifcbk_softmax_xent_distill (csrc/loss.hip,
softmax_xent_distill_kernel), shared by test_distill_cpu.py and the tests/test_gpu_distill_*.py files.  A plain helper module beside
mix_cases.py and loss_smooth_bounds.py, whose xent_ls() bounds the hard term, and op_bounds.py (notation: u = U = 2^-24, gamma_n, E =
E_LIBM; check_dict() is reused).  No tolerance is chosen anywhere: every term below is one operation of the kernel.

Reference, in float64 from the fp32 values the kernel reads (a = weight, alpha, T, eps as the C ABI rounds them to float; s = logits,
z = teacher; H, Dh = loss and dlogits of loss_smooth_bounds.reference at weight 1):
    r = softmax(s / T),  q = softmax(z / T),  K = 1 / N sum_n sum_j q (log q - log r)
    loss = a ((1 - alpha) H + alpha T^2 K),       d[n][j] = a ((1 - alpha) Dh[n][j] + alpha T / N (r[n][j] - q[n][j]))

What the kernel does beyond softmax_xent_ls_kernel, counted:
    arg_j = fl(fl(x_j - max) / T): a subtraction and a correctly rounded DIVISION (no rounded 1 / T): 2u |arg_j|, an absolute error of
        the exponent and so the same relative error of expf.
    softened probabilities p = r or q: (2u |arg_j| + 2 E u + gamma_NC + 2u) p_j + TINY, as op_bounds.softmax with the second rounding
        of the argument; TINY = 2^-126 covers a result in the denormal range, which has no relative bound, and a q flushed to 0.
        sum^: e_S = sum_j exp(arg_j) (2u |arg_j| + E u) + gamma_NC S;  log S^: e_lS = e_S / S (1 + 2^-10) + E u |log S|  (S >= 1).
    log p_j^ = fl(arg_j^ - log S^): both parts <= 0, so |log p_j| = |arg_j| + log S and nothing cancels:
        e_lp = 2u |arg_j| + e_lS + u (|log p_j| + 2u |arg_j| + e_lS)
    diff^ = fl(log q^ - log r^): e_diff = e_lq + e_lr + u (Lm + e_lq + e_lr),  Lm = |log q| + |log r| -- the difference cancels, the
        bound is on the magnitudes of the pieces.
    term^ = fl(q^ diff^) (an exact 0 when q^ == 0: the true q diff is then below e_q Lm):
        e_term = e_q (Lm + e_diff) + q e_diff,  + u (q Lm + that)
    K_n^: NC terms of either sign, a lane's chain and two butterfly adds: gamma_NC sum_j (q Lm + e_term) + sum_j e_term.
    K^ = fl(fl(sum over slots) * fl(1 / N)): gamma_(N + 1) on sum_n (mag_n + e_Kn) as op_bounds.xent, then 2u.
    loss: ch^ = fl(1 - alpha): u;  cs^ = fl(fl(alpha T) T): gamma_2;  H^ = fl(sum * fl(1 / W^)): loss_smooth_bounds.xent_ls at weight 1
        (which counts one product more);  S1 = fl(ch^ H^): gamma_2;  S2 = fl(cs^ K^): gamma_3 with cs;  the add (fused or not) u of
        |S1| + |S2| plus the errors;  the product with a: u;  one add when accumulating.
    dlogits: the weight a is folded into both factors.  (a Dh)^ exactly as softmax_xent_ls_kernel forms it (g = a / W): xent_ls at
        weight a bounds it;  D1 = fl(ch^ (a Dh)^): gamma_2;  fl(r^ - q^): e_r + e_q + u (r + q + e_r + e_q);
        cd^ = fl(a fl(fl(alpha T) / N)): gamma_3;  D2 = fl(cd^ (r^ - q^)): gamma_4 cd (r + q) -- relative to r + q, never to the
        difference;  the add (fused or not): u of |D1| + cd (r + q) plus the errors.
"""
import numpy as np
import torch

import loss_smooth_bounds as sb
import op_bounds as ob
from op_bounds import E_LIBM, TINY, U, f32, f64, gamma

NS, NCS, SHAPES, WEIGHTS = sb.NS, sb.NCS, sb.SHAPES, sb.WEIGHTS
ALPHAS = (0.0, 0.3, 1.0)
TS = (0.5, 1.0, 4.0)
EPSS = (0.0, 0.1)
SCALES = (1.0, 0.4)
# (alpha, T, eps, weight, class weights, offset variant, loss_accumulate, with dlogits): every value of every parameter, run at every shape
CASES = [
    (0.3, 4.0, 0.1, 1.0, 'random', False, 0, 1),
    (0.3, 1.0, 0.0, 0.4, 'none', False, 1, 1),
    (1.0, 0.5, 0.0, 1.0, 'none', True, 0, 1),
    (0.0, 4.0, 0.1, 0.4, 'zero', False, 1, 0),
    (1.0, 4.0, 0.1, 0.4, 'random', True, 1, 1),
    (0.0, 0.5, 0.0, 1.0, 'random', False, 0, 1),
    (0.3, 0.5, 0.1, 1.0, 'zero', True, 0, 0),
    (0.3, 1.0, 0.1, 0.4, 'none', True, 1, 1),
    (1.0, 1.0, 0.0, 1.0, 'zero', False, 0, 1),
    (0.0, 1.0, 0.1, 1.0, 'none', False, 0, 1),
]
OLD_LOSS = 5.0                     # what loss_out holds before an accumulating call


def case_name(N, NC, case):
    return 'distill (%d, %d) alpha %g T %g eps %g weight %g %s%s acc %d dlogits %d' % ((N, NC) + case[:5] + (' offset' if case[5] else '',) + case[6:])


def inputs(N, NC, weights='random', offset=False, seed=0):
    """(logits, target, teacher, class_weight or None): student and teacher logits independent randn * 4; target and class weights as
    loss_smooth_bounds.inputs draws them.  offset: + 80 on one student row and + 80 on a different teacher row (the same one when
    N == 1) -- a shift of a whole row, which only the subtraction of the maximum sees -- and one element of that teacher row raised by
    another 1000, so that every other q of the row underflows to an exact 0 at every temperature of TS while r does not."""
    l, t, cw = sb.inputs(N, NC, weights)
    gen = torch.Generator().manual_seed(7000 * N + NC + 31 * seed)
    z = torch.randn(N, NC, generator=gen) * 4.0
    if offset:
        l = l.clone()
        l[N // 2] += 80.0
        row = (N // 2 + 1) % N
        z[row] += 80.0
        z[row, (3 * N + 1) % NC] += 1000.0
    return l, t, z, cw


def reference(logits, target, teacher, class_weight, weight, eps, alpha, T):
    """(loss, dlogits) in float64, from the definition alone"""
    a, alpha, T = f32(weight), f32(alpha), f32(T)
    H, Dh = sb.reference(logits, target, class_weight, 1.0, eps)
    s, z = f64(logits), f64(teacher)
    N = s.shape[0]
    logr, logq = torch.log_softmax(s / T, 1), torch.log_softmax(z / T, 1)
    r, q = logr.exp(), logq.exp()
    K = torch.where(q > 0, q * (logq - logr), torch.zeros_like(q)).sum() / N
    return a * ((1.0 - alpha) * H + alpha * T * T * K), a * ((1.0 - alpha) * Dh + alpha * T / N * (r - q))


def _soft(x, T):
    """softmax(x / T) as the kernel forms it -> (p, e_p, log p, e_logp, |log p|)"""
    mx = x.max(1, keepdim=True).values
    arg = (x - mx) / T
    ex = torch.exp(arg)
    S = ex.sum(1, keepdim=True)
    p = ex / S
    NC = x.shape[1]
    e_p = (2 * U * arg.abs() + 2 * E_LIBM * U + gamma(NC) + 2 * U) * p * (1 + 2.0 ** -10) + TINY
    e_S = (ex * (2 * U * arg.abs() + E_LIBM * U)).sum(1, keepdim=True) + gamma(NC) * S
    lS = torch.log(S)
    e_lS = e_S / S * (1 + 2.0 ** -10) + E_LIBM * U * lS.abs()
    logp = arg - lS
    mag = arg.abs() + lS
    e_lp = 2 * U * arg.abs() + e_lS + U * (mag + 2 * U * arg.abs() + e_lS)
    return p, e_p, logp, e_lp, mag


def bounds(logits, target, teacher, class_weight, weight, eps, alpha, T, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of ifcbk_softmax_xent_distill; class_weight None = all ones"""
    a, alpha, T = f32(weight), f32(alpha), f32(T)
    s, z = f64(logits), f64(teacher)
    N, NC = s.shape
    hard = sb.xent_ls(logits, target, class_weight, 1.0, eps)
    Dh, e_Dh = sb.xent_ls(logits, target, class_weight, weight, eps)['dlogits']          # a Dh: the weight is folded in
    H, e_H = hard['loss'][0][0], hard['loss'][1][0]
    r, e_r, logr, e_lr, mag_r = _soft(s, T)
    q, e_q, logq, e_lq, mag_q = _soft(z, T)
    ch, cs, cd = 1.0 - alpha, alpha * T * T, alpha * T / N
    # ---- dlogits
    cda = abs(a) * cd
    D1, D2 = ch * Dh, a * cd * (r - q)
    e_D1 = ch * e_Dh * (1 + gamma(2)) + gamma(2) * D1.abs()
    e_sub = e_r + e_q + U * (r + q + e_r + e_q)
    e_D2 = cda * e_sub * (1 + gamma(4)) + gamma(4) * cda * (r + q)
    dl = D1 + D2
    e_dl = e_D1 + e_D2 + U * (D1.abs() + cda * (r + q) + e_D1 + e_D2)
    # ---- loss
    Lm = mag_q + mag_r
    e_diff = e_lq + e_lr + U * (Lm + e_lq + e_lr)
    e_t0 = e_q * (Lm + e_diff) + q * e_diff
    e_term = e_t0 + U * (q * Lm + e_t0)
    mag_n = (q * Lm).sum(1)
    e_Kn = gamma(NC) * (mag_n + e_term.sum(1)) + e_term.sum(1)
    K = torch.where(q > 0, q * (logq - logr), torch.zeros_like(q)).sum() / N
    e_K = (gamma(N + 1) * (mag_n + e_Kn).sum() + e_Kn.sum()) / N
    e_K = e_K + 2 * U * (mag_n.sum() / N + e_K)
    S1, S2 = ch * H, cs * K
    e_S1 = ch * e_H * (1 + gamma(2)) + gamma(2) * S1.abs()
    e_S2 = cs * e_K * (1 + gamma(3)) + gamma(3) * cs * (K.abs() + e_K)
    e_sum = e_S1 + e_S2 + U * (S1.abs() + S2.abs() + e_S1 + e_S2)
    loss = a * (S1 + S2)
    e = abs(a) * e_sum * (1 + U) + U * loss.abs()
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


def emulate(logits, target, teacher, class_weight, weight, eps, alpha, T, old_loss=None):
    """softmax_xent_distill_kernel's operations in its order, in numpy float32 (numpy's exp / log for the device's; products and sums
    rounded one by one, where the device may fuse a multiply-add): {'loss': [1], 'dlogits': [N, NC]}.  Rows are carried as arrays; the
    lane chains over the classes and the slot chains over the rows run in the kernel's order."""
    F = np.float32
    l, z = logits.numpy().astype(F), teacher.numpy().astype(F)
    N, NC = l.shape
    t = target.numpy().astype(np.int64)
    w = np.ones(NC, F) if class_weight is None else class_weight.numpy().astype(F)
    wgt, eps, alpha, T = F(weight), F(eps), F(alpha), F(T)
    rows = np.arange(N)

    def slots(v):
        """256 slot chains (slot s: elements s, s + 256, ... in order), then the chain over the slots"""
        part = np.zeros(256, F)
        for n in range(len(v)):
            part[n % 256] = part[n % 256] + v[n]
        tot = F(0)
        for i in range(256):
            tot = F(tot + part[i])
        return tot

    def lanes(vals, zero):
        """[N, NC] -> [N]: four lane chains over j = sub, sub + 4, ... from ``zero`` and the two butterflies"""
        acc = [np.full(N, zero, F) for _ in range(4)]
        for j in range(NC):
            acc[j % 4] = (acc[j % 4] + vals[:, j]).astype(F)
        return ((acc[0] + acc[1]).astype(F) + (acc[2] + acc[3]).astype(F)).astype(F)
    with np.errstate(all='ignore'):
        W, SW = slots(w[t]), slots(w)
        invW = F(1) / W
        c1, eC = F(1) - eps, eps / F(NC)
        ch, cs, cd = F(1) - alpha, F(F(alpha * T) * T), F(wgt * F(F(alpha * T) / F(N)))
        g = wgt / W
        mx, mz = l.max(1, keepdims=True), z.max(1, keepdims=True)
        dl_, dz_ = (l - mx).astype(F), (z - mz).astype(F)
        ar, aq = (dl_ / T).astype(F), (dz_ / T).astype(F)
        ex, er, eq = np.exp(dl_).astype(F), np.exp(ar).astype(F), np.exp(aq).astype(F)
        s, sr, sq = lanes(ex, 0), lanes(er, 0), lanes(eq, 0)
        ls, lsr, lsq = np.log(s).astype(F), np.log(sr).astype(F), np.log(sq).astype(F)
        isr, isq = (F(1) / sr).astype(F), (F(1) / sq).astype(F)
        pieces = (w[None] * (((mx - l).astype(F) + ls[:, None]).astype(F))).astype(F)
        qs = lanes(pieces, 0)
        qj = (eq * isq[:, None]).astype(F)
        rj = (er * isr[:, None]).astype(F)
        diff = ((aq - lsq[:, None]).astype(F) - (ar - lsr[:, None]).astype(F)).astype(F)
        term = np.where(qj > 0, (qj * diff).astype(F), F(0)).astype(F)
        kl = lanes(term, 0)
        wt = w[t]
        hard = (c1 * wt).astype(F)
        li = ((mx[:, 0] + ls).astype(F) - l[rows, t]).astype(F)
        hterm = ((c1 * (wt * li).astype(F)).astype(F) + (eC * qs).astype(F)).astype(F)
        Hs, Ks = slots(hterm), slots(kl)
        is_ = (F(1) / s).astype(F)
        A = (hard + F(eC * SW)).astype(F)
        oh = np.zeros((N, NC), F)
        oh[rows, t] = 1
        v = (A[:, None] * (ex * is_[:, None]).astype(F)).astype(F)
        v = (v - (oh * hard[:, None]).astype(F)).astype(F)
        v = (v - (eC * w[None]).astype(F)).astype(F)
        dh = (g * v).astype(F)
        soft = (cd * (rj - qj).astype(F)).astype(F)
        dl = ((ch * dh).astype(F) + soft).astype(F)
        H = F(Hs * invW)
        K = F(Ks * F(F(1) / F(N)))
        tot = F(wgt * F(F(ch * H) + F(cs * K)))
        if old_loss is not None:
            tot = F(F(old_loss) + tot)
    return {'loss': torch.tensor([tot]), 'dlogits': torch.from_numpy(dl)}


def check(name, got, want, family=None, raise_=True):
    """op_bounds.check_dict: |got - want| <= 1/2 ulp(|want| + e) + e per element; returns the worst err / bound"""
    return ob.check_dict(name, got, want, family=family, raise_=raise_)
