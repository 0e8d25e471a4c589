"""TRAIN --mixup / --cutmix: float64 references and per-element bounds of the two kernels, shared by test_mix_cpu.py and the
tests/test_gpu_mix_*.py files.  A plain helper module beside loss_smooth_bounds.py, whose count this one extends term by term, and
op_bounds.py (notation: u = U = 2^-24, gamma_n, E_LIBM; softmax() and check_dict() are reused).

---- ifcbk_batch_mix (csrc/batch_mix.hip).  Partner of image n: m = N - 1 - n.  Exact value, in float64 from the stored inputs and the
fp32 factor:  inside the box x[m]; outside it lam[n] x[n] + (1 - lam[n]) x[m].  The kernel forms d = fl(a - b) and v = fl(lam d + b), one
fused rounding:
    dense fp32   |v - exact| <= lam u |a - b| + u |v|  <=  2u (|a| + |b|)                                   (E_F32 below)
    dense bf16   the same v, then one round-to-nearest-even to bf16: 2^-8 |exact| (half a bf16 ulp, relative 2^-9 ... 2^-8) on top
    u8           a - b is an integer, exact; v carries one rounding, at most 2^-17 below 256, and v + 0.5f a second one: the result is
                 floor(exact + 0.5) unless the fractional part of exact lies within 2^-16 of 0.5.  The test allows either neighbour
                 within AMBIG = 1e-3 of 0.5 and caps the share of such elements at AMBIG_MAX = 1 % per case.
    lam == 1 rows, box pixels and the middle image of an odd batch are copies: compared for equality.

---- ifcbk_softmax_xent_mix (csrc/loss.hip).  Reference as the issue states it, in float64 from the fp32 values the kernel reads:
    a = t[n], b = t[N-1-n], ta = lam_n w[a], tb = (1 - lam_n) w[b], h_n = ta + tb, W = sum h_n, SW = sum w, c1 = 1 - eps, eC = eps / NC
    loss = wgt / W sum_n [ c1 (ta L_a + tb L_b) + eC q_n ],   L_k = -log p[n][k],  q_n = sum_j w[j] L_j
    d[n][j] = wgt / W [ (c1 h_n + eC SW) p[n][j] - c1 ta [j = a] - c1 tb [j = b] - eC w[j] ]
What the kernel does beyond softmax_xent_ls_kernel (loss_smooth_bounds' docstring counts that one), counted:
    ta^ = fl(lam w_a): u.  om^ = fl(1 - lam): u.  tb^ = fl(om^ w_b): gamma_2.  h^ = fl(ta^ + tb^): non-negative terms, gamma_3.
    W^: N non-negative terms h^ in a fixed order: gamma_(N + 3) in all; r_W = gamma_(N + 3) / (1 - gamma_(N + 3)).
    A^ = fl(c1^ h^ + eC^ SW^): non-negative terms; the first carries c1 (u), h (gamma_3), the product and the add: gamma_6; the second
        gamma_NC + 3u as there:  r_A = gamma_(NC + 6) covers both.
    T2a = fl(c1^ ta^): gamma_3;  T2b = fl(c1^ tb^): gamma_4 -- gamma_4 for both.  T3 = fl(eC^ w_j): gamma_2.
    three subtractions from A^ p^ (two when a != b meet different j; counted as three): 3u of M = A p + T2a + T2b + T3 plus the errors.
    loss term: fl(c1^ * fl(fl(ta^ L_a^) + fl(tb^ L_b^)) + eC^ q^): h1 = c1 (ta L_a + tb L_b), each product chain at most gamma_6 (c1,
        lam / 1 - lam, the weight product, the L product, the inner add, the c1 product); L_k^ carries e_i of op_bounds.xent.
    The rest -- q_n, the slot sums, 1 / W^, the accumulate -- is loss_smooth_bounds.xent_ls's, with this r_W.
"""
import numpy as np
import torch

import op_bounds as ob
from op_bounds import E_LIBM, U, f32, f64, gamma

AMBIG = 1e-3               # u8: distance of the exact value's fractional part from 0.5 below which either neighbour passes
AMBIG_MAX = 0.01           # ... and the largest share of such elements per case

# ------------------------------------------------------------------------------------------------------ batch mix
MIX_S = (5, 16, 299)
MIX_N = (1, 2, 3, 8)


def boxes(S):
    """the boxes of the issue's list: empty, one pixel, a full row band, the whole image, one touching each of the four edges"""
    h = max(1, S // 3)
    return {'empty': (0, 0, 0, 0), 'pixel': (S // 2, S // 2 + 1, S // 2, S // 2 + 1), 'band': (S // 3, S // 3 + h, 0, S),
            'all': (0, S, 0, S), 'top': (0, h, 1, S - 1), 'bottom': (S - h, S, 1, S - 1), 'left': (1, S - 1, 0, h),
            'right': (1, S - 1, S - h, S)}


def lam_rows(N, seed=0):
    """per-image factors that differ from row to row and hold exactly 0, 1 and 0.5 (as far as N allows)"""
    g = torch.Generator().manual_seed(77 + 13 * N + seed)
    lam = torch.rand(N, generator=g)
    for k, v in enumerate((1.0, 0.0, 0.5)):
        if k < N:
            lam[(k * 3 + seed) % N if N > 3 else k] = v
    return lam.float()


def u8_batch(N, S, seed=0, lam=None):
    """random bytes.  With ``lam``: the partner of a row whose factor is exactly 0.5 gets that row's parity, so that a - b is even there
    and lam (a - b) + b an integer -- otherwise half of such a row would sit exactly on a rounding tie and count against AMBIG_MAX"""
    g = torch.Generator().manual_seed(1000 * S + N + seed)
    x = torch.randint(0, 256, (N, S, S), dtype=torch.uint8, generator=g)
    for n in range(N if lam is not None else 0):
        if float(lam[n]) == 0.5 and n != N - 1 - n:
            x[N - 1 - n] = (x[N - 1 - n] & 0xFE) | (x[n] & 1)
    return x


def dense_from_u8(x8, dtype):
    """[N,S,S] u8 -> [N,S,S,8] of the engine's dense layout: three normalised channels and five zero ones"""
    x = x8.float()[..., None] / 255.0
    mean = torch.tensor([0.485, 0.456, 0.406])
    std = torch.tensor([0.229, 0.224, 0.225])
    out = torch.zeros(x8.shape + (8,), dtype=torch.float32)
    out[..., :3] = (x - mean) / std
    return out.to(dtype)


def mix_reference(x, lam, box):
    """-> (exact float64 values, copy mask, |a| + |b|): x [N,S,S] or [N,S,S,C] of any dtype, lam float32 [N], box (y0, y1, x0, x1).
    copy: elements that are plain copies (box pixels, rows with lam == 1, the middle image of an odd batch)"""
    xd = f64(x)
    N = xd.shape[0]
    part = xd.flip(0)
    l = f64(lam).reshape((N,) + (1,) * (xd.dim() - 1))
    exact = l * xd + (1.0 - l) * part
    copy = (l == 1.0).expand_as(xd).clone()
    y0, y1, x0, x1 = box
    exact[:, y0:y1, x0:x1] = part[:, y0:y1, x0:x1]
    copy[:, y0:y1, x0:x1] = True
    if N % 2:
        exact[N // 2] = xd[N // 2]
        copy[N // 2] = True
    return exact, copy, xd.abs() + part.abs()


def _report(name, err, bound):
    ratio = err / bound
    k = int(ratio.argmax())
    worst = float(ratio.reshape(-1)[k])
    if worst > 1.0:
        idx = np.unravel_index(k, tuple(ratio.shape))
        raise AssertionError('%s: element %s err %.3e > bound %.3e (err/bound %.3f)'
                             % (name, idx, float(err.reshape(-1)[k]), float(bound.reshape(-1)[k]), worst))
    return worst


def check_mix_dense(name, got, x, lam, box, out):
    """dense form: out 'f32' or 'bf16'; -> worst err / bound"""
    exact, copy, mag = mix_reference(x, lam, box)
    g = f64(got)
    want_copy = torch.where(copy, exact, g)
    assert torch.equal(torch.where(copy, g, want_copy), want_copy), '%s: a copied element (box, lam == 1, middle image) changed' % name
    bound = 2 * U * mag + (2.0 ** -8 * exact.abs() if out == 'bf16' else 0.0) + 2.0 ** -140
    return _report(name, (g - exact).abs(), bound)


def u8_verdict(got, exact):
    """-> (wrong, ambiguous share): got must be floor(exact + 0.5) unless frac(exact) is within AMBIG of 0.5, where either neighbour passes"""
    g = f64(got)
    fr = exact - torch.floor(exact)
    amb = (fr - 0.5).abs() <= AMBIG
    want = torch.floor(exact + 0.5)
    ok = (g == want) | (amb & ((g == torch.floor(exact)) | (g == torch.floor(exact) + 1)))
    return ~ok, float(amb.double().mean())


def check_mix_u8(name, got, x, lam, box):
    exact, copy, _ = mix_reference(x, lam, box)
    g = f64(got)
    assert torch.equal(g[copy], exact[copy]), '%s: a copied byte (box, lam == 1, middle image) changed' % name
    wrong, share = u8_verdict(got, exact)
    assert share <= AMBIG_MAX, '%s: %.4f of the elements lie within %g of a rounding tie' % (name, share, AMBIG)
    assert not bool(wrong.any()), '%s: %d bytes differ from floor(exact + 0.5), first at %s' % (
        name, int(wrong.sum()), tuple(int(v) for v in wrong.nonzero()[0]))
    return share


# ------------------------------------------------------------------------------------------------------ two-target loss
LOSS_NS = (1, 2, 3, 257)          # 257 crosses the 256-slot loop and is odd
LOSS_NCS = (1, 3, 5, 100)         # NC that is no multiple of 4 reaches the lane tail
WEIGHTS = ('none', 'random', 'zero')
EPSS = (0.0, 0.1, 1.0)
LAMS = ('rows', 'ones', 'zeros', 'half')


def loss_inputs(N, NC, weights='random', lam='rows', spread=4.0):
    """(logits, target, lam, class_weight or None): logits randn * spread (spread 30: some rows +-30 apart and more), a quarter of the
    rows with a == b, weights 'none', 'random' in [0.1, 1.1] or 'zero': one class -- the one fewest targets name -- at 0"""
    g = torch.Generator().manual_seed(5000 * N + NC)
    l = torch.randn(N, NC, generator=g) * spread
    t = torch.randint(0, NC, (N,), generator=g)
    for n in range(0, N // 2, 4):
        t[N - 1 - n] = t[n]                                   # rows whose two targets coincide (the middle row of an odd N always does)
    cw = torch.rand(NC, generator=g) + 0.1
    lm = {'rows': torch.rand(N, generator=g), 'ones': torch.ones(N), 'zeros': torch.zeros(N), 'half': torch.full((N,), 0.5)}[lam].float()
    if weights == 'none':
        return l, t, lm, None
    if weights == 'zero':
        cw[int(torch.bincount(t, minlength=NC).argmin())] = 0.0
    return l, t, lm, cw


def loss_reference(logits, target, lam, class_weight, weight, eps):
    """(loss, dlogits) in float64, from the definition alone"""
    l = f64(logits)
    N, NC = l.shape
    wgt, eps = f32(weight), f32(eps)
    a = target.cpu().long()
    b = a.flip(0)
    lm = f64(lam)
    w = torch.ones(NC, dtype=torch.float64) if class_weight is None else f64(class_weight)
    ta, tb = lm * w[a], (1.0 - lm) * w[b]
    W, SW = (ta + tb).sum(), w.sum()
    c1, eC = 1.0 - eps, eps / NC
    logp = torch.log_softmax(l, 1)
    p = logp.exp()
    r = torch.arange(N)
    oa, ob_ = torch.zeros_like(p), torch.zeros_like(p)
    oa[r, a] = 1.0
    ob_[r, b] = 1.0
    loss = wgt / W * (c1 * (ta * -logp[r, a] + tb * -logp[r, b]) + eC * (w[None] * -logp).sum(1)).sum()
    dl = wgt / W * ((c1 * (ta + tb) + eC * SW)[:, None] * p - c1 * ta[:, None] * oa - c1 * tb[:, None] * ob_ - eC * w[None])
    return loss, dl


def xent_mix(logits, target, lam, class_weight, weight, eps, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of ifcbk_softmax_xent_mix; class_weight None = all ones"""
    l = f64(logits)
    N, NC = l.shape
    wgt, eps = f32(weight), f32(eps)
    a = target.cpu().long()
    b = a.flip(0)
    lm = f64(lam)[:, None]
    w = (torch.ones(NC, dtype=torch.float64) if class_weight is None else f64(class_weight))[None]
    ta, tb = lm * w[0][a][:, None], (1.0 - lm) * w[0][b][:, None]
    h = ta + tb
    W, SW = h.sum(), w.sum()
    c1, eC = 1.0 - eps, eps / NC
    r_W = gamma(N + 3) / (1 - gamma(N + 3))
    r_A = gamma(NC + 6)
    r_T = r_A + U + r_A * U
    r_g = r_W + U * (1 + r_W)
    r_c = r_g + U + r_g * U
    p, e_p, (mx, s, e_s) = ob.softmax(l)
    r = torch.arange(N)
    oa, ob_ = torch.zeros_like(p), torch.zeros_like(p)
    oa[r, a] = 1.0
    ob_[r, b] = 1.0
    # ---- dlogits
    A = c1 * h + eC * SW
    T1, T2, T3 = A * p, c1 * ta * oa + c1 * tb * ob_, eC * w.expand_as(p)
    e_T = A * e_p * (1 + r_T) + r_T * T1 + gamma(4) * T2 + gamma(2) * T3
    M = T1 + T2 + T3
    e_in = e_T + 3 * U * (M + e_T)
    g = wgt / W
    dl = g * (T1 - T2 - T3)
    e_dl = abs(g) * e_in * (1 + r_c) + r_c * dl.abs()
    # ---- loss
    ls = torch.log(s)
    e_ls = e_s / s * (1 + 2.0 ** -10) + E_LIBM * U * ls.abs()
    la_, lb_ = l[r, a][:, None], l[r, b][:, None]
    lia, lib = mx + ls - la_, mx + ls - lb_
    e_ia = e_ls + 2 * U * (mx.abs() + ls.abs() + la_.abs())
    e_ib = e_ls + 2 * U * (mx.abs() + ls.abs() + lb_.abs())
    d = mx - l
    bb = d + ls
    e_b = U * d + e_ls + U * (d + ls + U * d + e_ls)
    e_piece = w * e_b * (1 + U) + U * w * bb
    q = (w * bb).sum(1, keepdim=True)
    e_q = gamma(NC) * (q + e_piece.sum(1, keepdim=True)) + e_piece.sum(1, keepdim=True)
    h1a, h1b, h2 = c1 * ta * lia, c1 * tb * lib, eC * q
    e_h1 = gamma(6) * (h1a.abs() + h1b.abs()) + c1 * (ta * e_ia + tb * e_ib) * (1 + gamma(6))
    e_h2 = gamma(2) * h2 + eC * e_q * (1 + gamma(2))
    mag = h1a.abs() + h1b.abs() + h2
    e_term = e_h1 + e_h2 + U * (mag + e_h1 + e_h2)
    loss = wgt / W * (h1a + h1b + h2).sum()
    e = abs(wgt) / W * (gamma(N + 1) * (mag + e_term).sum() + e_term.sum())
    e = e + (3 * U + r_W) * (loss.abs() + e)
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


def emulate_f32(logits, target, lam, class_weight, weight, eps, old_loss=None):
    """softmax_xent_mix_kernel's operations in its order, in numpy float32 (numpy's exp / log for the device's; products and sums rounded
    one by one, where the device may fuse a multiply-add): {'loss': [1], 'dlogits': [N, NC]}"""
    F = np.float32
    l = logits.numpy().astype(F)
    N, NC = l.shape
    a = target.numpy().astype(np.int64)
    b = a[::-1].copy()
    lm = lam.numpy().astype(F)
    w = np.ones(NC, F) if class_weight is None else class_weight.numpy().astype(F)
    wgt, eps = F(weight), F(eps)
    ta = lm * w[a]
    tb = (F(1) - lm) * w[b]
    h = ta + tb
    slots = np.zeros(256, F)
    for n in range(N):
        slots[n % 256] = slots[n % 256] + h[n]
    kslots = np.zeros(256, F)
    for k in range(NC):
        kslots[k % 256] = kslots[k % 256] + w[k]
    W, SW = F(0), F(0)
    for i in range(256):
        W = W + slots[i]
        SW = SW + kslots[i]
    invW, g = F(1) / W, wgt / W
    c1, eC = F(1) - eps, eps / F(NC)

    def lanes(vals, op):
        """four lane chains over j = sub, sub + 4, ... and the two butterflies"""
        acc = []
        for sub in range(4):
            v = None
            for j in range(sub, NC, 4):
                v = vals[j] if v is None else op(v, vals[j])
            acc.append(v)
        return acc
    local = np.zeros(256, F)
    dl = np.zeros((N, NC), F)
    for n in range(N):
        mxs = [v if v is not None else F(-np.inf) for v in lanes(l[n], max)]
        mx = max(max(mxs[0], mxs[1]), max(mxs[2], mxs[3]))
        ex = np.exp(l[n] - mx).astype(F)
        ss = [v if v is not None else F(0) for v in lanes(ex, lambda x, y: F(x + y))]
        s = F(F(ss[0] + ss[1]) + F(ss[2] + ss[3]))
        ls = np.log(s).astype(F)
        pieces = (w * ((mx - l[n]) + ls)).astype(F)
        qs = [v if v is not None else F(0) for v in lanes(pieces, lambda x, y: F(x + y))]
        q = F(F(qs[0] + qs[1]) + F(qs[2] + qs[3]))
        lia, lib = F(F(mx + ls) - l[n][a[n]]), F(F(mx + ls) - l[n][b[n]])
        term = F(F(c1 * F(F(ta[n] * lia) + F(tb[n] * lib))) + F(eC * q))
        local[n % 256] = local[n % 256] + term
        is_ = F(1) / s
        ha, hb = F(c1 * ta[n]), F(c1 * tb[n])
        A = F(F(c1 * h[n]) + F(eC * SW))
        for j in range(NC):
            v = F(A * F(ex[j] * is_))
            v = F(v - (ha if j == a[n] else F(0)))
            v = F(v - (hb if j == b[n] else F(0)))
            v = F(v - F(eC * w[j]))
            dl[n][j] = F(g * v)
    tot = F(0)
    for i in range(256):
        tot = tot + local[i]
    tot = F(F(tot * invW) * wgt)
    if old_loss is not None:
        tot = F(F(old_loss) + tot)
    return {'loss': torch.tensor([tot]), 'dlogits': torch.from_numpy(dl)}


def check(name, got, want, family=None, raise_=True):
    """op_bounds.check_dict: |got - want| <= 1/2 ulp(|want| + e) + e per element; returns the worst err / bound"""
    return ob.check_dict(name, got, want, family=family, raise_=raise_)
