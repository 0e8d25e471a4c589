"""Per-element error bounds for the kernels around the convolutions (bn.hip, pool_head.hip, plain.hip), against float64 references.

A plain helper module like conv_bounds.py, whose U, gamma, ulp, rne, _finish, _record and MISMATCH_MAX it reuses.  Everything here runs
on the CPU in float64, from the values the kernel read: bf16- or fp32-representable tensors and the fp32 mean / invstd / scale / shift
arrays as handed to the kernel.  Lines in the measured section of the log start with 'op bound'.

Notation: u = 2^-24, gamma_n = n u / (1 - n u); a fp32 sum of n terms in any order is within gamma_(n-1) * sum |terms|; every bound
below ends with the store, 1/2 ulp_out taken at |want| + e (e: everything before the store).  The library is built with
-ffp-contract=on and without fast-math flags (csrc/Makefile, checked by test_op_inventory_cpu.py): a * b + c is one rounding or two,
sqrtf and / are correctly rounded (one u each).

Elementwise affine  y = act(x * s + b (+ r))   [bn_apply, bn_apply_maxpool, nchw_to_nhwc, avgpool3x3_affine's epilogue]
    e = 2u (|x s| + |b|)  (+ u (|x s| + |b| + |r|) for the residual add);  the ReLU is 1-Lipschitz.
    dropout_apply  y (+)= x * scale: one rounding, one more for the add.  flatten_chw, nhwc_to_nchw, bias_relu_bwd's dz: copies (exact).

Pools
    max forward: values and arg-max bit-exact against the rule of maxpool_fwd_kernel: taps in row-major order, a tap replaces the
      best when it is the first valid one, when it is greater, or when it is NaN (so NaN takes the window).
    max backward: n = ceil(R / sh) * ceil(S / sw) terms (4 in the 3x3 / stride-2 kernel): e = gamma_n * sum |terms|.
    average (forward, and backward with its n windows): n terms, the rounding of 1 / (R S) and of the product:
      e = gamma_(n + 2) * sum |x| / (R S).
    accumulate: the old value joins the fp32 sum as one more term, want = old + ref, e = gamma_(n + 1) (A + |old|) -- conv_bounds.check's
      rule without its staging term (these kernels add in fp32 registers and store once).
    avgpool3x3_affine rounds the average to the storage type, then applies the affine: e_avg + 1/2 ulp_out(avg) goes through |s|;
      either rounding model counts as a match (as conv_bounds.check_affine).

BatchNorm statistics
    bn_stats partial rows: conv_bounds.check_sums per row tile (1024 rows, fp32) and in total.
    bn_finalize (the rows are its input; reference: their float64 sum).  The kernel sums in double (d = 2^-53 per add) and rounds once:
      e_S = rows * d * sum |rows|                  (+ u * sum |rows| in the prereduce route: its 64-row chunks are stored as fp32)
      mean:    2u |mean| + e_S1 / M
      var = E[x^2] - mean^2 in double, stated relative to E2 + mean^2, never to the variance:
               e_var = e_S2 / M + 2 |mean| e_S1 / M + 4 d (E2 + mean^2)
      invstd:  (2u + e_var / (2 (var + eps))) invstd
      scale = gamma * invstd: |gamma| e_invstd + u |scale|;   shift = beta - mean_f32 * scale: |scale| e_mean + |mean| e_scale + 2u (|mean scale| + |beta|)
      running_mean = c1 * rm + mom * mean_f32, c1 = fl(1 - mom) taken as an input: two roundings per term, 2u (|c1 rm| + |mom mean|) + mom e_mean
      running_var: the same plus the conversion of var * unbias to fp32, a third rounding the source has: gamma_3 (...) + mom unbias e_var.
      eval form (bn_eval_scale_kernel): rvar + eps, sqrtf, /: 3u on scale; shift as above.

BatchNorm backward  (dz = dy where the ReLU passed)
    dbeta = sum dz, dgamma = sum dz * ((x - mean) * invstd): conv_bounds.check_sums with n = the fp32 row tile (the tiles are combined
      in double and rounded once) and mags = |dz| (|x| + |mean|) invstd (the roundings of a term act on these); param_accumulate adds
      the old value as one more term.
    dx = A dz + (B x + K),  A = gamma invstd,  B = -A invstd dgamma / M,  K = A (mean invstd dgamma / M - dbeta / M).  Counted in
      bn_bwd_dx_kernel: A 1 rounding; dgamma / M and dbeta / M 2 each (fl(1 / M), the product); B 2 more (5); K: mean * invstd 1,
      * dg 1, the subtraction 1, * A 1 (7 with A and dg):
        e_B = gamma_5 |B| + |A invstd| e_dgamma / M,     e_K = |A| (gamma_7 (|T| + |db|) + |mean invstd| e_dgamma / M + e_dbeta / M)
        e   = u |A dz| + |A| e_dz + e_B |x| + e_K + 2u (|B x| + |K|) + 2u (|A dz| + |B x| + |K|)
      relative to |A dz| + |B x| + |K|, never to |dx|.  e_dgamma, e_dbeta: the sum bounds above; e_dz: 0, or gamma_3 * sum |terms| when
      dz is gathered from a pooled gradient (bn_bwd_maxpool, up to 4 terms).  dx accumulating (dres_accumulate bit 1): one more add.
    recomputed mask (x * scale + shift > 0): an element with |pre| <= 4u (|x scale| + |shift|) may fall on either side: both values are
      accepted for it and its term joins the sum bounds.  At most 1e-4 of a case's elements may be treated so (asserted).
    dres (+)= dz: a copy, or one add.

Head
    gap: HW terms, fl(1 / HW), the product, the mask product: gamma_(HW + 3).  fc forward: C products and the bias: gamma_(C + 2).
    fc_wgrad / fc_bgrad: N terms (+ the old value): gamma_(N + 2).  head_dx: NC terms, fl(1 / HW), two products: gamma_(NC + 3); all HW copies.

Softmax and cross-entropy   (E = ulp error of the device expf / logf)
    The ROCm installation this was written against ships no document with ulp figures for its device maths library, so
    E = 4: the OpenCL full-profile limit of 3 ulp for exp / log, plus one.  (A bf16-rounded intermediate is 2^15 u.)
    l_j - max is rounded: an absolute error u |l_j - max| in the exponent is the same relative error in exp:
        p_j:  (u |l_j - max| + 2 E u + gamma_NC + 2u) p_j        (numerator and sum each carry E; 1 / s and the product: 2u)
        dlogits = w / N * (p - onehot):  |w / N| (e_p + u (p + onehot)) + 3u |dlogits|
        loss_i = max + log s - l_t:  e_s / s + E u |log s| + 2u (|max| + |log s| + |l_t|),   e_s = sum_j exp(.) (u |l_j - max| + E u) + gamma_NC s
        loss = w / N * sum_i: gamma_(N + 1) sum |loss_i| + sum e_i, 3u for fl(1 / N) and the two products, one add when accumulating.

Adam, SGD (one step from the kernel's own fp32 state; scalars as rounded to fp32 by the call)
    gr = g * gs + wd * p: gamma_2 (|g gs| + |wd p|).   m' = b1 m + (1 - b1) gr: gamma_2 |b1 m| + gamma_3 (1 - b1) |gr| + (1 - b1) e_gr.
    v' = b2 v + ((1 - b2) gr) gr: gamma_2 |b2 v| + gamma_4 (1 - b2) gr^2 + (1 - b2) (2 |gr| e_gr + e_gr^2).
    host: bc1 = 1 - powf(b1, t), sbc2 = sqrtf(1 - powf(b2, t)), powf within 1 ulp (2u):  r_bc = 2u b^t / (1 - b^t) + u,  r_sbc2 = r_bc2 / 2 + u.
    denom = sqrtf(v') / sbc2 + eps:  r_sqrt = e_v / (2 v' (1 - e_v / v')) + u;  a = sqrt(v') / sbc2: r_a = r_sqrt + r_sbc2 + u;
        e_denom = a r_a + u (a + eps).     q = m' / denom: e_q = (e_m + |m'| r_d) / (denom (1 - r_d)) + u (|q| + that).
    p' = p - (lr / bc1) q: e_step = |lr / bc1| (e_q (1 + r_bc1 + 3u) + |q| (r_bc1 + 2u));  e_p = e_step + u (|p'| + e_step).
    SGD: b = mu mom + gr: e_gr + gamma_2 (|mu mom| + |gr|);  p' = p - lr b: lr e_b + 2u (|p| + |lr b|).

Bf16 outputs keep the sensitivity check of conv_bounds: at most MISMATCH_MAX of the elements may differ from the correctly rounded
float64 value (or from the designed second rounding model, where one is named above).

Out of scope: the 32-bit index paths (fdiv on indices near 2^31, the `total >= 2^31` guards).  Nothing here needs such sizes.
"""
import contextlib
import math

import torch

import conv_bounds as cb
from conv_bounds import MISMATCH_MAX, U, _finish, _record, gamma, rne, ulp      # noqa: F401  (re-exported for the tests)

PREFIX = 'op bound'
D = 2.0 ** -53
E_LIBM = 4.0                # ulp error allowed for the device expf / logf (see the docstring)
AMBIGUOUS_MAX = 1e-4        # largest fraction of a case's elements whose ReLU mask may fall on either side
TINY = 2.0 ** -126


_ON_DEVICE = False


def f64(t):
    t = t.detach().double()
    return t if _ON_DEVICE else t.cpu()


@contextlib.contextmanager
def on_device():
    """inside: the float64 evaluations stay on the device of their operands (the same torch operations in IEEE float64; for buffers of
    10^8 elements, where the host takes ~0.15 s per million).  A caller cross-checks a part against the host evaluation."""
    global _ON_DEVICE
    old, _ON_DEVICE = _ON_DEVICE, True
    try:
        yield
    finally:
        _ON_DEVICE = old


def f32(v):
    """a python scalar as the C ABI rounds it to float"""
    return float(torch.tensor(v, dtype=torch.float32))


def elem(name, got, want, e, out, family=None, alts=(), also=(), dims=('i',), raise_=True):
    """|got - want| <= 1/2 ulp_out(|want| + e) + e per element.  alts: further rounding models that count as a match in the bf16
    mismatch fraction.  also: (want, e) pairs of other acceptable values (an ambiguous ReLU mask): the smallest err / bound counts."""
    got, want = f64(got), f64(want)
    e = torch.as_tensor(e, dtype=torch.float64).expand_as(want)
    bound = 0.5 * ulp(want.abs() + e, out) + e + 1e-300
    err = (got - want).abs()
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))           # (inf == inf, NaN where NaN is due)
    err = torch.where(same, torch.zeros_like(err), err)
    match = got == rne(want, out)
    for w2, e2 in also:
        w2 = f64(w2)
        e2 = torch.as_tensor(e2, dtype=torch.float64).expand_as(want)
        b2 = 0.5 * ulp(w2.abs() + e2, out) + e2 + 1e-300
        err2 = (got - w2).abs()
        better = err2 / b2 < err / bound
        err, bound = torch.where(better, err2, err), torch.where(better, b2, bound)
        match = match | (got == rne(w2, out))
    for a in alts:
        match = match | (got == rne(f64(a), out))
    frac = float((~(match | same)).double().mean()) if out == 'bf16' else None
    return _finish(name, family, got, want, err, bound, frac, dims, raise_, PREFIX)


def exact(name, got, want, family=None):
    """bit-exact (NaN == NaN)"""
    got, want = f64(got), f64(want)
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if family is not None:
        _record(family, 0.0 if bool(same.all()) else math.inf, None, PREFIX)
    if not bool(same.all()):
        i = int(torch.argmax((~same).flatten().int()))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r want %r' % (
            name, int((~same).sum()), got.numel(), idx, float(got[idx]), float(want[idx])))


def sums(name, got, terms, mags=None, n=None, ops=2, old=None, family=None, raise_=True):
    """conv_bounds.check_sums with the fp32 chain length n; old: the destination before an accumulating call (one more term)"""
    terms = terms.double()
    mags = terms.abs() if mags is None else mags.double()
    n = terms.shape[0] if n is None else n
    if old is not None:
        o = f64(old)[None]
        terms, mags, n = torch.cat([terms, o]), torch.cat([mags, o.abs()]), n + 1
    return cb.check_sums(name, got, terms, mags, ops=ops, family=family, raise_=raise_, n=n, prefix=PREFIX)


def sum_bound(mags, n, ops=2):
    return gamma(n + ops) * mags.double().sum(0) + 1e-30


# ------------------------------------------------------------------------------------------------------ elementwise
def affine(x, s, b, r=None, relu=False):
    """(want, e) of act(x * s + b (+ r)); s, b broadcast over the last axis"""
    x, s, b = f64(x), f64(s), f64(b)
    lin, mag = x * s + b, (x * s).abs() + b.abs()
    e = 2 * U * mag
    if r is not None:
        r = f64(r)
        lin, e = lin + r, e + U * (mag + r.abs())
    return (lin.clamp_min(0) if relu else lin), e


# ------------------------------------------------------------------------------------------------------ pools
class Geo:
    def __init__(self, H, W, R, S, sh, sw, ph, pw, P=None, Q=None):
        self.H, self.W, self.R, self.S, self.sh, self.sw, self.ph, self.pw = H, W, R, S, sh, sw, ph, pw
        self.P = (H + 2 * ph - R) // sh + 1 if P is None else P
        self.Q = (W + 2 * pw - S) // sw + 1 if Q is None else Q

    def tap(self, r, s):
        """input rows / columns of tap (r, s) for every output row / column, and which are inside"""
        h = torch.arange(self.P) * self.sh - self.ph + r
        w = torch.arange(self.Q) * self.sw - self.pw + s
        return h, w, (h >= 0) & (h < self.H), (w >= 0) & (w < self.W)

    def gather(self, x, r, s):
        """x[N, H, W, C] -> values [N, P, Q, C] under tap (r, s) and the [P, Q] validity"""
        h, w, hv, wv = self.tap(r, s)
        v = x[:, h.clamp(0, self.H - 1)][:, :, w.clamp(0, self.W - 1)]
        return v, (hv[:, None] & wv[None, :])

    def scatter(self, t, r, s, out):
        """out[N, H, W, C] += t[N, P, Q, C] at the input pixel of tap (r, s) (indices of one tap are distinct)"""
        h, w, hv, wv = self.tap(r, s)
        pi, qi = torch.nonzero(hv)[:, 0], torch.nonzero(wv)[:, 0]
        if len(pi) and len(qi):
            out[:, h[pi][:, None], w[qi][None, :]] += t[:, pi][:, :, qi]

    @property
    def nback(self):
        return -(-self.R // self.sh) * -(-self.S // self.sw)


def maxpool_fwd(x, g, last_on_tie=False):
    """float64 values and arg-max (tap index r * S + s) by the rule of maxpool_fwd_kernel"""
    x = f64(x)
    N, _, _, C = x.shape
    best = torch.full((N, g.P, g.Q, C), -math.inf, dtype=torch.float64)
    bi = torch.zeros((N, g.P, g.Q, C), dtype=torch.int64)
    first = torch.ones((g.P, g.Q), dtype=torch.bool)
    for r in range(g.R):
        for s in range(g.S):
            v, ok = g.gather(x, r, s)
            okb = ok[None, :, :, None]
            take = okb & (first[None, :, :, None] | (v >= best if last_on_tie else v > best) | torch.isnan(v))
            best = torch.where(take, v, best)
            bi = torch.where(take, torch.full_like(bi, r * g.S + s), bi)
            first = first & ~ok
    return best, bi


def maxpool_bwd(dy, arg, g, N, C):
    """(ref, A, n): dx[n, h, w, c] = sum of the windows whose arg-max is this pixel"""
    dy, arg = f64(dy), arg.cpu().long()
    ref = torch.zeros((N, g.H, g.W, C), dtype=torch.float64)
    A = torch.zeros_like(ref)
    for r in range(g.R):
        for s in range(g.S):
            t = torch.where(arg == r * g.S + s, dy, torch.zeros(()).double())
            g.scatter(t, r, s, ref)
            g.scatter(t.abs(), r, s, A)
    return ref, A, g.nback


def avgpool_fwd(x, g):
    x = f64(x)
    ref = torch.zeros((x.shape[0], g.P, g.Q, x.shape[3]), dtype=torch.float64)
    A = torch.zeros_like(ref)
    for r in range(g.R):
        for s in range(g.S):
            v, ok = g.gather(x, r, s)
            v = torch.where(ok[None, :, :, None], v, torch.zeros(()).double())
            ref, A = ref + v, A + v.abs()
    rs = g.R * g.S
    return ref / rs, A / rs, rs + 2


def avgpool_bwd(dy, g, N, C):
    dy = f64(dy)
    ref = torch.zeros((N, g.H, g.W, C), dtype=torch.float64)
    A = torch.zeros_like(ref)
    for r in range(g.R):
        for s in range(g.S):
            g.scatter(dy, r, s, ref)
            g.scatter(dy.abs(), r, s, A)
    rs = g.R * g.S
    return ref / rs, A / rs, g.nback + 2


def check_sum(name, got, ref, A, n, out, old=None, family=None, dims=('n', 'h', 'w', 'c'), raise_=True):
    """an fp32 sum of n roundings' worth, stored once; old: the destination before an accumulating call"""
    ref, A = f64(ref), f64(A)
    if old is None:
        return elem(name, got, ref, gamma(n) * A, out, family, dims=dims, raise_=raise_)
    old = f64(old)
    return elem(name, got, old + ref, gamma(n + 1) * (A + old.abs()), out, family, dims=dims, raise_=raise_)


def check_avg_affine(name, got, x, g, s, b, relu, out, family=None, raise_=True):
    """avgpool3x3_affine: the average is rounded to the storage type before act(avg * s + b)"""
    avg, A, n = avgpool_fwd(x, g)
    e_avg = gamma(n) * A
    e_avg = e_avg + (0.5 * ulp(avg.abs() + e_avg, out))
    s, b = f64(s), f64(b)
    want, e = affine(avg, s, b, relu=relu)
    e = e + s.abs() * e_avg * (1 + 2 * U)
    alt, _ = affine(rne(avg, out), s, b, relu=relu)
    return elem(name, got, want, e, out, family, alts=(alt,), dims=('n', 'h', 'w', 'c'), raise_=raise_)


# ------------------------------------------------------------------------------------------------------ BatchNorm statistics
def finalize(part, M, eps, mom, gam, bet, rm, rv, prereduce=None):
    """part [rows, 2, C] fp32 as the kernel reads it.  prereduce: None = decide as the library does (rows > 1536).
    returns {name: (want, e)} for mean, invstd, scale, shift, running_mean, running_var, and the variance with its bound"""
    p = f64(part)
    rows = p.shape[0]
    pre = rows > 1536 if prereduce is None else prereduce
    S, Sa = p.sum(0), p.abs().sum(0)
    eS = rows * D * Sa + (U * Sa if pre else 0.0)
    eps, mom = f32(eps), f32(mom)
    gam, bet, rm, rv = f64(gam), f64(bet), f64(rm), f64(rv)
    mean, E2 = S[0] / M, S[1] / M
    var = (E2 - mean * mean).clamp_min(0)
    e_mean = 2 * U * mean.abs() + eS[0] / M
    e_var = eS[1] / M + 2 * mean.abs() * eS[0] / M + 4 * D * (E2 + mean * mean)
    invstd = 1 / torch.sqrt(var + eps)
    e_inv = (2 * U + e_var / (2 * (var + eps))) * invstd
    scale = gam * invstd
    e_scale = gam.abs() * e_inv + U * scale.abs()
    shift = bet - mean * scale
    e_shift = scale.abs() * e_mean + mean.abs() * e_scale + 2 * U * ((mean * scale).abs() + bet.abs())
    c1 = f32(1.0 - mom)                      # fl(1 - momentum): 1 and momentum are fp32 values, their difference is rounded once
    unb = M / (M - 1.0) if M > 1 else 1.0
    rmean = c1 * rm + mom * mean
    e_rmean = 2 * U * ((c1 * rm).abs() + (mom * mean).abs()) + mom * e_mean
    rvar = c1 * rv + mom * var * unb
    e_rvar = gamma(3) * ((c1 * rv).abs() + mom * var * unb) + mom * unb * e_var
    return {'mean': (mean, e_mean), 'invstd': (invstd, e_inv), 'scale': (scale, e_scale), 'shift': (shift, e_shift),
            'running_mean': (rmean, e_rmean), 'running_var': (rvar, e_rvar), 'var': (var, e_var)}


def finalize_eval(eps, gam, bet, rm, rv):
    eps = f32(eps)
    gam, bet, rm, rv = f64(gam), f64(bet), f64(rm), f64(rv)
    scale = gam / torch.sqrt(rv + eps)
    e_scale = 3 * U * scale.abs()
    shift = bet - rm * scale
    return {'scale': (scale, e_scale), 'shift': (shift, rm.abs() * e_scale + 2 * U * ((rm * scale).abs() + bet.abs()))}


def check_finalize(name, got, want, family=None, raise_=True):
    """got: {name: tensor}; want: from finalize().  returns the worst ratio"""
    worst = 0.0
    for k, t in got.items():
        w, e = want[k]
        worst = max(worst, elem('%s %s' % (name, k), t, w, e, 'f32', family, dims=('channel',), raise_=raise_).ratio)
    return worst


def check_stats(name, part, x, tile=1024, family=None, raise_=True):
    """bn_stats: part [rows, 2, C] against the stored values x [M, C]: every partial row, and the total"""
    x, p = f64(x), f64(part)
    worst = 0.0
    for r in range(p.shape[0]):
        blk = x[r * tile:(r + 1) * tile]
        worst = max(worst, sums('%s row %d sum' % (name, r), p[r, 0], blk, family=family, raise_=raise_).ratio)
        worst = max(worst, sums('%s row %d sumsq' % (name, r), p[r, 1], blk * blk, family=family, raise_=raise_).ratio)
    worst = max(worst, sums(name + ' sum', p.sum(0)[0], x, n=tile, family=family, raise_=raise_).ratio)
    worst = max(worst, sums(name + ' sumsq', p.sum(0)[1], x * x, n=tile, family=family, raise_=raise_).ratio)
    return worst


# ------------------------------------------------------------------------------------------------------ BatchNorm backward
class BnBwd:
    """float64 reference of one BatchNorm(+ReLU) backward.  x, dy [M, C]; gam, mean, invstd [C]; mask: 0 none, 1 from y > 0 (y given),
    2 recomputed from x * scale + shift > 0.  dz_abs / dz_ops: sum |terms| and extra roundings of a gathered dy (bn_bwd_maxpool)"""

    def __init__(self, x, dy, gam, mean, invstd, mask=0, y=None, scale=None, shift=None, dz_abs=None, dz_ops=0, tile=1024):
        x, dy = f64(x), f64(dy)
        self.x, self.M, self.tile = x, x.shape[0], min(tile, x.shape[0])
        self.gam, self.mean, self.invstd = f64(gam), f64(mean), f64(invstd)
        self.amb = torch.zeros_like(x, dtype=torch.bool)
        on = torch.ones_like(x, dtype=torch.bool)
        if mask == 1:
            on = f64(y) > 0
        elif mask == 2:
            sc, sh = f64(scale), f64(shift)
            pre = x * sc + sh
            on = pre > 0
            self.amb = pre.abs() <= 4 * U * ((x * sc).abs() + sh.abs())
        self.on, self.dy = on, dy
        self.dy_abs = dy.abs() if dz_abs is None else f64(dz_abs)
        self.dz_ops = dz_ops
        self.dz = torch.where(on, dy, torch.zeros(()).double())
        self.e_dz = torch.where(on | self.amb, gamma(dz_ops) * self.dy_abs, torch.zeros(()).double()) if dz_ops else torch.zeros_like(x)
        self.xhat = (x - self.mean) * self.invstd
        self.amb_frac = float(self.amb.double().mean())
        za = torch.where(on, self.dy_abs, torch.zeros(()).double())
        big = 1.0 / gamma(self.tile + 3 + dz_ops)                           # an ambiguous term joins the bound whole
        self.m1 = za + self.amb * self.dy_abs * big
        self.m2 = za * (x.abs() + self.mean.abs()) * self.invstd + self.amb * (self.dy_abs * self.xhat.abs()) * big
        self.dbeta, self.dgamma = self.dz.sum(0), (self.dz * self.xhat).sum(0)
        self.e_dbeta = sum_bound(self.m1, self.tile, 3 + dz_ops)
        self.e_dgamma = sum_bound(self.m2, self.tile, 3 + dz_ops)

    def use_partials(self, part):
        """bn_bwd_partials: the sums are the given partial rows [ntiles, 2, C] (sum dz, sum dz * xhat), added in double, rounded once"""
        p = f64(part)
        self.dbeta, self.dgamma = p.sum(0)[0], p.sum(0)[1]
        e = p.shape[0] * D * p.abs().sum(0)
        self.e_dbeta, self.e_dgamma = e[0] + U * self.dbeta.abs(), e[1] + U * self.dgamma.abs()
        return self

    def check_partial_params(self, name, dgamma, dbeta, old_dgamma=None, old_dbeta=None, family=None, raise_=True):
        for k, got, w, e, old in (('dbeta', dbeta, self.dbeta, self.e_dbeta, old_dbeta), ('dgamma', dgamma, self.dgamma, self.e_dgamma, old_dgamma)):
            if old is not None:
                e = e + U * (w.abs() + f64(old).abs())
                w = w + f64(old)
            elem('%s %s' % (name, k), got, w, e, 'f32', family, dims=('channel',), raise_=raise_)

    def check_params(self, name, dgamma, dbeta, old_dgamma=None, old_dbeta=None, family=None, raise_=True):
        assert self.amb_frac <= AMBIGUOUS_MAX, '%s: %.2e of the elements have an ambiguous ReLU mask' % (name, self.amb_frac)
        a = sums(name + ' dbeta', dbeta, self.dz, self.m1, n=self.tile, ops=3 + self.dz_ops, old=old_dbeta, family=family, raise_=raise_)
        b = sums(name + ' dgamma', dgamma, self.dz * self.xhat, self.m2, n=self.tile, ops=3 + self.dz_ops, old=old_dgamma, family=family,
                 raise_=raise_)
        return a, b

    def dx(self, dz):
        A = self.gam * self.invstd
        dg, db = self.dgamma / self.M, self.dbeta / self.M
        B = -A * self.invstd * dg
        T = self.mean * self.invstd * dg
        K = A * (T - db)
        want = A * dz + (B * self.x + K)
        e_B = gamma(5) * B.abs() + (A * self.invstd).abs() * self.e_dgamma / self.M
        e_K = A.abs() * (gamma(7) * (T.abs() + db.abs()) + (self.mean * self.invstd).abs() * self.e_dgamma / self.M + self.e_dbeta / self.M)
        inner = (B * self.x).abs() + K.abs()
        e = U * (A * dz).abs() + A.abs() * self.e_dz + e_B * self.x.abs() + e_K + 2 * U * inner + 2 * U * ((A * dz).abs() + inner)
        return want, e

    def check_dx(self, name, got, out, old=None, family=None, raise_=True):
        """got [M, C]; old: dx before the call when it accumulates (dres_accumulate bit 1)"""
        w, e = self.dx(self.dz)
        w2, e2 = self.dx(torch.where(self.amb, self.dy - self.dz, self.dz))        # the other side of an ambiguous mask
        if old is not None:
            o = f64(old)
            e, e2 = e + U * (w.abs() + e + o.abs()), e2 + U * (w2.abs() + e2 + o.abs())
            w, w2 = w + o, w2 + o
        also = ((w2, e2),) if bool(self.amb.any()) else ()
        return elem(name + ' dx', got, w, e, out, family, also=also, dims=('m', 'c'), raise_=raise_)

    def check_dres(self, name, got, out, old=None, family=None, raise_=True):
        w, w2 = self.dz, torch.where(self.amb, self.dy - self.dz, self.dz)
        e = torch.zeros_like(w)
        if old is not None:
            o = f64(old)
            e = U * (w.abs() + o.abs())
            w, w2 = w + o, w2 + o
        also = ((w2, e),) if bool(self.amb.any()) else ()
        return elem(name + ' dres', got, w, e, out, family, also=also, dims=('m', 'c'), raise_=raise_)


# ------------------------------------------------------------------------------------------------------ head
def gap(x, mask, keep_scale):
    """x [N, HW, C] -> (feat, A, n)"""
    x = f64(x)
    HW = x.shape[1]
    k = 1.0 if mask is None else f64(mask) * f32(keep_scale)
    return x.sum(1) / HW * k, x.abs().sum(1) / HW * k, HW + 3


def fc_fwd(feat, W, b):
    feat, W, b = f64(feat), f64(W), f64(b)
    return feat @ W.t() + b, feat.abs() @ W.abs().t() + b.abs(), W.shape[1] + 2


def fc_wgrad(dl, feat):
    dl, feat = f64(dl), f64(feat)
    return dl.t() @ feat, dl.abs().t() @ feat.abs(), dl.shape[0] + 2


def fc_bgrad(dl):
    dl = f64(dl)
    return dl.sum(0), dl.abs().sum(0), dl.shape[0] + 2


def head_dx(dl, W, mask, keep_scale, HW, C):
    """(ref, A, n) [N, C] of one pixel; every one of the HW copies holds it.  W None: the pooled-logits form"""
    dl = f64(dl)
    N, NC = dl.shape
    if W is None:
        g = torch.zeros((N, C), dtype=torch.float64)
        g[:, :NC] = dl
        a, n = g.abs(), 3
    else:
        W = f64(W)
        g, a, n = dl @ W, dl.abs() @ W.abs(), NC + 3
    k = 1.0 if mask is None else f64(mask) * f32(keep_scale)
    return g / HW * k, a / HW * k, n


# ------------------------------------------------------------------------------------------------------ softmax, cross-entropy
def softmax(logits, arg_term=True):
    """(p, e_p, parts); arg_term=False leaves the rounding of l_j - max out (test_op_bounds_cpu.py shows that it is needed)"""
    l = f64(logits)
    mx = l.max(1, keepdim=True).values
    d = l - mx
    ex = torch.exp(d)
    s = ex.sum(1, keepdim=True)
    p = ex / s
    NC = l.shape[1]
    rel = (U * d.abs() if arg_term else 0.0) + 2 * E_LIBM * U + gamma(NC) + 2 * U
    e_s = (ex * (U * d.abs() + E_LIBM * U)).sum(1, keepdim=True) + gamma(NC) * s
    return p, rel * p + TINY, (mx, s, e_s)


def xent(logits, target, weight, old_loss=None):
    """{'dlogits': (want, e), 'loss': (want, e)} of weight * mean cross-entropy"""
    l = f64(logits)
    N, NC = l.shape
    w = f32(weight)
    p, e_p, (mx, s, e_s) = softmax(l)
    oh = torch.zeros_like(p)
    oh[torch.arange(N), target.cpu().long()] = 1.0
    dl = w / N * (p - oh)
    e_dl = abs(w) / N * (e_p + U * (p + oh)) + 3 * U * dl.abs()
    lt = l[torch.arange(N), target.cpu().long()][:, None]
    li = mx + torch.log(s) - lt
    e_i = e_s / s * (1 + 2.0 ** -10) + E_LIBM * U * torch.log(s).abs() + 2 * U * (mx.abs() + torch.log(s).abs() + lt.abs())
    loss = w / N * li.sum()
    e = abs(w) / N * (gamma(N + 1) * li.abs().sum() + e_i.sum() * (1 + gamma(N + 1)))
    e = e + 3 * U * (loss.abs() + e)
    if old_loss is not None:
        e = e + U * (loss.abs() + e + abs(old_loss))
        loss = loss + old_loss
    return {'dlogits': (dl, e_dl), 'loss': (loss.reshape(1), e.reshape(1))}


# ------------------------------------------------------------------------------------------------------ optimizers
def _bias_correction(beta, step):
    bt = beta ** step
    bc = 1.0 - bt
    return bc, 2 * U * bt / bc + U


def adam(p, g, m, v, lr, b1, b2, eps, wd, step, gs):
    """one step from the fp32 state: {'p' | 'm' | 'v': (want, e)}"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    lr, b1, b2, eps, wd, gs = (f32(t) for t in (lr, b1, b2, eps, wd, gs))
    bc1, r1 = _bias_correction(b1, step)
    bc2, r2 = _bias_correction(b2, step)
    sbc2, rs2 = math.sqrt(bc2), r2 / 2 + U
    gr = g * gs + wd * p
    e_gr = gamma(2) * ((g * gs).abs() + (wd * p).abs())
    m2 = b1 * m + (1 - b1) * gr
    e_m = gamma(2) * (b1 * m).abs() + gamma(3) * (1 - b1) * gr.abs() + (1 - b1) * e_gr * (1 + gamma(3))
    v2 = b2 * v + (1 - b2) * gr * gr
    e_v = gamma(2) * (b2 * v).abs() + gamma(4) * (1 - b2) * gr * gr + (1 - b2) * (2 * gr.abs() * e_gr + e_gr * e_gr) * (1 + gamma(4))
    rv = torch.where(v2 > 0, e_v / v2.clamp_min(1e-300), torch.zeros(()).double()).clamp_max(0.5)
    r_sqrt = rv / (2 * (1 - rv)) + U
    a = torch.sqrt(v2) / sbc2
    r_a = r_sqrt + rs2 + U
    den = a + eps
    e_den = a * r_a + U * den
    r_d = e_den / den
    q = m2 / den
    e_q = (e_m + m2.abs() * r_d) / (den * (1 - r_d))
    e_q = e_q + U * (q.abs() + e_q)
    k = lr / bc1
    step_ = k * q
    e_step = abs(k) * (e_q * (1 + r1 + 3 * U) + q.abs() * (r1 + 2 * U))
    p2 = p - step_
    e_p = e_step + U * (p2.abs() + e_step)
    return {'p': (p2, e_p), 'm': (m2, e_m), 'v': (v2, e_v)}


def sgd(p, g, mom, lr, mu, wd, gs):
    p, g = f64(p), f64(g)
    lr, mu, wd, gs = (f32(t) for t in (lr, mu, wd, gs))
    gr = g * gs + wd * p
    e = gamma(2) * ((g * gs).abs() + (wd * p).abs())
    out = {}
    if mom is not None:
        mom = f64(mom)
        b = mu * mom + gr
        e = e + gamma(2) * ((mu * mom).abs() + gr.abs())
        out['mom'] = (b, e)
        gr = b
    p2 = p - lr * gr
    out['p'] = (p2, lr * e + 2 * U * (p.abs() + (lr * gr).abs()))
    return out


def check_dict(name, got, want, family=None, raise_=True):
    worst = 0.0
    for k, t in got.items():
        w, e = want[k]
        worst = max(worst, elem('%s %s' % (name, k), t, w, e, 'f32', family, raise_=raise_, dims=tuple('ijkl'[:max(1, w.dim())])).ratio)
    return worst
